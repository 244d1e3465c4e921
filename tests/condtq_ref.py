"""The yardstick of the condtq tests: a NumPy transcription of the reference's condtq
(Main/mod_micro_interface.F90:407-482, the idynamic /= 3 branch) with pfesat / pfwsat / wlh
(Share/pfesat.inc, Share/pfwsat.inc, Share/wlh.inc), written from the Fortran text line by line,
and the two-pass oracle built on it.  A plain module (nothing collected).

The oracle stubs condtq (it adds + 0.0 where the reference calls it) but accepts TPHY / QVPHY /
QCPHY.  With no host physics tendencies ((x + 0) + d) and (x + (0 + d)) are the same bits, so a
probe oracle P that runs tend from the state and clock of the real oracle R, the transcription on
P's totals, and R's tend with the three increments put as TPHY / QVPHY / QCPHY is the reference's
tend with condtq.  NumPy's elementwise + - * / and sqrt are the IEEE operations, one rounding
each, in the order written: the transcription rounds as the Fortran text does.
"""
import numpy as np

# Share/mod_constants.F90 (:57, 68, 92-94, 107-109, 130-144, 183, 197, 306)
MINQQ, DLOWVAL = 1.0e-8, 1.0e-20
TZERO = 273.15
AMD, AMW = 28.96454, 18.01528
RGASMOL = 6.02214129e23 * 1.3806504e-23
RGAS = (RGASMOL / AMD) * 1000.0
RWAT = (RGASMOL / AMW) * 1000.0
CPD = 3.5 * RGAS
RCPD = 1.0 / CPD
EP2 = AMW / AMD
RH0MAX = 0.99999          # cldfrac's upper clamp of rh0adj (:355), condtq's high-cover threshold (:447)

_A = (6.11213476, 0.444007856, 0.143064234e-01, 0.264461437e-03, 0.305903558e-05,
      0.196237241e-07, 0.892344772e-10, -0.373208410e-12, 0.209339997e-15)
_C = (6.11123516, 0.503109514, 0.188369801e-01, 0.420547422e-03, 0.614396778e-05,
      0.602780717e-07, 0.387940929e-09, 0.149436277e-11, 0.262655803e-14)


def pfesat(t):
    """Share/pfesat.inc: t_limit clamped to [-75, 100], the two Horner forms, es in Pa."""
    td = np.asarray(t, dtype=np.float64) - TZERO
    td = np.where(td > 100.0, 100.0, td)
    td = np.where(td < -75.0, -75.0, td)

    def horner(c):
        return c[0] + td * (c[1] + td * (c[2] + td * (c[3] + td * (c[4] + td * (c[5] + td * (c[6] + td * (c[7] + td * c[8])))))))
    return np.where(td >= 0.0, horner(_A), horner(_C)) * 100.0, td


def pfwsat(t, p):
    """Share/pfwsat.inc: ws = ep2 * (es / (p - es))."""
    es, _ = pfesat(t)
    return EP2 * (es / (p - es))


def wlh(t):
    """Share/wlh.inc, with its tc*tc*tc association and the * 1.0e3."""
    tc = np.asarray(t, dtype=np.float64) - TZERO
    warm = 2500.79 - 2.36418 * tc + 1.58927e-3 * tc * tc - 6.14342e-5 * tc * tc * tc
    cold = 2834.1 - 0.29 * tc - 0.004 * tc * tc
    return np.where(tc > 0.0, warm, cold) * 1.0e3


def condtq(t2, qv2, qc2, tt, tqv, tqc, psc, pres, qs, rh0adj, dt, conf):
    """:407-482 on arrays (psc broadcasts).  Returns a dict: tmp2, wwlh, the coupled increments
    it / iqv / iqc (zero where |tmp2| <= dlowval), rhc, and the branch masks."""
    with np.errstate(all="ignore"):
        tmp3 = (t2 + dt * tt) / psc                                  # :407
        qvcs = qv2 + dt * tqv                                        # :408
        qccs = qc2 + dt * tqc                                        # :409
        qvc_cld = np.maximum(qs, 0.0)                                # :410-411, mc2mo%qxten = 0
        clamp_qv = qvcs < MINQQ * psc                                # :418-420
        qvcs = np.where(clamp_qv, MINQQ * psc, qvcs)
        clamp_qc = qccs < DLOWVAL * psc                              # :421-423
        qccs = np.where(clamp_qc, 0.0, qccs)
        qvcs = qvcs / psc                                            # :424
        qccs = qccs / psc                                            # :425
        es, td = pfesat(tmp3)
        qvs = EP2 * (es / (pres - es))                               # :440
        wwlh = wlh(tmp3)                                             # :441
        r1 = 1.0 / (1.0 + wwlh * wwlh * qvs / (RWAT * CPD * tmp3 * tmp3))    # :442
        rhc = np.minimum(np.maximum(qvcs / qvs, 0.0), 1.0)           # :443
        low = rhc < rh0adj                                           # :445
        high = ~low & (rhc > RH0MAX)                                 # :447
        part = ~low & ~high
        fccc = 1.0 - np.sqrt(np.where(part, (1.0 - rhc) / (1.0 - rh0adj), 0.0))   # :450
        fccc = np.minimum(np.maximum(fccc, 0.0), 1.0)                # :451
        dqv = np.where(part, conf * fccc * (qvc_cld - qvs), conf * (qvcs - qvs))  # :446, 448, 453
        tmp1 = r1 * dqv                                              # :457
        exces = qccs + tmp1                                          # :460
        left = exces >= 0.0
        tmp2 = np.where(left, tmp1 / dt, -qccs / dt)                 # :461-465
        on = np.abs(tmp2) > DLOWVAL                                  # :469
        iqv = np.where(on, 0.0 - psc * tmp2, 0.0)                    # :475-476
        iqc = np.where(on, 0.0 + psc * tmp2, 0.0)                    # :477-478
        it = np.where(on, 0.0 + psc * tmp2 * wwlh * RCPD, 0.0)       # :479-480
    return dict(tmp2=tmp2, wwlh=wwlh, it=it, iqv=iqv, iqc=iqc, rhc=rhc, low=low, high=high, part=part,
                left=left, on=on, clamp_qv=clamp_qv, clamp_qc=clamp_qc, tc=tmp3 - TZERO, td=td,
                near=np.minimum(np.abs(rhc - rh0adj), np.abs(rhc - RH0MAX)) < 1e-9)


# ------------------------------------------------------------------ synthetic inputs of the GPU tests
def interior(rc):
    """The interior cross points jci1:jci2 x ici1:ici2 of the whole grid as array slices (a band,
    periodic in j, takes every column)."""
    return (slice(None), slice(1, rc.iy - 2), slice(0, rc.jx) if rc.i_band else slice(1, rc.jx - 2))


def rh0adj_field(rc, seed=11):
    """Continuous random in [0, 0.99999], with patches pinned to both ends."""
    rng = np.random.Generator(np.random.PCG64(seed))
    r = rng.uniform(0.0, RH0MAX, (rc.kz, rc.iy, rc.jx))
    r[:, 3:7, 4:10] = 0.0
    r[:, rc.iy - 9:rc.iy - 5, rc.jx - 12:rc.jx - 6] = RH0MAX
    return np.minimum(r, RH0MAX)


def hsigma(rc):
    s = np.asarray(rc.sigma, dtype=np.float64)
    return (s[1:rc.kz + 1] + s[:rc.kz]) * 0.5


def qsb3d(rc, st):
    """atms%qsb3d as mkslice forms it (Main/mod_slice.F90:185-228, 331-333) from a state:
    pfwsat(atm2%t / psb, pb3d), the NH pb3d with its k = 1 floor."""
    with np.errstate(all="ignore"):          # the cross grid's unused last row and column hold p* = 0
        rpsb = 1.0 / st["PSB"][0]
        tb = st["ATM2_T"] * rpsb
        if rc.idynamic == 2:
            pb = st["ATM0_PR"] + st["ATM2_PP"] * rpsb
            pb[0] = np.maximum(pb[0], rc.ptop * 1000.0 + 1.0)
        else:
            pb = (hsigma(rc)[:, None, None] * st["PSB"][0] + rc.ptop) * 1000.0
        return np.nan_to_num(pfwsat(tb, pb), nan=0.0, posinf=0.0, neginf=0.0)


def moist_state(rc, state, seed=5):
    """The case's state with its moisture rescaled: qv at a smooth target rh of about 0.2 - 1.15
    times qsb3d, qc patches that straddle the dry and the saturated regions."""
    rng = np.random.Generator(np.random.PCG64(seed))
    st = {k: v.copy() for k, v in state.items()}
    qs = qsb3d(rc, st)
    ii, jj = np.meshgrid(np.arange(rc.iy), np.arange(rc.jx), indexing="ij")
    kk = np.arange(rc.kz)[:, None, None]
    rh = 0.675 + 0.475 * np.sin(2.0 * np.pi * (jj / 17.0 + kk / 7.0)) * np.cos(2.0 * np.pi * ii / 13.0)
    rh = rh + 0.02 * rng.standard_normal(rh.shape)
    rh = np.clip(rh, 0.2, 1.15)
    qv = np.maximum(rh * qs, 1.0e-7)
    qc = np.zeros_like(qv)
    for (i0, j0) in ((2, 2), (2, 20), (12, 8), (12, 26), (20, 14), (20, 30)):
        qc[:, i0:i0 + 6, j0:j0 + 6] = 2.0e-4 * rng.uniform(0.2, 1.0, qc[:, i0:i0 + 6, j0:j0 + 6].shape)
    if rc.i_band:                            # cloud across the seam of the period, on both sides
        for js in (slice(0, 3), slice(rc.jx - 3, rc.jx)):
            qc[:, 5:23, js] = 2.0e-4 * rng.uniform(0.2, 1.0, qc[:, 5:23, js].shape)
    for lev, ps in (("ATM1", "PSA"), ("ATM2", "PSB")):
        st[lev + "_QV"] = qv * st[ps][0]
        st[lev + "_QC"] = qc * st[ps][0]
    return st


# ------------------------------------------------------------------ the two-pass oracle
class TwoPass:
    """The reference's tend with condtq, step by step.  make() gives a fresh oracle at the start
    state (after its initial bdyval).  An oracle keeps more than the prognostic fields (bdyval's
    boundary slices, which decouple reads), so the probe of a step is not a copy of R: it is a
    fresh oracle that replays R's history, the recorded increments put before each step, and then
    runs the step to be probed with zero increments.  tend's diagnostics (TTEN .., PSC,
    ATMS_QSB3D, the NH work array ppten) still hold that tend's values after the step's bdyval.
    sfs%psc of the NH core is sfs%psa (Main/mod_atm_interface.F90:890); its total of ppten is
    recovered from the work array, which tend decoupled by 1 / psa (:497) and sound scaled by its
    sub-step: two roundings on a term of a few Pa beside atm0%pr of 1e4 - 1e5 Pa, so pres keeps
    its bits but for the rare point at a rounding boundary."""

    PHY = (("it", "TPHY"), ("iqv", "QVPHY"), ("iqc", "QCPHY"))

    def __init__(self, make, rc, names, rh0adj, conf=1.0, probe=None):
        """probe: another factory for the probe of the first step, the only one then allowed.  With
        the NH Rayleigh damping on (ifrayd = 1) the oracle's TTEN, QVTEN and ppten hold the totals
        after the damping (Main/mod_tendency.F90:356-364, 466-470), while condtq reads them
        before it; the damping adds tau * (bdy - atm2) and reads no tendency, so a probe with
        ifrayd = 0 from the same start state holds exactly the totals condtq sees."""
        self.make, self.rc, self.names, self.rh0adj, self.conf = make, rc, names, rh0adj, conf
        self.probe = probe
        self.R = make()
        self.hist = []

    def _put(self, o, inc):
        for _, name in self.PHY:
            o.put(name, inc[name] if inc else np.zeros((self.rc.kz, self.rc.iy, self.rc.jx)))

    def step(self):
        """One tend + bdyval of R; returns the increments and the transcription's record."""
        rc, R = self.rc, self.R
        assert not (self.probe and self.hist), "a probe of its own serves the first step only"
        P = (self.probe or self.make)()
        for inc in self.hist:
            self._put(P, inc)
            P.step(1)
        before = {n: P.get(n) for n in self.names}
        for n in self.names:                      # the probe stands where R stands
            assert np.array_equal(before[n], R.get(n), equal_nan=True), n
        assert P.get_time() == R.get_time()
        lcount, dt, _ = P.get_time()
        self._put(P, None)
        P.step(1)
        c = interior(rc)
        with np.errstate(all="ignore"):           # the cross grid's unused last row and column
            if rc.idynamic == 2:
                psc = before["PSA"][0]
                # the work array after the step: (total / psa) * dts, dts = dt / istep of sound
                # (Main/mod_sound.F90:163-245; the clock is the one before the tend)
                istep = max(int(dt / P.cfg.nh_dtsmax), 2)
                if lcount > 0:
                    istep = max(istep, 4)
                pt = P.get_work("ppten") / (dt / istep) * before["PSA"][0]
                pres = P.get("ATM0_PR") + (before["ATM2_PP"] + dt * pt) / psc
            else:
                psc = P.get("PSC")[0]
                pres = (hsigma(rc)[:, None, None] * psc + rc.ptop) * 1000.0
        out = condtq(before["ATM2_T"][c], before["ATM2_QV"][c], before["ATM2_QC"][c], P.get("TTEN")[c],
                     P.get("QVTEN")[c], P.get("QCTEN")[c], psc[c[1:]], pres[c], P.get("ATMS_QSB3D")[c],
                     self.rh0adj[c], dt, self.conf)
        inc = {}
        for key, name in self.PHY:
            a = np.zeros((rc.kz, rc.iy, rc.jx))
            a[c] = out[key]
            inc[name] = a
        self._put(R, inc)
        R.step(1)
        self.hist.append(inc)
        return inc, out
