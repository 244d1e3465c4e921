"""The yardstick of the subex tests: a NumPy transcription of the reference's cldfrac with
subex_cldfrac (Main/mod_micro_interface.F90:211-362, Main/cloudlib/mod_cloud_subex.F90:46-107;
ipptls = 1, icldfrac = 0, icldmstrat = 0) and subex (Main/microlib/mod_micro_subex.F90:99-393; the
non-aerosol dqc, l_lat_hack = .false., the idynamic 1 / 2 form), written from the Fortran text line
by line.  Arrays are (k, i, j) as in tests/tracer_ref.py; 2-D fields are (i, j).  A plain module
(nothing collected).

The oracle stubs the microphysics, so this transcription is the reference.  NumPy's elementwise
+ - * / and sqrt are the IEEE operations, one rounding each, in the order written.  The two
transcendental functions are arguments: pow10 (10**x of qcth, :163) and the chis table (its exp,
allocate_micro :117-120), so a test can hand over the values of the host-compiled header and
compare everything else bit for bit.
"""
from types import SimpleNamespace

import numpy as np

from tests import condtq_ref as cq

# Share/mod_constants.F90 (:44, 58, 68, 85, 182-183, 197, 371-372)
D_R1000, MINQC, DLOWVAL = 0.001, 1.0e-10, 1.0e-20
REGRAV = 1.0 / 9.80665
TZERO, RCPD = cq.TZERO, cq.RCPD
LOWCLD, HICLD = 0.0001, 0.9999
NCHI = 256                                             # Main/mod_micro_interface.F90:56
# Main/microlib/mod_micro_subex.F90:53-57
REMFRC, PPTMIN, ACTCLD, ACCRFRC = 0.0, 0.0, 0.0, 0.5


def params(rhmax=1.01, rhmin=0.01, tc0=238.0, larcticcorr=False, iconvlwp=1):
    """The run's scalars, with the defaults of Main/mod_params.F90:266, 331-335."""
    return SimpleNamespace(rhmax=rhmax, rhmin=rhmin, tc0=tc0, larcticcorr=bool(larcticcorr), iconvlwp=int(iconvlwp))


def pow10(x):
    return 10.0 ** np.asarray(x, dtype=np.float64)


def chis_table(exp=np.exp):
    """allocate_micro, :117-120."""
    cf = np.arange(NCHI, dtype=np.float64) / float(NCHI - 1)                  # :118
    return 0.97 * exp(-((cf - 0.098) * (cf - 0.098)) / 0.0365) + 0.255        # :119


def clwfromt(t):
    """Share/clwfromt.inc."""
    tcel = t - TZERO
    return np.where(tcel < -50.0, 0.001,
                    0.127 + 6.78e-03 * tcel + 1.29e-04 * (tcel * tcel) + 8.68e-07 * (tcel * tcel * tcel))


def qcth_arg(t):
    """The exponent of :163."""
    return -0.48911 + 0.01344 * (t - TZERO)


def cldfrac(t, p, qv, qc, rh, rho, rh0, cu_cldfra, cu_cldlwc, par, chis):
    """cldfrac for ipptls = 1 with subex_cldfrac.  t, p, qv, qc, rh, rho: mo2mc%t, phs, qvn, qcn,
    rh, rho (k, i, j); rh0 (i, j); cu_cldfra / cu_cldlwc: cldfra / cldlwc as cucloud left them.
    Returns fcc, cldfra, cldlwc, rh0adj and the branch masks."""
    with np.errstate(all="ignore"):
        totc = np.where(qc <= 1.0e-10, 0.0, qc)                               # :241, 249
        # subex_cldfrac, Main/cloudlib/mod_cloud_subex.F90:62-81
        gate = totc > 1.0e-7                                                  # :62
        rhrng = np.minimum(np.maximum(rh, par.rhmin), par.rhmax)              # :64
        warm = t > par.tc0                                                    # :65
        r0 = np.where(warm, rh0[None], 0.99999 - (1.0 - rh0[None]) / (1.0 + 0.15 * (par.tc0 - t)))   # :66-69
        none = rhrng <= r0                                                    # :71
        full = ~none & (rhrng > 0.99999)                                      # :73
        sund = ~none & ~full
        fcc = np.where(none, 0.0, np.where(full, 1.0, 1.0 - np.sqrt(np.where(sund, (1.0 - rhrng) / (1.0 - r0), 0.0))))
        fcc = np.where(gate, fcc, 0.0)                                        # :79-81
        arctic = np.zeros(fcc.shape, bool)
        if par.larcticcorr:                                                   # :92-105
            arctic = (p >= 75000.0) & (qv <= 0.003)
            fac = np.maximum(0.15, np.minimum(1.0, qv / 0.003))
            fcc = np.where(arctic, fcc * fac, fcc)
        hi_clamp = fcc > HICLD
        fcc = np.maximum(np.minimum(fcc, HICLD), 0.0)                         # Main/mod_micro_interface.F90:301
        # 2. the merge with the convective cloud, :314-348
        cloudy = fcc > LOWCLD                                                 # :317
        if par.iconvlwp == 1:
            ex = clwfromt(t)                                                  # :321
        else:
            ex = (totc * 1000.0) * rho                                        # :324
            ex = ex / np.where(cloudy, fcc, 1.0)                              # :326
        ichi = (np.where(cloudy, fcc, 0.0) * float(NCHI - 1)).astype(np.int64)    # :331
        ex = ex * chis[ichi]                                                  # :332
        exlwc = np.where(cloudy, ex, 0.0)                                     # :314
        conv = cu_cldfra > LOWCLD                                             # :334
        lwc_m = (exlwc * fcc + cu_cldlwc * cu_cldfra) / np.where(conv, cu_cldfra + fcc, 1.0)   # :336-338
        cldlwc = np.where(conv, lwc_m, exlwc)                                 # :342
        cldfra = np.where(conv, np.maximum(cu_cldfra, fcc), fcc)              # :339, 341
        wet = cldlwc > 0.0                                                    # :344
        cldfra = np.where(wet, np.minimum(np.maximum(cldfra, 0.0), HICLD), 0.0)   # :345-347
        rh0adj = 1.0 - (1.0 - rh) / ((1.0 - cldfra) * (1.0 - cldfra))         # :354
        rh0adj = np.maximum(0.0, np.minimum(rh0adj, 0.99999))                 # :355
    return dict(fcc=fcc, cldfra=cldfra, cldlwc=cldlwc, rh0adj=rh0adj, totc=totc, ichi=ichi, gate=gate,
                warm=gate & warm, cold=gate & ~warm, none=gate & none, full=gate & full, sund=gate & sund,
                arctic=arctic, arctic_lo=arctic & (qv / 0.003 < 0.15), arctic_hi=arctic & (qv / 0.003 >= 1.0),
                hi_clamp=hi_clamp, cloudy=cloudy, conv=conv, wet=wet)


def subex(fcc, t, p, pf, qv, qc, rh, rho, psb, qck1, cgul, cevap, caccr, dt, dtsec, par, rainnc, lsmrnc, trrate,
          pow10=pow10, rem=False):
    """subex.  fcc: mc2mo%fcc of cldfrac; t, p, qv, qc, rh, rho as in cldfrac; pf: mo2mc%pfs (kz + 1,
    i, j); psb and the tables (i, j); rainnc, lsmrnc, trrate: the accumulators before the call.
    Returns the three coupled increments on a zero tendency (lsc_t, lsc_qv, lsc_qc), the new
    rainnc / lsmrnc / trrate, dqc, qcth, remrat / rembc (with rem), and the branch masks."""
    kz = t.shape[0]
    z3 = np.zeros(t.shape)
    with np.errstate(all="ignore"):
        # 0. dqc, :147-173
        cloud = (qc > MINQC) & (fcc > ACTCLD)                                 # :158
        safe = np.where(cloud, fcc, 1.0)
        qcincl = qc / safe                                                    # :160
        qcth = cgul[None] * pow10(qcth_arg(t)) * D_R1000                      # :161-163
        dqc = np.where(cloud, np.maximum(qcincl - qcth, 0.0), 0.0)            # :167, 169
        lsc_t, lsc_qv, lsc_qc, remrat, rembc = z3.copy(), z3.copy(), z3.copy(), z3.copy(), z3.copy()
        m = {n: np.zeros(t.shape, bool) for n in (
            "rains", "pptmax_auto", "pptmax_acc", "evap", "lim_dqv", "lim_km1", "lim_none", "evap_gate", "floor",
            "dqv_neg", "noppt")}
        m["cloud"] = cloud
        seen = np.zeros(psb.shape, bool)          # the column carried rain at some level
        # 1a. the top layer, :196-240
        afc, qcw = fcc[0], qc[0]
        c0 = cloud[0]
        pptmax = (1.0 - REMFRC) * qcw / dt                                    # :200
        auto = qck1 * dqc[0] * afc
        pptnew = np.minimum(pptmax, auto)                                     # :204
        m["pptmax_auto"][0] = c0 & (auto > pptmax)
        qcleft = np.maximum(qcw - pptnew * dt, 0.0)                           # :210
        pptkm1 = ACCRFRC * pptnew / np.where(c0, afc, 1.0) * rho[0] * dt      # :212
        pptacc = caccr * qcleft * pptkm1                                      # :214
        m["pptmax_acc"][0] = c0 & (pptacc + pptnew > pptmax) & ~(auto > pptmax)
        pptnew = np.minimum(pptmax, pptacc + pptnew)                          # :217
        new = c0 & (pptnew > PPTMIN)                                          # :219
        dpovg = (pf[1] - pf[0]) * REGRAV                                      # :220
        pptsum = np.where(new, pptnew * dpovg, 0.0)                           # :185, 221
        lsc_qc[0] = np.where(new, 0.0 - pptnew * psb, 0.0)                    # :229-230
        remrat[0] = np.where(new, pptnew / np.where(new, qcw, 1.0), 0.0)      # :234
        m["rains"][0] = new
        seen |= pptsum > 0.0
        # 1b. the second layer to the surface, :247-348
        for k in range(1, kz):
            dpovg = (pf[k + 1] - pf[k]) * REGRAV                              # :252
            afc, qcw = fcc[k], qc[k]                                          # :253-254
            above = pptsum > 0.0                                              # :256
            pptkm1 = np.where(above, pptsum / dpovg, 0.0)                     # :257, 259
            has = pptkm1 > PPTMIN                                             # :266
            m["noppt"][k] = ~has
            qs = cq.pfwsat(t[k], p[k])                                        # :267
            dqv = (qs - qv[k]) / dt                                           # :268
            pos = has & (dqv > 0.0)                                           # :269
            m["dqv_neg"][k] = has & ~(dqv > 0.0)
            rhcs = (rh[k] - afc * par.rhmax) / (1.0 - afc)                    # :271
            rhcs = np.maximum(np.minimum(rhcs, par.rhmax), par.rhmin)         # :272
            r0 = cevap * (par.rhmax - rhcs) * np.sqrt(np.where(above, pptsum, 0.0)) * (1.0 - afc)   # :274
            r1 = np.minimum(r0, dqv)                                          # :275
            rdevap = np.minimum(r1, pptkm1)                                   # :276
            ev = pos & (rdevap > DLOWVAL)                                     # :279
            m["evap_gate"][k] = pos & ~(rdevap > DLOWVAL)
            m["lim_km1"][k] = ev & (r1 > pptkm1)
            m["lim_dqv"][k] = ev & ~(r1 > pptkm1) & (r0 > dqv)
            m["lim_none"][k] = ev & ~(r1 > pptkm1) & ~(r0 > dqv)
            left = pptsum - rdevap * dpovg
            m["floor"][k] = ev & (left <= 0.0)
            pptsum = np.where(ev, np.maximum(left, 0.0), pptsum)              # :280
            pptkm1 = np.where(ev, pptkm1 - rdevap, pptkm1)                    # :281
            lsc_qv[k] = np.where(ev, 0.0 + rdevap * psb, 0.0)                 # :293-294
            lsc_t[k] = np.where(ev, 0.0 - cq.wlh(t[k]) * RCPD * rdevap * psb, 0.0)   # :297-298
            m["evap"][k] = ev
            # 1bd. autoconversion and accretion, :304-345
            ck = cloud[k]
            pptmax = (1.0 - REMFRC) * qcw / dt                                # :305
            auto = qck1 * dqc[k] * afc
            pptnew = np.minimum(pptmax, auto)                                 # :309
            m["pptmax_auto"][k] = ck & (auto > pptmax)
            qcleft = np.maximum(qcw - pptnew * dt, 0.0)                       # :314
            km1 = (pptkm1 + ACCRFRC * pptnew / np.where(ck, afc, 1.0)) * rho[k] * dt   # :318
            pptacc = caccr * qcleft * km1                                     # :320
            m["pptmax_acc"][k] = ck & (pptacc + pptnew > pptmax) & ~(auto > pptmax)
            pptnew = np.minimum(pptmax, pptacc + pptnew)                      # :323
            new = ck & (pptnew > PPTMIN)                                      # :324
            pptsum = np.where(new, pptsum + pptnew * dpovg, pptsum)           # :326
            lsc_qc[k] = np.where(new, 0.0 - pptnew * psb, 0.0)                # :334-335
            remrat[k] = np.where(new, pptnew / np.where(new, qcw, 1.0), 0.0)  # :339
            m["rains"][k] = new
            seen |= pptsum > 0.0
        # 2. the below-cloud removal, :359-376
        if rem:
            for k in range(1, kz):
                acc = np.zeros(psb.shape)                                     # :365
                for kk in range(k):                                           # :367
                    acc = acc + remrat[kk] * qc[k] * (pf[k + 1] - pf[k]) * REGRAV    # :369-371
                rembc[k] = np.where(remrat[k] > 0.0, acc, 0.0)                # :366
        # 3. the surface, :384-393
        prainx = pptsum * dtsec                                               # :386
        wet = prainx > DLOWVAL                                                # :387
        out = dict(lsc_t=lsc_t, lsc_qv=lsc_qv, lsc_qc=lsc_qc, dqc=dqc, qcth=qcth, pptsum=pptsum, prainx=prainx,
                   rainnc=np.where(wet, rainnc + prainx, rainnc),             # :388
                   lsmrnc=np.where(wet, lsmrnc + pptsum, lsmrnc),             # :389
                   trrate=np.where(wet, pptsum, trrate),                      # :390
                   surface=wet, dry_surface=~wet, lost_all=seen & ~wet, masks=m)
        if rem:
            out.update(remrat=remrat, rembc=rembc)
    return out


# ------------------------------------------------------------------ synthetic inputs of the GPU tests
# the patch of the arctic correction's points: rows, columns (inside the interior of every test grid)
ARCTIC = (slice(14, 20), slice(12, 20))


def tables(rc, seed=17):
    """The five 2-D tables (Main/mod_params.F90:2455-2480): the land / ocean values in a
    checkerboard of 5 x 7 patches; strips with a raindrop evaporation coefficient large enough for
    rain to evaporate within one level, and with none (rdevap = 0: the dlowval gate); rows with an
    autoconversion rate and rows with an accretion rate that run into pptmax; and over the ARCTIC
    patch a threshold rh0 low enough for cloud in the cold-dry air rainy_state puts there."""
    ii, jj = np.meshgrid(np.arange(rc.iy), np.arange(rc.jx), indexing="ij")
    land = ((ii // 5 + jj // 7) % 2) == 0
    tab = dict(RH0=np.where(land, 0.80, 0.90), QCK1=np.where(land, 0.0005, 0.0005), CGUL=np.where(land, 0.65, 0.30),
               CEVAP=np.where(land, 1.0e-5, 1.0e-5), CACCR=np.where(land, 6.0, 4.0))
    tab["CEVAP"] = np.where(jj % 9 < 3, 2.0e-3, tab["CEVAP"])
    tab["CEVAP"] = np.where(jj % 9 == 4, 0.0, tab["CEVAP"])       # cevap = max(cevap, 0), :2106-2108
    tab["QCK1"] = np.where(ii % 11 < 2, 0.5, tab["QCK1"])         # autoconversion up against pptmax
    tab["CACCR"] = np.where(ii % 7 == 3, 5.0e4, tab["CACCR"])     # accretion up against pptmax
    tab["RH0"][ARCTIC] = 0.02
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in tab.items()}


def _coupled_exactly(q, ps):
    """c with (c * (1 / ps)) == q where one of q * ps and its two neighbours gives it, else q * ps:
    mkslice decouples with the reciprocal of p*."""
    r = 1.0 / ps
    c0 = q * ps
    out = c0.copy()
    for c in (np.nextafter(c0, np.inf), np.nextafter(c0, -np.inf), c0):
        out = np.where(c * r == q, c, out)
    return out


def rainy_state(rc, st, seed=5):
    """condtq_ref.moist_state with columns that rain: its cloud patches keep their water in the
    upper two thirds of the column on even patches (so rain falls through clear, partly dry air and
    evaporates, entirely in places) and everywhere on odd ones (rain reaches the surface), with
    some cloud water tiny enough for the minqc / 1e-7 / 1e-10 gates.  Over the ARCTIC patch the
    four lowest levels (p >= 75000 Pa) hold cloud in dry air: qv under 0.15 * 0.003, between, and
    0.003 itself (the arctic factor's two clamps; tables() lowers rh0 there so fcc > 0)."""
    s = cq.moist_state(rc, st, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 100))
    psb = s["PSB"][0]
    with np.errstate(all="ignore"):
        qc = np.nan_to_num(s["ATM2_QC"] / psb, nan=0.0, posinf=0.0, neginf=0.0)
    kz = rc.kz
    kcut = (2 * kz) // 3
    ii, jj = np.meshgrid(np.arange(rc.iy), np.arange(rc.jx), indexing="ij")
    upper_only = ((ii // 3 + jj // 3) % 2) == 0
    qc[kcut:] = np.where(upper_only[None], 0.0, qc[kcut:])
    qc[:, :, 5::7] *= 1.0e-4                     # 2e-8 .. : under 1e-7, above minqc
    qc[:, 4::9, :] *= 1.0e-7                     # 2e-11 .. : under 1e-10
    low = (slice(kz - 4, kz),) + ARCTIC
    qc[low] = 1.0e-4
    nj = ARCTIC[1].stop - ARCTIC[1].start
    qv = rng.uniform(1.0e-5, 4.0e-4, qc[low].shape)          # qv / 0.003 < 0.15
    qv[:, :, nj // 3:2 * nj // 3] = rng.uniform(6.0e-4, 2.9e-3, qv[:, :, nj // 3:2 * nj // 3].shape)
    qv[:, :, 2 * nj // 3:] = 0.003                           # qv / 0.003 = 1
    for lev, ps in (("ATM1", "PSA"), ("ATM2", "PSB")):
        s[lev + "_QC"] = qc * s[ps][0]
        s[lev + "_QV"][low] = _coupled_exactly(qv, np.broadcast_to(s[ps][0][ARCTIC], qv.shape))
    return s


def cucloud(rc, seed=23):
    """A convective cloud (cldfra, cldlwc) that populates both merge branches: towers over a few
    patches, none elsewhere, with fractions up to cucloud's cap."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fra = np.zeros((rc.kz, rc.iy, rc.jx))
    lwc = np.zeros_like(fra)
    for (i0, j0) in ((3, 3), (10, 18), (18, 9)):
        blk = (slice(2, rc.kz - 2), slice(i0, i0 + 7), slice(j0, j0 + 8))
        fra[blk] = rng.uniform(0.0, 0.8, fra[blk].shape)
        lwc[blk] = 0.3
    fra[:, 6, :] = np.where(fra[:, 6, :] > 0, 0.00005, 0.0)      # at most lowcld: the large-scale cloud alone
    return fra, lwc


def host_slice(rc, st):
    """The mkslice fields subex reads (Main/mod_slice.F90:185-252, 331-338), formed in NumPy from a
    state: what the device's export holds at the first tend, to rounding.  For the CPU-side check
    of the GPU tests' inputs only."""
    rgas = cq.RGAS
    with np.errstate(all="ignore"):
        psb = st["PSB"][0]
        rpsb = 1.0 / psb
        tb = st["ATM2_T"] * rpsb
        qv = np.maximum(st["ATM2_QV"] * rpsb, cq.MINQQ)
        qc = np.maximum(st["ATM2_QC"] * rpsb, 0.0)
        sig = np.asarray(rc.sigma, dtype=np.float64)
        if rc.idynamic == 2:
            ppb = st["ATM2_PP"] * rpsb
            pb = st["ATM0_PR"] + ppb
            pb[0] = np.maximum(pb[0], rc.ptop * 1000.0 + 1.0)
            pf = np.array(st["ATM0_PF"], dtype=np.float64)
            pf[0] = rc.ptop * 1000.0
            pf[rc.kz] = st["ATM0_PS"][0] + rc.ptop * 1000.0 + ppb[rc.kz - 1]
            pf[1:rc.kz] = st["ATM0_PF"][1:rc.kz] + 0.5 * (ppb[:-1] + ppb[1:])
        else:
            pb = (cq.hsigma(rc)[:, None, None] * psb + rc.ptop) * 1000.0
            pf = (sig[:rc.kz + 1, None, None] * psb + rc.ptop) * 1000.0
        qs = cq.pfwsat(tb, pb)
        rh = np.minimum(np.maximum(qv / qs, rc.rhmin), rc.rhmax)
        f = dict(t=tb, p=pb, pf=pf, qv=qv, qc=qc, rho=pb / (rgas * tb), rh=rh, psb=psb)
    return {k: np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0) for k, v in f.items()}


def slice_inputs(get, psb):
    """The mkslice fields the device reads, from an engine's get: a dict for cldfrac / subex."""
    return dict(t=get("ATMS_TB3D"), p=get("ATMS_PB3D"), pf=get("ATMS_PF3D"), qv=get("ATMS_QVB3D"),
                qc=get("ATMS_QCB3D"), rho=get("ATMS_RHOB3D"), rh=get("ATMS_RHB3D"), psb=psb)


def run(f, tab, par, dt, dtsec, chis, pow10=pow10, cu=None, acc=None, rem=False):
    """cldfrac then subex on the inputs f (slice_inputs) over whole (k, i, j) arrays; cu: (cldfra,
    cldlwc) of cucloud or None; acc: dict RAINNC / LSMRNC / TRRATE (i, j) or None for zeros."""
    shp2 = f["psb"].shape
    cufra, culwc = cu if cu is not None else (np.zeros(f["t"].shape), np.zeros(f["t"].shape))
    acc = acc or {n: np.zeros(shp2) for n in ("RAINNC", "LSMRNC", "TRRATE")}
    c = cldfrac(f["t"], f["p"], f["qv"], f["qc"], f["rh"], f["rho"], tab["RH0"], cufra, culwc, par, chis)
    s = subex(c["fcc"], f["t"], f["p"], f["pf"], f["qv"], f["qc"], f["rh"], f["rho"], f["psb"], tab["QCK1"], tab["CGUL"],
              tab["CEVAP"], tab["CACCR"], dt, dtsec, par, acc["RAINNC"], acc["LSMRNC"], acc["TRRATE"], pow10=pow10,
              rem=rem)
    return c, s
