"""A NumPy statement of the reference's chain of one chemical tracer through one tend and one bdyval
of either core on one limited-area tile (ichem = 1, ichebdy = 1), written from the Fortran text.  The
two cores differ for a tracer only in the diffusion coefficient they hand it (the non-hydrostatic
calc_coeff is restated in tests/dyn_ref.py, nh_xkc) and in gnu2: the NH adiabatic term atmx%qx * cr runs over
n = 1..nqx only (Main/mod_tendency.F90:1615-1617).  Test infrastructure: tests/test_tracers_gpu.py compares the engine with it bit for bit,
tests/test_tracers_cpu.py checks its own vectorised negative-value fix against a plain triple loop.

Every expression keeps the operation order of the text (left to right, the parentheses of the
source), in float64; the chain has no transcendental function, so NumPy's elementwise operations
round as the Fortran does.

  decoupling       atmx%chi = atm1%chi * rpsa, no floor        Main/mod_tendency.F90:1027-1032
  start_advect     the cell's mass fluxes                      Main/mod_advection.F90:111-120
  hadvtr           both upstream_mode branches                 Main/mod_advection.F90:666-720
  vadv4d, ind = 2  threshold mintr * ps                        Main/mod_advection.F90:895-916, 958-961
  vadv4d, ind = 3  the PBL-top rule (ibltyp 2, iuwvadv 1)      Main/mod_advection.F90:917-957
  calc_coeff (NH)  tests/dyn_ref.py nh_xkc                     Main/mod_diffusion.F90:215-250
  nudge_chiten     ichebdy = 1, on atm2                        Main/chemlib/mod_che_bdyco.F90:898-982
  diffu_x4d        idiffu 1 and 2, on chib3d                   Main/mod_diffusion.F90:805-892
  chib3d           max(atm2 * rpsb, 0)                         Main/mod_slice.F90:196-200
  the sums         chiten + chidyn + chiphy                    Main/mod_tendency.F90:549-563
  the forecast     atmc = atm2 (+ dt * chiten on jci x ici)    Main/mod_tendency.F90:564-569
  the fix          0.1 * sum |atmc(j-1:j+1,i-1:i+1)| / 9       Main/mod_tendency.F90:571-582
  the filter       filter_raw_4d, gnu2, 0.53, low = 0          Main/mod_timefilter.F90:231-255
  bdyval           chem_bdyval_coupled                         Main/chemlib/mod_che_bdyco.F90:565-758

Arrays are (k, i, j) with the Fortran point (j, i, k) at [k - 1, i - 1, j - 1]; cross fields hold
i = 1..iy-1, j = 1..jx-1 (the last row and column are unused).
"""
import dataclasses

import numpy as np

from tests.dyn_ref import band_sides, nh_xkc  # noqa: F401  (nh_xkc: the tracer tests read it from here)

MINTR = 1.0e-30                 # Share/mod_constants.F90:63
RAW_BETA = 0.53                 # Main/mod_tendency.F90:585
Z4 = (1.0, -4.0, 12.0)          # z4_c1..3, Main/mod_diffusion.F90
O4 = (4.0 / 6.0, 1.0 / 6.0, -20.0 / 6.0)


def chib3d(atm2, psb):
    """mkslice's export (Main/mod_slice.F90:196-200); rpsb = 1 / psb (:163-165)."""
    with np.errstate(divide="ignore", invalid="ignore"):       # the unused last row and column hold zeros
        rpsb = 1.0 / psb
        return np.maximum(atm2 * rpsb[None], 0.0)


def relaxation_band(rc):
    """(side, ibnd) of the cross relaxation band ba_cr on (i, j) planes, from the one statement of
    setup_boundaries (tests/dyn_ref.py band_sides): side 0 none, 1 south, 2 north, 3 west, 4 east."""
    side = np.zeros((rc.iy, rc.jx), dtype=np.int8)
    ibnd = np.full((rc.iy, rc.jx), -1, dtype=np.int16)
    for (j, i), (sd, ib) in band_sides(rc, dot=False).items():
        side[i - 1, j - 1], ibnd[i - 1, j - 1] = sd, ib
    return side, ibnd


@dataclasses.dataclass
class StepInputs:
    """What the tracers read of the step: the pre-step state, and QDOT and the scaled XKC of the same
    tend (exact inputs: both come out of transcendental chains the tracers do not own)."""
    psa: np.ndarray
    psb: np.ndarray
    umc: np.ndarray          # atm1%u * msfd (decouple, Main/mod_tendency.F90:1016-1018)
    vmc: np.ndarray
    xmapf: np.ndarray        # 1 / (msfx * msfx * dx4) (Main/mod_advection.F90 init)
    qdot: np.ndarray
    xkc: np.ndarray
    dt: float
    xt_tend: float           # xbctime + dt of tend
    xt_bdyval: float         # xbctime + dt of the bdyval that follows
    integrating: bool = True
    kpbl: np.ndarray = None  # (iy, jx): itrvadv = 3 (ibltyp = 2 with iuwvadv = 1), else ind = 2

    @classmethod
    def from_state(cls, rc, st, qdot, xkc, dt, xt_tend, xt_bdyval, integrating=True, kpbl=None):
        dx4 = 4.0 * (rc.ds * 1000.0)
        msfx = st["MSFX"][0]
        with np.errstate(divide="ignore", invalid="ignore"):
            xmapf = 1.0 / (msfx * msfx * dx4)
        return cls(st["PSA"][0], st["PSB"][0], st["ATM1_U"] * st["MSFD"][0][None], st["ATM1_V"] * st["MSFD"][0][None],
                   xmapf, qdot, xkc, dt, xt_tend, xt_bdyval, integrating, kpbl)


@dataclasses.dataclass
class Result:
    atm1: np.ndarray
    atm2: np.ndarray
    forecast: np.ndarray     # atmc%chi before the fix
    nnegative: int
    ndependent: int          # negatives with a negative sweep predecessor


def vertical_constants(rc):
    sig = rc.sigma
    hs = (sig[1:] + sig[:-1]) * 0.5
    ds = sig[1:] - sig[:-1]
    kz = rc.kz
    twt1 = np.zeros(kz + 1)
    twt2 = np.zeros(kz + 1)
    for k in range(2, kz + 1):          # Main/mod_params.F90:2208-2215; index k = Fortran level
        twt1[k] = (sig[k - 1] - hs[k - 2]) / (hs[k - 1] - hs[k - 2])
        twt2[k] = 1.0 - twt1[k]
    return twt1, twt2, 1.0 / ds


def uw_interface_values(rc, f, kpb, twt1, twt2):
    """vadv4d ind = 3 before the svv factor (Main/mod_advection.F90:917-955): fg(k), k = 2..kz, the
    linear interpolation, replaced at kpb - 1 and kpb (kpb >= 4) by the PBL-top rule.  f: (kz, ni, nj)
    coupled atm1, kpb: (ni, nj) levels as doubles.  Returns (kz - 1, ni, nj), index 0 = interface 2."""
    kz = rc.kz
    sig = rc.sigma
    hs = (sig[1:] + sig[:-1]) * 0.5
    fg = np.stack([twt1[k] * f[k - 1] + twt2[k] * f[k - 2] for k in range(2, kz + 1)])
    kp = kpb.astype(np.int64)
    for i, j in zip(*np.nonzero(kp >= 4)):
        col = f[:, i, j]
        kb = int(kp[i, j])
        k = kb - 2                                          # Fortran levels; col[k - 1] is f(k)
        up, dn = col[k] - col[k - 1], col[k - 1] - col[k - 2]
        if up > 0.0 and dn > 0.0:
            slope = min(up / (hs[k] - hs[k - 1]), dn / (hs[k - 1] - hs[k - 2]))
        elif up < 0.0 and dn < 0.0:
            slope = max(up / (hs[k] - hs[k - 1]), dn / (hs[k - 1] - hs[k - 2]))
        else:
            slope = 0.0
        k = kb
        fg[k - 1 - 2, i, j] = col[k - 3] + slope * (sig[k - 2] - hs[k - 3])
        if abs(col[k - 3] + slope * (hs[k - 2] - hs[k - 3]) - col[k - 1]) > abs(col[k - 2] - col[k - 1]):
            fg[k - 2, i, j] = col[k - 1]
        else:
            fg[k - 2, i, j] = col[k - 3] + slope * (sig[k - 1] - hs[k - 3])
    return fg


def serial_fix(cq, rc, factor=0.1):
    """The reference's loop (Main/mod_tendency.F90:571-582): k, then i, then j ascending, each negative
    interior value replaced in place by factor * sum(|3 x 3|) / 9, the sum in the array section's
    element order (j fastest).  Vectorised over the planes' independent points: only a negative
    point with a negative sweep predecessor ((j-1,i), (j-1,i-1), (j,i-1), (j+1,i-1), all interior)
    reads a fixed value, so every other negative is computed from the original plane at once and the
    dependent ones are walked in order.  Returns (fixed, negatives, dependent negatives)."""
    iy, jx = rc.iy, rc.jx
    out = cq.copy()
    neg = np.zeros(cq.shape, dtype=bool)
    neg[:, 1:iy - 2, 1:jx - 2] = cq[:, 1:iy - 2, 1:jx - 2] < 0.0
    p = np.pad(neg, ((0, 0), (1, 1), (1, 1)))
    pred = p[:, 1:-1, :-2] | p[:, :-2, :-2] | p[:, :-2, 1:-1] | p[:, :-2, 2:]
    dep = neg & pred
    a = np.abs(cq)
    ap = np.pad(a, ((0, 0), (1, 1), (1, 1)))
    s = np.zeros(cq.shape)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            s = s + ap[:, 1 + di:1 + di + iy, 1 + dj:1 + dj + jx]
    ind = neg & ~dep
    out[ind] = (factor * s / 9.0)[ind]
    for k, i, j in zip(*np.nonzero(dep)):          # np.nonzero: k, then i, then j ascending
        t = 0.0
        for ii in (i - 1, i, i + 1):
            for jj in (j - 1, j, j + 1):
                # the sweep has passed the predecessors (their fixed values); the others are original
                done = ii < i or (ii == i and jj < j)
                t = t + abs(out[k, ii, jj] if done else cq[k, ii, jj])
        out[k, i, j] = factor * t / 9.0
    return out, int(neg.sum()), int(dep.sum())


def serial_fix_loops(cq, rc, factor=0.1):
    """The same as the plain triple loop of the text."""
    out = cq.copy()
    for k in range(cq.shape[0]):
        for i in range(1, rc.iy - 2):
            for j in range(1, rc.jx - 2):
                if out[k, i, j] < 0.0:
                    t = 0.0
                    for ii in (i - 1, i, i + 1):
                        for jj in (j - 1, j, j + 1):
                            t = t + abs(out[k, ii, jj])
                    out[k, i, j] = factor * t / 9.0
    return out


def tend_bdyval(rc, s, atm1, atm2, chiphy, chib0, chibt, cefc, cegc, bdyval=True):
    """One tend (and one bdyval) of one tracer.  cefc, cegc: (kz, nspgx), [k - 1, ib - 1]."""
    kz, iy, jx = rc.kz, rc.iy, rc.jx
    I, J = slice(1, iy - 2), slice(1, jx - 2)              # ici, jci

    def at(a, di=0, dj=0):
        """a(j + dj, i + di, :) on jci x ici."""
        return a[..., 1 + di:iy - 2 + di, 1 + dj:jx - 2 + dj]

    with np.errstate(divide="ignore", invalid="ignore"):
        rpsa = 1.0 / s.psa
        chi = atm1 * rpsa[None]                            # no floor
    chib = chib3d(atm2, s.psb)
    ps = at(s.psa)[None]
    # start_advect
    uavg1 = at(s.umc, 1, 0) + at(s.umc)
    uavg2 = at(s.umc, 1, 1) + at(s.umc, 0, 1)
    vavg1 = at(s.vmc, 0, 1) + at(s.vmc)
    vavg2 = at(s.vmc, 1, 1) + at(s.vmc, 1, 0)
    fc, fw, fe, fs, fn = at(chi), at(chi, 0, -1), at(chi, 0, 1), at(chi, -1, 0), at(chi, 1, 0)
    xm = at(s.xmapf)[None]
    if rc.upstream_mode:
        ul = rc.uoffc * 0.5 * rc.dt / (rc.ds * 1000.0)
        f1 = 0.5 * ul * (uavg2 + uavg1) / ps
        f2 = 0.5 * ul * (vavg2 + vavg1) / ps
        fx1 = (1.0 + f1) * fw + (1.0 - f1) * fc
        fx2 = (1.0 + f1) * fc + (1.0 - f1) * fe
        fy1 = (1.0 + f2) * fs + (1.0 - f2) * fc
        fy2 = (1.0 + f2) * fc + (1.0 - f2) * fn
    else:
        fx1, fx2, fy1, fy2 = fw + fc, fc + fe, fs + fc, fc + fn
    fg = -xm * (uavg2 * fx2 - uavg1 * fx1 + vavg2 * fy2 - vavg1 * fy1)
    ten = 0.0 + fg
    # vadv4d, ind = 2, on the coupled atm1
    twt1, twt2, xds = vertical_constants(rc)
    f = at(atm1)
    svv = at(s.qdot)
    thr = MINTR * ps[0]
    flux = np.zeros((kz + 2,) + f.shape[1:])               # fg(k), Fortran interface k = 2..kz
    if s.kpbl is not None:
        flux[2:kz + 1] = uw_interface_values(rc, f, at(s.kpbl), twt1, twt2) * svv[1:kz]
    for k in range(2, kz + 1):
        if s.kpbl is not None:
            break
        sv, fk, fkm = svv[k - 1], f[k - 1], f[k - 2]
        val = sv * (twt1[k] * fk + twt2[k] * fkm)
        flux[k] = np.where(sv > 0.0, np.where(fkm > thr, val, 0.0), np.where(fk > thr, val, 0.0))
    for k in range(1, kz + 1):                             # level k: + fg(k) xds(k), then - fg(k+1) xds(k)
        if k >= 2:
            ten[k - 1] = ten[k - 1] + flux[k] * xds[k - 1]
        if k + 1 <= kz:
            ten[k - 1] = ten[k - 1] - flux[k + 1] * xds[k - 1]
    # nudge_chiten (iboudy 1 or 5)
    if rc.iboudy in (1, 5):
        side, ibnd = relaxation_band(rc)
        sd, ib = at(side), at(ibnd)
        fls = chib0 + s.xt_tend * chibt - atm2
        for k in range(kz):
            for sides, order in (((1, 2), ((0, -1), (0, 1), (-1, 0), (1, 0))), ((3, 4), ((-1, 0), (1, 0), (0, -1), (0, 1)))):
                m = (sd == sides[0]) | (sd == sides[1])
                if not m.any():
                    continue
                xf, xg = cefc[k][np.maximum(ib, 1) - 1], cegc[k][np.maximum(ib, 1) - 1]
                f0 = at(fls[k])
                f1_, f2_, f3_, f4_ = (at(fls[k], di, dj) for di, dj in order)
                new = ten[k] + xf * f0 - xg * (f1_ + f2_ + f3_ + f4_ - 4.0 * f0)
                ten[k] = np.where(m, new, ten[k])
    # diffu_x4d on chib3d with the step's scaled xkc
    xk = at(s.xkc)
    c, w, e, so, n = at(chib), at(chib, 0, -1), at(chib, 0, 1), at(chib, -1, 0), at(chib, 1, 0)
    if rc.idiffu == 2:
        diag = at(chib, 1, 1) + at(chib, -1, -1) + at(chib, 1, -1) + at(chib, -1, 1)
        ten = ten + 1.0 * xk * (O4[0] * (e + w + n + so) + O4[1] * diag + O4[2] * c)
    else:
        ii, jj = np.meshgrid(np.arange(2, iy - 1), np.arange(2, jx - 1), indexing="ij")      # Fortran i, j of ici x jci
        inner = (ii >= 3) & (ii <= iy - 3) & (jj >= 3) & (jj <= jx - 3)                       # jcii x icii
        chp = np.pad(chib, ((0, 0), (2, 2), (2, 2)))

        def at2(di, dj):
            return chp[:, 3 + di:iy + di, 3 + dj:jx + dj]
        far = at2(0, 2) + at2(0, -2) + at2(2, 0) + at2(-2, 0)
        fourth = ten - 1.0 * xk * (Z4[0] * far + Z4[1] * (e + w + n + so) + Z4[2] * c)
        ten = np.where(inner[None], fourth, ten)
        for line in (jj == 2, jj == jx - 2, ii == 2, ii == iy - 2):                           # west, east, south, north
            second = ten + 1.0 * xk * (Z4[0] * (e + w + n + so) + Z4[1] * c)
            ten = np.where(line[None], second, ten)
    # the sums and the forecast
    ten = (0.0 + ten) + at(chiphy)
    cq = atm2.copy()
    cq[:, I, J] = at(atm2) + s.dt * ten
    fixed, nneg, ndep = serial_fix(cq, rc)
    # filter_raw_4d (gnu2, 0.53, low = 0) on jci x ici
    v = at(fixed)
    d = rc.gnu2 * (v + at(atm2) - 2.0 * at(atm1))
    n2 = at(atm1) + RAW_BETA * d
    n1 = v + (RAW_BETA - 1.0) * d
    a1, a2 = atm1.copy(), atm2.copy()
    a2[:, I, J] = np.where(n2 < 0.0, 0.0, n2)
    a1[:, I, J] = np.where(n1 < 0.0, 0.0, n1)
    if bdyval:
        chem_bdyval(rc, a1, a2, chib0, chibt, s.xt_bdyval, s.integrating)
    return Result(a1, a2, cq, nneg, ndep)


def chem_bdyval(rc, a1, a2, chib0, chibt, xt, integrating=True):
    """chem_bdyval_coupled, ichebdy = 1, in place: chib = chia on the lines (west / east over ice,
    south / north over jci), then chia = chib0 + xt * chibt (west / east over ici, south / north
    over jce)."""
    iy, jx = rc.iy, rc.jx
    jce1, jce2, ice1, ice2 = 0, jx - 2, 0, iy - 2          # python indices of the cross lines
    ICE, JCI = slice(0, iy - 1), slice(1, jx - 2)
    ICI, JCE = slice(1, iy - 2), slice(0, jx - 1)
    if integrating:
        a2[:, ICE, jce1] = a1[:, ICE, jce1]
        a2[:, ICE, jce2] = a1[:, ICE, jce2]
        a2[:, ice1, JCI] = a1[:, ice1, JCI]
        a2[:, ice2, JCI] = a1[:, ice2, JCI]
    b = chib0 + xt * chibt
    a1[:, ICI, jce1] = b[:, ICI, jce1]
    a1[:, ICI, jce2] = b[:, ICI, jce2]
    a1[:, ice1, JCE] = b[:, ice1, JCE]
    a1[:, ice2, JCE] = b[:, ice2, JCE]
