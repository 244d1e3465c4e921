"""The chain of tests/tracer_ref.py's tend_bdyval restated with the snapshots of the reference's tracer
budget (ichdiag > 0): tend copies the running chidyn into chiten0 before a stage and books the stage's
term through ten2diag / extracttenchi, store = store + (chidyn - chiten0) * alarm_out_atm%rw on
jci x ici (Main/mod_tendency.F90:1403-1412, 1503-1511, 1540-1542, 2177-2207):

  ADVH  after hadv, no chiten0: chidyn * rw (the running sum is 0 + hadv)
  ADVV  after vadv, against the value after hadv
  BDY   after nudge_chi, on every iboudy: + 0.0 where iboudy is not 1 / 5 or the tables are zero
  DIFH  after diffu_x

Each is the rounded difference of two running sums times rw.  The helpers and constants are
tracer_ref's; tests/test_tracer_diag_cpu.py holds the final state equal to tracer_ref.tend_bdyval's bit
for bit, so the two statements cannot drift.  Test infrastructure of tests/test_tracer_diag_gpu.py.
"""
import numpy as np

from tests.tracer_ref import (MINTR, O4, RAW_BETA, Z4, Result, StepInputs, chem_bdyval, chib3d, relaxation_band,
                              serial_fix, uw_interface_values, vertical_constants)

TERMS = ("ADVH", "ADVV", "BDY", "DIFH")
__all__ = ["TERMS", "StepInputs", "tend_bdyval"]


def tend_bdyval(rc, s, atm1, atm2, chiphy, chib0, chibt, cefc, cegc, rw, bdyval=True):
    """One tend (and one bdyval) of one tracer with the four stage terms of the budget: (terms,
    Result).  terms: {name: (kz, iy, jx)}, what one tend adds to a zero accumulator, zero outside
    jci x ici.  cefc, cegc: (kz, nspgx), [k - 1, ib - 1]; rw: alarm_out_atm%rw."""
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
    terms = {}

    def book(name, x):
        """store = store + x * rw on jci x ici (extracttenchi), store zero before."""
        full = np.zeros((kz, iy, jx))
        full[:, I, J] = 0.0 + x * rw
        terms[name] = full
    book("ADVH", ten)                                      # ten2diag(aten%chi, cadvhdiag, pc_dynamic): no ten0
    ten0 = ten.copy()
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
    book("ADVV", ten - ten0)
    ten0 = ten.copy()
    # nudge_chiten (iboudy 1 or 5); cbdydiag is booked on every iboudy (Main/mod_tendency.F90:1503-1511)
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
    book("BDY", ten - ten0)
    ten0 = ten.copy()
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
    book("DIFH", ten - ten0)
    terms["CHIDYN"] = np.zeros((kz, iy, jx))                # the dynamic total the four terms close on
    terms["CHIDYN"][:, I, J] = ten
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
    return terms, Result(a1, a2, cq, nneg, ndep)
