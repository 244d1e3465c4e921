"""A NumPy statement of one step of the UW-PBL turbulent kinetic energy in the hydrostatic core
(ibltyp = 2) on a limited-area domain: the tend rows and bdyval's TKE lines.  Written from the
Fortran text; nothing here reads the oracle or the engine.  A sibling of tests/dyn_ref.py, which
supplies compute_omega's qdot, the diffusion coefficients and the diffusion forms.  Test
infrastructure: tests/test_tke_rows_cpu.py compares the oracle with it, tests/test_tke_rows_gpu.py the
engine.

Every expression keeps the operation order of the text (left to right, the parentheses of the
source), in float64.  The chain holds no transcendental function (calc_coeff's sqrt is correctly
rounded), so it is comparable bit for bit.

  start_advect      uavg1/2, vavg1/2 from atmx%umc / vmc          Main/mod_advection.F90:111-120
  init_advection    dds, ul                                      Main/mod_advection.F90:100-106
  hadv3d ind = 1    winds interpolated to full levels with twt;  Main/mod_advection.F90:427-451 (centred),
                    f1 / f2 from the level-k winds                 481-507 (upstream_mode)
  tkeps             atm1%tke * psa                               Main/mod_tendency.F90:1414-1425
  vadv3d nk = kzp1  ind = 0: qq, fx, the two adds per level      Main/mod_advection.F90:755-765
  diffu_x3df        atm2%tke with fac = nuk on xkcf, idiffu 1, 2  Main/mod_diffusion.F90:523-601, 232-245;
                    and 3 (xkc read on kz + 1 levels)              602-651; called Main/mod_tendency.F90:1545-1548
  the sum, forecast tketen + tkedyn*rpsa + tkephy, max(tkemin,.) Main/mod_tendency.F90:515-542
  filter_ra_3d      timefilter_apply(atm1, atm2, atmc, gnu2)     Main/mod_tendency.F90:543; Main/mod_timefilter.F90:92-110
  bdyuv             the wind slices of the inflow / outflow test  Main/mod_bdycod.F90:896-1061
  bdyval            atm2 = atm1 on the lines; tkemin on level 1;  Main/mod_bdycod.F90:1166-1172, 1212-1218,
                    inflow tkemin / outflow interior neighbour     1258-1264, 1301-1307, 2433-2514

Arrays are (k, i, j) with the Fortran point (j, i, k) at [k - 1, i - 1, j - 1], kz + 1 levels; cross
fields hold i = 1..iy-1, j = 1..jx-1.
"""
import numpy as np

from tests import dyn_ref as dr

TKE_INPUTS = ("ATM1_TKE", "ATM2_TKE", "TKEPHY")


def sigma_weights(rc):
    """(twt1, twt2) indexed by the 1-based k = 2..kz (Main/mod_params.F90, as tests/dyn_ref.py), dds
    indexed by the 1-based k = 1..kz+1 with dds(1) = dds(kzp1) = 0 (Main/mod_advection.F90:100-105)."""
    kz = rc.kz
    sig = rc.sigma
    hsig = (sig[1:] + sig[:-1]) * 0.5
    dsig = sig[1:] - sig[:-1]
    twt1, twt2 = np.zeros(kz + 1), np.zeros(kz + 1)
    for k in range(2, kz + 1):
        twt1[k] = (sig[k - 1] - hsig[k - 2]) / (hsig[k - 1] - hsig[k - 2])
        twt2[k] = 1.0 - twt1[k]
    dds = np.zeros(kz + 2)
    for k in range(2, kz + 1):
        dds[k] = 1.0 / (dsig[k - 1] + dsig[k - 2])
    return twt1, twt2, dds


def interior(rc):
    """[i, j] of jci x ici."""
    return dr.domain_mask(rc)


def tke_tend(rc, g, tke1, tke2, tkephy, dt, tiles=None):
    """The TKE rows of one hydrostatic tend.  g: dyn_ref.HYDRO_INPUTS after bdyval; tke1, tke2: atm1 /
    atm2 tke (decoupled); tkephy: the UW scheme's tendency; dt: the step's dt (rcmdyn get_time).
    Returns atm1 / atm2 tke after the time filter (`a1`, `a2`) and the stages: `had` (tkedyn after
    hadv3d), `adv` (after vadv3d), `dif` (the diffusion increments), `dyn` (tkedyn), `ten` (tketen), `raw`
    (atm2 + dt tketen), `fc` (atmc), `qdot`.  tiles: the decomposition, for idiffu = 3 alone."""
    kz, iy, jx = rc.kz, rc.iy, rc.jx
    dx = rc.ds * 1000.0
    ul = rc.uoffc * 0.5 * rc.dt / dx
    twt1, twt2, dds = sigma_weights(rc)
    pa, msfx, msfd = g["PSA"][0], g["MSFX"][0], g["MSFD"][0]
    rpsa = np.divide(1.0, pa, out=np.zeros_like(pa), where=pa > 0)
    sh = dr.sh
    m = interior(rc)
    old_err = np.seterr(divide="ignore", invalid="ignore")      # frame edges: masked off below
    _, _, qdot = dr.compute_omega(rc, g)
    umc, vmc = g["ATM1_U"] * msfd, g["ATM1_V"] * msfd
    uavg1 = sh(umc, 0, 1) + umc                                  # ua(j,i+1,k) + ua(j,i,k)
    uavg2 = sh(umc, 1, 1) + sh(umc, 1, 0)                        # ua(j+1,i+1,k) + ua(j+1,i,k)
    vavg1 = sh(vmc, 1, 0) + vmc                                  # va(j+1,i,k) + va(j,i,k)
    vavg2 = sh(vmc, 1, 1) + sh(vmc, 0, 1)                        # va(j+1,i+1,k) + va(j,i+1,k)
    xmapf = 1.0 / (msfx * msfx * (4.0 * dx))

    # ---- hadv3d(tkedyn, atm1%tke, 1): levels k = 2..kz; the interpolated winds carry the flux, the
    # upstream weights f1 / f2 are formed from the level-k winds (:497-498)
    dyn = np.zeros((kz + 1, iy, jx))
    f = tke1
    for k in range(2, kz + 1):
        c = f[k - 1]
        w, e_, s_, n = sh(c, -1, 0), sh(c, 1, 0), sh(c, 0, -1), sh(c, 0, 1)
        uaz1 = twt1[k] * uavg1[k - 1] + twt2[k] * uavg1[k - 2]
        uaz2 = twt1[k] * uavg2[k - 1] + twt2[k] * uavg2[k - 2]
        vaz1 = twt1[k] * vavg1[k - 1] + twt2[k] * vavg1[k - 2]
        vaz2 = twt1[k] * vavg2[k - 1] + twt2[k] * vavg2[k - 2]
        if rc.upstream_mode:
            f1 = 0.5 * ul * (uavg2[k - 1] + uavg1[k - 1]) / pa
            f2 = 0.5 * ul * (vavg2[k - 1] + vavg1[k - 1]) / pa
            fx1 = (1.0 + f1) * w + (1.0 - f1) * c
            fx2 = (1.0 + f1) * c + (1.0 - f1) * e_
            fy1 = (1.0 + f2) * s_ + (1.0 - f2) * c
            fy2 = (1.0 + f2) * c + (1.0 - f2) * n
        else:
            fx1, fx2, fy1, fy2 = w + c, c + e_, s_ + c, c + n
        dyn[k - 1] = dyn[k - 1] - xmapf * (uaz2 * fx2 - uaz1 * fx1 + vaz2 * fy2 - vaz1 * fy1)
    dyn = np.where(m[None], dyn, 0.0)
    had = dyn.copy()

    # ---- tkeps and vadv3d(tkedyn, tkeps, kzp1, 0): k = 1..kz in turn, so level k takes
    # + fx(k-1) dds(k) first and - fx(k) dds(k) second
    tkeps = tke1 * pa[None]
    for k in range(1, kz + 1):
        qq = 0.5 * (qdot[k - 1] + qdot[k])
        fx = qq * (tkeps[k - 1] + tkeps[k])
        dyn[k] = dyn[k] + fx * dds[k + 1]
        dyn[k - 1] = dyn[k - 1] - fx * dds[k]
    dyn = np.where(m[None], dyn, 0.0)
    adv = dyn.copy()

    # ---- diffu_x3df(tkedyn, atm2%tke, nuk): xkcf(1) = xkc(1), xkcf(k+1) = xkc(k), scaled like xkc
    # (:232-245).  At idiffu = 3 the text reads xkc(j,i,k) up to k = kzp1, one level past xkc's kz; the
    # coefficient is diff_6th_coef * p*b on every level (what xkcf holds), which is what is taken here.
    co = dr.hydro_coeff(rc, g)
    xkcf = np.concatenate([co["xkc"][:1], co["xkc"]], axis=0)
    if rc.idiffu == 3:
        dif = dr.diffu6(rc, tke2, tke2 / msfd[None], xkcf, dr.tile_columns(rc, False, tiles), dot=False, fac=rc.nuk)
    else:
        dif = dr._diffu(rc, tke2, xkcf, dot=False, fac=rc.nuk)
    dyn = dr.apply(dyn, dif)
    np.seterr(**old_err)

    # ---- tketen (zero at the start of tend) + tkedyn * rpsa + tkephy; the forecast with its floor
    ten = np.where(m[None], np.zeros_like(dyn) + dyn * rpsa[None] + tkephy, 0.0)
    raw = tke2 + dt * ten
    fc = np.maximum(rc.tkemin, raw)
    # ---- filter_ra_3d on jci x ici, every level
    d = rc.gnu2 * (fc + tke2 - 2.0 * tke1)
    a2 = np.where(m[None], tke1 + d, tke2)
    a1 = np.where(m[None], fc, tke1)
    return dict(a1=a1, a2=a2, had=had, adv=adv, dif=dif, dyn=dyn, ten=ten, raw=raw, fc=fc, qdot=qdot, xkcf=xkcf)


def bdyuv_slices(rc, u1, v1, b, xt):
    """bdyuv on one limited-area tile, iboudy /= 0: the u slices west / east and the v slices south /
    north, exterior (the boundary value b0 + xt bt on jde1 / jde2 / ide1 / ide2) and interior (atm1 on
    jdi1 / jdi2 / idi1 / idi2), (kz, iy + 2) or (kz, jx + 2) indexed by the 1-based i or j, zero where
    never written, with the corner fills of the interior slices (:1030-1061)."""
    kz, iy, jx = rc.kz, rc.iy, rc.jx
    ub = b["XUB_B0"] + xt * b["XUB_BT"]
    vb = b["XVB_B0"] + xt * b["XVB_BT"]
    ri = np.arange(2, iy)                                        # idi1..idi2
    rj = np.arange(2, jx)                                        # jdi1..jdi2
    re = np.arange(1, jx + 1)                                    # jde1..jde2
    sl = {n: np.zeros((kz, iy + 2)) for n in ("wue", "wui", "eue", "eui")}
    sl.update({n: np.zeros((kz, jx + 2)) for n in ("sve", "svi", "nve", "nvi", "sue", "nue")})
    sl["wui"][:, ri], sl["eui"][:, ri] = u1[:, ri - 1, 1], u1[:, ri - 1, jx - 2]
    sl["wue"][:, ri], sl["eue"][:, ri] = ub[:, ri - 1, 0], ub[:, ri - 1, jx - 1]
    sl["svi"][:, rj], sl["nvi"][:, rj] = v1[:, 1, rj - 1], v1[:, iy - 2, rj - 1]
    sl["sve"][:, re], sl["nve"][:, re] = vb[:, 0, re - 1], vb[:, iy - 1, re - 1]
    sl["sue"][:, re], sl["nue"][:, re] = ub[:, 0, re - 1], ub[:, iy - 1, re - 1]
    we = {"wve": vb[:, :, 0], "eve": vb[:, :, jx - 1]}           # wve / eve at idi1 and idi2
    sl["wui"][:, iy], sl["wui"][:, 1] = sl["nue"][:, 2], sl["sue"][:, 2]
    sl["eui"][:, iy], sl["eui"][:, 1] = sl["nue"][:, jx - 1], sl["sue"][:, jx - 1]
    sl["nvi"][:, 1], sl["svi"][:, 1] = we["wve"][:, iy - 2], we["wve"][:, 1]
    sl["nvi"][:, jx], sl["svi"][:, jx] = we["eve"][:, iy - 2], we["eve"][:, 1]
    return sl


def tke_bdyval(rc, a1, a2, u1, v1, b, xt):
    """bdyval's TKE lines past the start (rcmtimer%integrating, bdyflow).  a1, a2: atm1 / atm2 tke
    after tend; u1, v1: atm1 u, v after tend, of which only the lines jdi1, jdi2, idi1, idi2 are read (the
    interior slices of the inflow / outflow test); b: the boundary fields XUB / XVB _B0 / _BT; xt =
    xbctime + dt at the call.  Returns (atm1, atm2, inflow) with inflow {side: bool (kz - 1, n)} the
    choice at the levels k + 1 = 3..kz+1 of each line.

    In the text's order: atm2 = atm1 on the four lines (west / east over ici1..ici2, south / north over
    jce1..jce2), from atm1 before it takes its new boundary values; then, west, east, south, north:
    level 1 of both time levels is tkemin along the whole line; for k = 2..kz the level k + 1 of atm1 is
    tkemin where the eight-wind sum of levels k and k - 1 blows in and the first interior point's
    value (read when its turn comes) where it does not.  Level 2 of the lines is never written.  West
    and east run over ice1..ice2 (the corners theirs), south and north over jci1..jci2."""
    kz, iy, jx = rc.kz, rc.iy, rc.jx
    a1, a2 = a1.copy(), a2.copy()
    ci = np.arange(2, iy - 1)                                    # ici1..ici2
    a2[:, ci - 1, 0] = a1[:, ci - 1, 0]
    a2[:, ci - 1, jx - 2] = a1[:, ci - 1, jx - 2]
    a2[:, 0, :jx - 1] = a1[:, 0, :jx - 1]
    a2[:, iy - 2, :jx - 1] = a1[:, iy - 2, :jx - 1]
    sl = bdyuv_slices(rc, u1, v1, b, xt)
    tkemin = rc.tkemin
    inflow = {}
    ie = np.arange(1, iy)                                        # ice1..ice2
    jc = np.arange(2, jx - 1)                                    # jci1..jci2
    for side, ext, itr, col, cin, sign in (("west", "wue", "wui", 0, 1, 1.0), ("east", "eue", "eui", jx - 2, jx - 3, -1.0)):
        a1[0, :iy - 1, col] = tkemin
        a2[0, :iy - 1, col] = tkemin
        flow = np.zeros((kz - 1, ie.size), dtype=bool)
        for k in range(2, kz + 1):
            e, n = sl[ext], sl[itr]
            windavg = (e[k - 1, ie] + e[k - 1, ie + 1] + n[k - 1, ie] + n[k - 1, ie + 1] +
                       e[k - 2, ie] + e[k - 2, ie + 1] + n[k - 2, ie] + n[k - 2, ie + 1])
            flow[k - 2] = sign * windavg > 0.0
            a1[k, ie - 1, col] = np.where(flow[k - 2], tkemin, a1[k, ie - 1, cin])
        inflow[side] = flow
    for side, ext, itr, row, rin, sign in (("south", "sve", "svi", 0, 1, 1.0),
                                           ("north", "nve", "nvi", iy - 2, iy - 3, -1.0)):
        a1[0, row, :jx - 1] = tkemin
        a2[0, row, :jx - 1] = tkemin
        flow = np.zeros((kz - 1, jc.size), dtype=bool)
        for k in range(2, kz + 1):
            e, n = sl[ext], sl[itr]
            windavg = (e[k - 1, jc] + e[k - 1, jc + 1] + n[k - 1, jc] + n[k - 1, jc + 1] +
                       e[k - 2, jc] + e[k - 2, jc + 1] + n[k - 2, jc] + n[k - 2, jc + 1])
            flow[k - 2] = sign * windavg > 0.0
            a1[k, row, jc - 1] = np.where(flow[k - 2], tkemin, a1[k, rin, jc - 1])
        inflow[side] = flow
    return a1, a2, inflow
