"""A NumPy statement of one step of the UW-PBL turbulent kinetic energy (ibltyp = 2) in either core,
on a limited area, a band (i_band = 1) or the cloud-resolving grid (i_crm = 1): the tend rows and
bdyval's TKE lines.  Written from the Fortran text; nothing here reads the oracle or the engine.  A
sibling of tests/dyn_ref.py, which supplies the grid (geom), compute_omega's qdot of either core
(compute_omega, nh_qdot), the diffusion coefficients (hydro_coeff, nh_coeff) and the diffusion forms.
The TKE rows themselves are the same text in both cores; the cores differ in qdot and in calc_coeff.
A periodic direction has no boundary line: bdyval acts on the south and north lines of a band, over
every j, and on nothing under CRM.  Test infrastructure: tests/test_tke_rows_cpu.py and
tests/test_periodic_rows_cpu.py compare the oracle with it, tests/test_tke_rows_gpu.py and
tests/test_periodic_rows_gpu.py the engine.

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
  compute_omega     qdot of either core (dyn_ref.compute_omega,   Main/mod_tendency.F90:1118-1178
                    dyn_ref.nh_qdot)
  calc_coeff        xkc of either core (dyn_ref.hydro_coeff,      Main/mod_diffusion.F90:193-249
                    dyn_ref.nh_coeff)
  bdyuv             the wind slices of the inflow / outflow test  Main/mod_bdycod.F90:896-1061
  bdyval            atm2 = atm1 on the lines; tkemin on level 1;  Main/mod_bdycod.F90:1166-1172, 1212-1218,
                    inflow tkemin / outflow interior neighbour     1258-1264, 1301-1307, 2433-2514

Arrays are (k, i, j) with the Fortran point (j, i, k) at [k - 1, i - 1, j - 1], kz + 1 levels; cross
fields hold i = 1..iy-1, j = 1..jx-1, and every point of a periodic direction.
"""
import numpy as np

from tests import dyn_ref as dr

TKE_INPUTS = ("ATM1_TKE", "ATM2_TKE", "TKEPHY")
BDY_WINDS = ("XUB_B0", "XUB_BT", "XVB_B0", "XVB_BT")
NH_INPUTS = tuple(dict.fromkeys(dr.NH_QDOT_INPUTS + ("ATM2_U", "ATM2_V", "ATM2_W", "PSB", "MSFX", "HT") + BDY_WINDS))


def input_names(rc):
    """The fields tke_tend and tke_bdyval read, by core."""
    return (dr.HYDRO_INPUTS if rc.idynamic == 1 else NH_INPUTS) + TKE_INPUTS


def sigma_weights(rc):
    """(twt1, twt2) indexed by the 1-based k = 2..kz (Main/mod_params.F90, as tests/dyn_ref.py), dds
    indexed by the 1-based k = 1..kz+1 with dds(1) = dds(kzp1) = 0 (Main/mod_advection.F90:100-105)."""
    kz = rc.kz
    sig = rc.sigma
    dsig = sig[1:] - sig[:-1]
    twt1, twt2 = dr.twt(rc)
    dds = np.zeros(kz + 2)
    for k in range(2, kz + 1):
        dds[k] = 1.0 / (dsig[k - 1] + dsig[k - 2])
    return twt1, twt2, dds


def interior(rc):
    """[i, j] of jci x ici."""
    return dr.domain_mask(rc)


def tke_tend(rc, g, tke1, tke2, tkephy, dt, tiles=None, hydro_qdot=False, swap_twt=False):
    """The TKE rows of one tend of either core.  g: input_names(rc) after bdyval; tke1, tke2: atm1 /
    atm2 tke (decoupled); tkephy: the UW scheme's tendency; dt: the step's dt (rcmdyn get_time).
    qdot is compute_omega's of the core (rc.idynamic) and the coefficient calc_coeff's.  The last two
    arguments are mutants for the tests' non-vacuity asserts: hydro_qdot takes the hydrostatic qdot in
    the non-hydrostatic core; swap_twt exchanges nh_qdot's weights (dyn_ref.zero_pad_for_the_wrap is a
    third, of every neighbour read).
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
    if rc.idynamic == 1 or hydro_qdot:
        _, _, qdot = dr.compute_omega(rc, g)
    else:
        qdot = dr.nh_qdot(rc, g, swap_twt=swap_twt)
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
    co = dr.hydro_coeff(rc, g) if rc.idynamic == 1 else dr.nh_coeff(rc, g)
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
    """bdyuv on the whole grid as one tile, iboudy /= 0: the u slices west / east and the v slices
    south / north, exterior (the boundary value b0 + xt bt on jde1 / jde2 / ide1 / ide2) and interior
    (atm1 on jdi1 / jdi2 / idi1 / idi2), (kz, iy + 2) or (kz, jx + 2) indexed by the 1-based i or j, zero
    where never written.  Each only on a side that exists (`if ( ma%has_bdyleft )` .., :909-1025).  The
    corner fills of the interior slices (:1030-1061) stand under has_bdytopleft .. alone, which need
    two sides: a band has none, and its south / north interior slices are whole already, since
    jdi1..jdi2 is every j; the j + 1 past jx that bdyval reads is the slice at j = 1
    (exchange_bdy_lr, :1063-1076)."""
    kz, iy, jx = rc.kz, rc.iy, rc.jx
    G = dr.geom(rc)
    if not (G.left or G.right or G.bottom or G.top):
        return {}
    ub = b["XUB_B0"] + xt * b["XUB_BT"]
    vb = b["XVB_B0"] + xt * b["XVB_BT"]
    ri = np.arange(G.idi1, G.idi2 + 1)
    rj = np.arange(G.jdi1, G.jdi2 + 1)
    re = np.arange(G.jde1, G.jde2 + 1)
    sl = {n: np.zeros((kz, iy + 2)) for n in ("wue", "wui", "eue", "eui")}
    sl.update({n: np.zeros((kz, jx + 2)) for n in ("sve", "svi", "nve", "nvi", "sue", "nue")})
    if G.left:
        sl["wui"][:, ri], sl["wue"][:, ri] = u1[:, ri - 1, G.jdi1 - 1], ub[:, ri - 1, G.jde1 - 1]
    if G.right:
        sl["eui"][:, ri], sl["eue"][:, ri] = u1[:, ri - 1, G.jdi2 - 1], ub[:, ri - 1, G.jde2 - 1]
    if G.bottom:
        sl["svi"][:, rj] = v1[:, G.idi1 - 1, rj - 1]
        sl["sve"][:, re], sl["sue"][:, re] = vb[:, G.ide1 - 1, re - 1], ub[:, G.ide1 - 1, re - 1]
    if G.top:
        sl["nvi"][:, rj] = v1[:, G.idi2 - 1, rj - 1]
        sl["nve"][:, re], sl["nue"][:, re] = vb[:, G.ide2 - 1, re - 1], ub[:, G.ide2 - 1, re - 1]
    we = {"wve": vb[:, :, 0], "eve": vb[:, :, jx - 1]}           # wve / eve at idi1 and idi2
    if G.top and G.left:
        sl["wui"][:, iy], sl["nvi"][:, 1] = sl["nue"][:, 2], we["wve"][:, iy - 2]
    if G.bottom and G.left:
        sl["wui"][:, 1], sl["svi"][:, 1] = sl["sue"][:, 2], we["wve"][:, 1]
    if G.top and G.right:
        sl["eui"][:, iy], sl["nvi"][:, jx] = sl["nue"][:, jx - 1], we["eve"][:, iy - 2]
    if G.bottom and G.right:
        sl["eui"][:, 1], sl["svi"][:, jx] = sl["sue"][:, jx - 1], we["eve"][:, 1]
    if G.perj:
        for n in ("sve", "svi", "nve", "nvi", "sue", "nue"):
            sl[n][:, jx + 1], sl[n][:, 0] = sl[n][:, 1], sl[n][:, jx]
    return sl


def tke_bdyval(rc, a1, a2, u1, v1, b, xt):
    """bdyval's TKE lines past the start (rcmtimer%integrating, bdyflow).  a1, a2: atm1 / atm2 tke
    after tend; u1, v1: atm1 u, v after tend, of which only the lines jdi1, jdi2, idi1, idi2 are read (the
    interior slices of the inflow / outflow test); b: the boundary fields XUB / XVB _B0 / _BT; xt =
    xbctime + dt at the call.  Returns (atm1, atm2, inflow) with inflow {side: bool (kz - 1, n)} the
    choice at the levels k + 1 = 3..kz+1 of each line that exists.

    In the text's order: atm2 = atm1 on the lines (west / east over ici1..ici2, south / north over
    jce1..jce2), from atm1 before it takes its new boundary values; then, west, east, south, north:
    level 1 of both time levels is tkemin along the whole line; for k = 2..kz the level k + 1 of atm1 is
    tkemin where the eight-wind sum of levels k and k - 1 blows in and the first interior point's
    value (read when its turn comes) where it does not.  Level 2 of the lines is never written.  West
    and east run over ice1..ice2 (the corners theirs), south and north over jci1..jci2.  Every block
    stands under its side's has_bdy flag: a band has the south and north lines alone, over every j
    (jce = jci = 1..jx), and the CRM grid has none, so that bdyval changes no TKE value there."""
    kz = rc.kz
    G = dr.geom(rc)
    a1, a2 = a1.copy(), a2.copy()
    ci = np.arange(G.ici1, G.ici2 + 1)
    je = slice(G.jce1 - 1, G.jce2)
    if G.left:
        a2[:, ci - 1, G.jce1 - 1] = a1[:, ci - 1, G.jce1 - 1]
    if G.right:
        a2[:, ci - 1, G.jce2 - 1] = a1[:, ci - 1, G.jce2 - 1]
    if G.bottom:
        a2[:, G.ice1 - 1, je] = a1[:, G.ice1 - 1, je]
    if G.top:
        a2[:, G.ice2 - 1, je] = a1[:, G.ice2 - 1, je]
    sl = bdyuv_slices(rc, u1, v1, b, xt)
    tkemin = rc.tkemin
    inflow = {}
    ie = np.arange(G.ice1, G.ice2 + 1)
    jc = np.arange(G.jci1, G.jci2 + 1)
    for has, side, ext, itr, col, cin, sign in ((G.left, "west", "wue", "wui", G.jce1 - 1, G.jci1 - 1, 1.0),
                                                (G.right, "east", "eue", "eui", G.jce2 - 1, G.jci2 - 1, -1.0)):
        if not has:
            continue
        a1[0, ie - 1, col] = tkemin
        a2[0, ie - 1, col] = tkemin
        flow = np.zeros((kz - 1, ie.size), dtype=bool)
        for k in range(2, kz + 1):
            e, n = sl[ext], sl[itr]
            windavg = (e[k - 1, ie] + e[k - 1, ie + 1] + n[k - 1, ie] + n[k - 1, ie + 1] +
                       e[k - 2, ie] + e[k - 2, ie + 1] + n[k - 2, ie] + n[k - 2, ie + 1])
            flow[k - 2] = sign * windavg > 0.0
            a1[k, ie - 1, col] = np.where(flow[k - 2], tkemin, a1[k, ie - 1, cin])
        inflow[side] = flow
    for has, side, ext, itr, row, rin, sign in ((G.bottom, "south", "sve", "svi", G.ice1 - 1, G.ici1 - 1, 1.0),
                                                (G.top, "north", "nve", "nvi", G.ice2 - 1, G.ici2 - 1, -1.0)):
        if not has:
            continue
        a1[0, row, je] = tkemin
        a2[0, row, je] = tkemin
        flow = np.zeros((kz - 1, jc.size), dtype=bool)
        for k in range(2, kz + 1):
            e, n = sl[ext], sl[itr]
            windavg = (e[k - 1, jc] + e[k - 1, jc + 1] + n[k - 1, jc] + n[k - 1, jc + 1] +
                       e[k - 2, jc] + e[k - 2, jc + 1] + n[k - 2, jc] + n[k - 2, jc + 1])
            flow[k - 2] = sign * windavg > 0.0
            a1[k, row, jc - 1] = np.where(flow[k - 2], tkemin, a1[k, rin, jc - 1])
        inflow[side] = flow
    return a1, a2, inflow
