"""A NumPy statement of the reference's horizontal diffusion and lateral-boundary relaxation, and of
the hydrostatic tendencies they are added to, on the whole grid as one tile, from the state after the
initial bdyval.  The grid is the text's: a limited area, a band (i_band = 1, periodic in j), or the
cloud-resolving grid (i_crm = 1 over a band, periodic in j and i); `geom` gives the sides that exist and
the loop ranges, and every mask and range below comes from it.  Written from the Fortran text; nothing here reads the
oracle or the engine.  Test infrastructure: tests/test_dyn_rows_cpu.py compares the oracle with it,
tests/test_dyn_rows_gpu.py the engine.

Every expression keeps the operation order of the text (left to right, the parentheses of the
source), in float64.  calc_coeff, diffu_d, diffu_x, the nudge and sponge routines and the surface
pressure tendency hold no transcendental function but the exp of the iboudy = 5 coefficient table
(math.exp, the C library's), so they are comparable bit for bit; the advection, adiabatic and
pressure-gradient terms hold libm pow / log and are compared at rtol 1e-10.

  the grid          has_bdy*, jde .. jcii, ide .. icii           Main/mod_atm_interface.F90:231-286;
                                                                Main/mpplib/mod_mppparam.F90:1104-1132, 1338-1360
  setup_boundaries  ba_cr / ba_dt, ibnd and the side           Main/mod_atm_interface.F90:383-542
  setup_bdycon      fnudge, gnudge, fcx.., wgtx.., hefc..      Main/mod_bdycod.F90:203-273
  psc2psd           psdotb, the edge and corner rules          Main/mpplib/mod_mppparam.F90:13811-13862
  mkslice           ubd3d, tb3d, qxb3d (floors minqq and 0)    Main/mod_slice.F90:169-195
  initialize_diff.  xkhz, xkhmax, dydc, hgfact                 Main/mod_diffusion.F90:100-140
  calc_coeff        xkc (both cores), xkd, the scaling         Main/mod_diffusion.F90:193-249
  diffu_d           idiffu 1 (interior, ring, corners) and 2   Main/mod_diffusion.F90:281-411
  diffu_x3d / 4d3d  the same on cross points                   Main/mod_diffusion.F90:673-735, 822-892
  calc_coeff        idiffu 3: diff_6th_coef * p* (xkc, xkcf, xkd) Main/mod_diffusion.F90:154, 174-183
  diffu_d / x3d /   idiffu 3: one column per tile, clamped       Main/mod_diffusion.F90:412-516, 602-651,
  x4d3d / x3df      neighbours, four limited fluxes, one add       736-785, 893-942
  pressure_grad.    ipgf 0 and 1 (ttld, the reference            Main/mod_tendency.F90:1886-2119;
                    temperature off rtbar, phi(kz))                Share/mod_constants.F90:359-362
  nudge3d / 4d3d    t, qv (nfac / rfac)                        Main/mod_bdycod.F90:4218-4406, 3206-3392
  nudgeuv           u, v on ba_dt                              Main/mod_bdycod.F90:3581-3823
  nudge2d           p* with the level-kz coefficient           Main/mod_bdycod.F90:4597-4766
  sponge3d/4d/uv/2d wgt * ften + (1 - wgt) * bt                Main/mod_bdycod.F90:2591-3122
  compute_omega     cr, pten, qdot, omega                      Main/mod_tendency.F90:1118-1215
  compute_omega     the idynamic = 2 qdot (nh_qdot)            Main/mod_tendency.F90:1158-1178
  new_pressure      the p* boundary term                       Main/mod_tendency.F90:1428-1438
  the call order    advection, curvature, adiabatic, boundary, diffusion, the sums, the
                    pressure-gradient force, the u / v sums    Main/mod_tendency.F90:257-294, 398-411

(The Coriolis term is `curvature`, called before `boundary`: u and v take advection, Coriolis,
relaxation, diffusion and then the two pressure-gradient terms.)

Arrays are (k, i, j) with the Fortran point (j, i, k) at [k - 1, i - 1, j - 1]; cross fields hold
i = 1..iy-1, j = 1..jx-1 (the last row and column are unused); in a periodic direction the cross grid
takes every point and a neighbour past the end is the one at the other end.
"""
import contextlib
import math

import numpy as np

EGRAV = 9.80665                 # Share/mod_constants.F90:85
REGRAV = 1.0 / EGRAV            # :182
VONKAR = 0.4                    # :296
MINQQ = 1.0e-8
EP1 = 28.96454 / 18.01528 - 1.0  # amd / amw - 1 (:303)
Z4 = (1.0, -4.0, 12.0)          # z4_c1..3, Main/mod_diffusion.F90:69-71
O4 = (4.0 / 6.0, 1.0 / 6.0, -20.0 / 6.0)   # o4_c1..3, :63-65
H4 = (10.0, -5.0, 1.0)          # h4_c1..3, :75-77
DIFF_6TH_FACTOR = 0.12          # :78
T00PG, P00PG, ALAM = 287.0, 101.325, 6.5e-3   # t00pg, p00pg, alam (:359-361); pgfaa1 = alam*rgas*regrav (:362)
SOUTH, NORTH, WEST, EAST = 1, 2, 3, 4


# ------------------------------------------------------------------------------ the grid
class Geom:
    """The sides the whole grid has and the 1-based loop ranges of the text, from i_band, i_crm, jx, iy.

    bandflag makes j periodic and crmflag i (Main/mpplib/mod_mppparam.F90:1104-1132): a periodic
    direction has no boundary side (has_bdyleft / right under the band, has_bdybottom / top under
    CRM are false).  The dot grid is 1..jx x 1..iy; the cross grid ends one short of it, but "takes
    all points" in a periodic direction (:1338-1360).  The interior ranges step in by one (jdi, jci)
    and by two (jdii, jcii) on the sides that exist only (Main/mod_atm_interface.F90:231-286)."""

    def __init__(self, jx, iy, band=False, crm=False):
        self.jx, self.iy = jx, iy
        self.perj, self.peri = bool(band), bool(crm)
        self.left = self.right = not self.perj                   # has_bdyleft, has_bdyright
        self.bottom = self.top = not self.peri                   # has_bdybottom, has_bdytop
        # the dot grid (:231-258)
        self.jde1 = self.jdi1 = self.jdii1 = 1
        self.jde2 = self.jdi2 = self.jdii2 = jx
        self.ide1 = self.idi1 = self.idii1 = 1
        self.ide2 = self.idi2 = self.idii2 = iy
        if self.left:
            self.jdi1, self.jdii1 = self.jde1 + 1, self.jde1 + 2
        if self.right:
            self.jdi2, self.jdii2 = self.jde2 - 1, self.jde2 - 2
        if self.bottom:
            self.idi1, self.idii1 = self.ide1 + 1, self.ide1 + 2
        if self.top:
            self.idi2, self.idii2 = self.ide2 - 1, self.ide2 - 2
        # the cross grid (:259-286), one short of the dot grid but in a periodic direction
        self.jce1 = self.jci1 = self.jcii1 = 1
        self.jce2 = self.jci2 = self.jcii2 = jx if self.perj else jx - 1
        self.ice1 = self.ici1 = self.icii1 = 1
        self.ice2 = self.ici2 = self.icii2 = iy if self.peri else iy - 1
        if self.left:
            self.jci1, self.jcii1 = self.jce1 + 1, self.jce1 + 2
        if self.right:
            self.jci2, self.jcii2 = self.jce2 - 1, self.jce2 - 2
        if self.bottom:
            self.ici1, self.icii1 = self.ice1 + 1, self.ice1 + 2
        if self.top:
            self.ici2, self.icii2 = self.ice2 - 1, self.ice2 - 2

    def rect(self, j1, j2, i1, i2):
        """[i, j] of the 1-based j1..j2 x i1..i2."""
        m = np.zeros((self.iy, self.jx), dtype=bool)
        m[i1 - 1:i2, j1 - 1:j2] = True
        return m

    def box(self, which, dot):
        """The mask of a named range: which = 'e' (jde x ide / jce x ice), 'i' or 'ii'."""
        if dot:
            r = {"e": (self.jde1, self.jde2, self.ide1, self.ide2), "i": (self.jdi1, self.jdi2, self.idi1, self.idi2),
                 "ii": (self.jdii1, self.jdii2, self.idii1, self.idii2)}
        else:
            r = {"e": (self.jce1, self.jce2, self.ice1, self.ice2), "i": (self.jci1, self.jci2, self.ici1, self.ici2),
                 "ii": (self.jcii1, self.jcii2, self.icii1, self.icii2)}
        return self.rect(*r[which])

    def lines(self, dot):
        """The masks of the first interior lines on the sides that exist, in the text's order west,
        east, south, north (j = jdi1 / jci1, jdi2 / jci2, i = idi1 / ici1, idi2 / ici2)."""
        jj, ii = np.meshgrid(np.arange(1, self.jx + 1), np.arange(1, self.iy + 1))
        j1, j2, i1, i2 = ((self.jdi1, self.jdi2, self.idi1, self.idi2) if dot else
                          (self.jci1, self.jci2, self.ici1, self.ici2))
        cand = ((self.left, jj == j1), (self.right, jj == j2), (self.bottom, ii == i1), (self.top, ii == i2))
        return [m for has, m in cand if has]

    def pad(self, a, n):
        """a with n more points on each side of its last two axes: the periodic neighbours in a
        periodic direction, zeros past a side that exists."""
        a = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(n, n)], mode="wrap" if self.perj and _WRAP else "constant")
        return np.pad(a, [(0, 0)] * (a.ndim - 2) + [(n, n), (0, 0)], mode="wrap" if self.peri and _WRAP else "constant")


def geom(rc):
    return Geom(rc.jx, rc.iy, getattr(rc, "i_band", 0) == 1, getattr(rc, "i_crm", 0) == 1)


_WRAP = True


@contextlib.contextmanager
def zero_pad_for_the_wrap():
    """A mutant of the whole module, for the tests' non-vacuity asserts: inside it a neighbour past
    the end of the grid is zero, the limited-area pad, where a periodic direction has the point at
    the other end (sh and Geom.pad).  The ranges stay those of the grid."""
    global _WRAP
    _WRAP = False
    try:
        yield
    finally:
        _WRAP = True


def twt(rc):
    """(twt1, twt2), twt(k,1) and twt(k,2) indexed by the 1-based k = 2..kz (Main/mod_params.F90):
    the weights that take half-level values k and k - 1 to the full level k."""
    kz, sig = rc.kz, rc.sigma
    hsig = (sig[1:] + sig[:-1]) * 0.5
    twt1, twt2 = np.zeros(kz + 1), np.zeros(kz + 1)
    for k in range(2, kz + 1):
        twt1[k] = (sig[k - 1] - hsig[k - 2]) / (hsig[k - 1] - hsig[k - 2])
        twt2[k] = 1.0 - twt1[k]
    return twt1, twt2


# ------------------------------------------------------------------------------ the band
def band_sides(rc, dot):
    """{(j, i): (side, ibnd)} of setup_boundaries for ba_dt (dot: icx = icy = 0, nspgd) or ba_cr
    (nspgx), on the points the nudge and sponge loops visit (jdi x idi or jci x ici).  The four sides
    do not overlap (asserted).  Under crmflag the band is empty (:434); under bandflag (:435-457) it
    is the south and north rows at every j, with no corner rule.  The band branch's `if ( j < jgbl1
    .and. j > jgbr2 ) cycle` asks for j < 2 and j > jx - icx - 1 at once, which no j satisfies: it is
    restated as written and never skips."""
    jx, iy = rc.jx, rc.iy
    G = geom(rc)
    nsp = rc.nspgd if dot else rc.nspgx
    ic = 0 if dot else 1
    igbb1, igbb2, jgbl1, jgbl2 = 2, nsp - 1, 2, nsp - 1
    igbt1, igbt2 = iy - ic - nsp + 2, iy - ic - 1
    jgbr1, jgbr2 = jx - ic - nsp + 2, jx - ic - 1
    out = {}

    def put(j, i, side, ib):
        assert (j, i) not in out, (j, i)
        out[(j, i)] = (side, ib)

    def visited(o):
        m = G.box("i", dot)
        return {p: v for p, v in o.items() if m[p[1] - 1, p[0] - 1]}
    if G.peri:
        return {}
    if G.perj:
        for i in range(1, iy + 1):
            if igbb1 <= i <= igbb2:
                for j in range(1, jx + 1):
                    if j < jgbl1 and j > jgbr2:
                        continue
                    put(j, i, SOUTH, i - igbb1 + 2)
        for i in range(1, iy + 1):
            if igbt1 <= i <= igbt2:
                for j in range(1, jx + 1):
                    if j < jgbl1 and j > jgbr2:
                        continue
                    put(j, i, NORTH, igbt2 - i + 2)
        return visited(out)
    for i in range(1, iy + 1):
        if igbb1 <= i <= igbb2:
            for j in range(1, jx + 1):
                if jgbl1 <= j <= jgbr2:
                    if j <= jgbl2 and i >= j:
                        continue
                    if j >= jgbr1 and i >= (jgbr2 - j + 2):
                        continue
                    put(j, i, SOUTH, i - igbb1 + 2)
    for i in range(1, iy + 1):
        if igbt1 <= i <= igbt2:
            for j in range(1, jx + 1):
                if jgbl1 <= j <= jgbr2:
                    if j <= jgbl2 and (igbt2 - i + 2) >= j:
                        continue
                    if j >= jgbr1 and (igbt2 - i) >= (jgbr2 - j):
                        continue
                    put(j, i, NORTH, igbt2 - i + 2)
    for i in range(1, iy + 1):
        if i < igbb1 or i > igbt2:
            continue
        for j in range(1, jx + 1):
            if jgbl1 <= j <= jgbl2:
                if i < igbb2 and j > i:
                    continue
                if i > igbt1 and j > (igbt2 - i + 2):
                    continue
                put(j, i, WEST, j - jgbl1 + 2)
    for i in range(1, iy + 1):
        if i < igbb1 or i > igbt2:
            continue
        for j in range(1, jx + 1):
            if jgbr1 <= j <= jgbr2:
                if i < igbb2 and (jgbr2 - j + 2) > i:
                    continue
                if i > igbt1 and (jgbr2 - j) > (igbt2 - i):
                    continue
                put(j, i, EAST, jgbr2 - j + 2)
    return visited(out)


def band(rc, dot=False):
    """{(j, i): ibnd} of the relaxation band on cross (ba_cr) or dot (ba_dt) points."""
    return {p: ib for p, (_, ib) in band_sides(rc, dot).items()}


def band_mask(rc, dot=False):
    m = np.zeros((rc.iy, rc.jx), dtype=bool)
    for (j, i) in band_sides(rc, dot):
        m[i - 1, j - 1] = True
    return m


def domain_mask(rc, dot=False):
    """[i, j] of jdi x idi (dot) or jci x ici."""
    return geom(rc).box("i", dot)


def ring_masks(rc, dot=False):
    """(ring, corners): the second-order lines jdi1 / jdi2 / idi1 / idi2 (or the cross ones) on the
    sides that exist, and the corners where two of them meet (none on a band)."""
    G = geom(rc)
    dom = G.box("i", dot)
    ring = dom & ~G.box("ii", dot)
    count = np.zeros(dom.shape, dtype=int)
    for line in G.lines(dot):
        count += (line & dom)
    assert np.array_equal(count > 0, ring)
    return ring, count > 1


# ------------------------------------------------------------------------------ the coefficient tables
def tables(rc):
    """setup_bdycon: tables indexed [n] (fcx, gcx, fcd, gcd, wgtx, wgtd; n = 2..nsp-1) and [n, k - 1]
    (hefc, hegc, hefd, hegd).  Every table is stated for every iboudy; the callers pick."""
    kz = rc.kz
    sig = rc.sigma
    hsig = (sig[1:] + sig[:-1]) * 0.5
    fnudge = rc.bdy_nm if rc.bdy_nm > 0.0 else 0.1 / rc.dt
    gnudge = rc.bdy_dm if rc.bdy_dm > 0.0 else 1.0 / (rc.dt * 50.0)
    t = dict(fnudge=fnudge, gnudge=gnudge)
    for tag, nsp in (("x", rc.nspgx), ("d", rc.nspgd)):
        f, g = np.zeros(nsp + 1), np.zeros(nsp + 1)
        for n in range(2, nsp):
            xfun = float(nsp - n) / float(nsp - 2)
            f[n], g[n] = fnudge * xfun, gnudge * xfun
        t["fc" + tag], t["gc" + tag] = f, g
    wd, wx = np.ones(max(rc.nspgd + 1, 6)), np.ones(max(rc.nspgx + 1, 5))
    wd[2:6] = (0.20, 0.55, 0.80, 0.95)
    wx[2:5] = (0.4, 0.7, 0.9)
    t["wgtd"], t["wgtx"] = wd, wx
    anudge = [rc.high_nudge if h < 0.4 else rc.medium_nudge if h < 0.8 else rc.low_nudge for h in hsig]
    for tag, nsp in (("c", rc.nspgx), ("d", rc.nspgd)):
        f, g = np.zeros((nsp + 1, kz)), np.zeros((nsp + 1, kz))
        for k in range(kz):
            for n in range(2, nsp):
                xfun = math.exp(-(float(n - 2) / anudge[k]))
                f[n, k], g[n, k] = fnudge * xfun, gnudge * xfun
        t["hef" + tag], t["heg" + tag] = f, g
    return t


# ------------------------------------------------------------------------------ slices
def psc2psd(pc, G=None):
    """psdot from the cross p* (iy, jx) on the whole grid as one tile; G: the grid (default: a limited
    area).  The interior form over jdi x idi, whose j - 1 (and i - 1 under CRM) is the periodic
    neighbour where the direction is periodic; the two-point edge lines (each over jdi or idi) and
    the corners only on the sides that exist (has_bdytop .., has_bdybottomleft ..)."""
    iy, jx = pc.shape
    G = G or Geom(jx, iy)
    pd = np.zeros_like(pc)
    inner = G.box("i", True)
    pd[inner] = ((pc + sh(pc, 0, -1) + sh(pc, -1, 0) + sh(pc, -1, -1)) * 0.25)[inner]
    js, is_ = slice(G.jdi1 - 1, G.jdi2), slice(G.idi1 - 1, G.idi2)
    if G.top:
        pd[G.ide2 - 1, js] = ((pc[G.ice2 - 1] + sh(pc, -1, 0)[G.ice2 - 1]) * 0.5)[js]
    if G.bottom:
        pd[G.ide1 - 1, js] = ((pc[G.ice1 - 1] + sh(pc, -1, 0)[G.ice1 - 1]) * 0.5)[js]
    if G.left:
        pd[is_, G.jde1 - 1] = ((pc[:, G.jce1 - 1] + sh(pc, 0, -1)[:, G.jce1 - 1]) * 0.5)[is_]
    if G.right:
        pd[is_, G.jde2 - 1] = ((pc[:, G.jce2 - 1] + sh(pc, 0, -1)[:, G.jce2 - 1]) * 0.5)[is_]
    if G.left and G.bottom:
        pd[G.ide1 - 1, G.jde1 - 1] = pc[G.ice1 - 1, G.jce1 - 1]
    if G.left and G.top:
        pd[G.ide2 - 1, G.jde1 - 1] = pc[G.ice2 - 1, G.jce1 - 1]
    if G.right and G.bottom:
        pd[G.ide1 - 1, G.jde2 - 1] = pc[G.ice1 - 1, G.jce2 - 1]
    if G.right and G.top:
        pd[G.ide2 - 1, G.jde2 - 1] = pc[G.ice2 - 1, G.jce2 - 1]
    return pd


def b_slices(st, G=None):
    """mkslice's b-level exports: (ubd3d, vbd3d, tb3d, qvb3d, qcb3d, psdotb)."""
    psb = st["PSB"][0]
    pd = psc2psd(psb, G)
    with np.errstate(divide="ignore"):
        rpd = 1.0 / pd
    with np.errstate(divide="ignore", invalid="ignore"):       # the unused last row and column hold zeros
        rpsb = 1.0 / psb
        tb = st["ATM2_T"] * rpsb[None]
        qv = np.maximum(st["ATM2_QV"] * rpsb[None], MINQQ)
        qc = np.maximum(st["ATM2_QC"] * rpsb[None], 0.0) if "ATM2_QC" in st else None
    return st["ATM2_U"] * rpd[None], st["ATM2_V"] * rpd[None], tb, qv, qc, pd


# ------------------------------------------------------------------------------ calc_coeff
def _hgfact(rc, ht, xkhz):
    iy, jx = rc.iy, rc.jx
    dx = rc.ds * 1000.0
    hg = np.full((iy, jx), xkhz)
    if rc.diffu_hgtf == 1:
        m = geom(rc).box("i", False)                             # jci x ici (:131-140)
        hg1 = np.abs((ht - sh(ht, 0, -1)) / dx)
        hg2 = np.abs((ht - sh(ht, 0, 1)) / dx)
        hg3 = np.abs((ht - sh(ht, -1, 0)) / dx)
        hg4 = np.abs((ht - sh(ht, 1, 0)) / dx)
        hgmax = np.maximum(np.maximum(hg1, hg2), np.maximum(hg3, hg4)) * REGRAV * 1.0e3
        hg[m] = (xkhz / (1.0 + hgmax * hgmax))[m]
    return hg


def _deformation(ud, vd):
    """(dudx - dvdy)^2 + (dvdx + dudy)^2 at every point (:198-206); the callers keep jce x ice, where
    j + 1 and i + 1 are dot points of the grid or, past the end of a periodic direction, the first."""
    def q(a):
        return a, sh(a, 1, 0), sh(a, 0, 1), sh(a, 1, 1)          # (j,i) (j+1,i) (j,i+1) (j+1,i+1)
    u00, u10, u01, u11 = q(ud)
    v00, v10, v01, v11 = q(vd)
    dudx = u10 + u11 - u00 - u01
    dvdx = v10 + v11 - v00 - v01
    dudy = u01 + u11 - u00 - u10
    dvdy = v01 + v11 - v00 - v10
    return (dudx - dvdy) * (dudx - dvdy) + (dvdx + dudy) * (dvdx + dudy)


def _scale_coeff(rc, raw, psb, pd):
    """xkd as the four-point mean of the unscaled xkc (:237-240), then both x rdxsq x p* (:241-249)."""
    G = geom(rc)
    dx = rc.ds * 1000.0
    rdxsq = 1.0 / (dx * dx)
    md, mc = G.box("i", True)[None], G.box("i", False)[None]
    xkd_raw = np.where(md, 0.25 * (raw + sh(raw, -1, -1) + sh(raw, -1, 0) + sh(raw, 0, -1)), 0.0)
    xkc = np.where(mc, raw * rdxsq * psb[None], 0.0)
    xkd = np.where(md, xkd_raw * rdxsq * pd[None], 0.0)
    return dict(xkc_raw=raw, xkd_raw=xkd_raw, xkc=xkc, xkd=xkd)


def coeff6(rc, st):
    """calc_coeff at idiffu = 3, either core (:174-183): xkc = diff_6th_coef p*b on jci x ici (every
    level alike; xkcf is the same on kz + 1 levels), xkd = diff_6th_coef p*dotb on jdi x idi, with
    diff_6th_coef = diff_6th_factor * 0.015625 / (2 dtsec) (:154); zero elsewhere.  st: PSB."""
    G = geom(rc)
    coef = DIFF_6TH_FACTOR * 0.015625 / (2.0 * rc.dt)
    psb = st["PSB"][0]
    pd = psc2psd(psb, G)
    one = np.ones((rc.kz, 1, 1))
    xkc = np.where(G.box("i", False)[None], one * (coef * psb)[None], 0.0)
    xkd = np.where(G.box("i", True)[None], one * (coef * pd)[None], 0.0)
    return dict(xkc=xkc, xkd=xkd)


def hydro_coeff(rc, st):
    """calc_coeff of the hydrostatic core: xkc_raw on ice x jce, xkd_raw on idi x jdi, and the scaled
    xkc (ici x jci) and xkd (idi x jdi); zero elsewhere.  st: ATM2_U, ATM2_V, PSB, HT."""
    if rc.idiffu == 3:
        return coeff6(rc, st)
    dx = rc.ds * 1000.0
    dxsq = dx * dx
    xkhmax = dxsq / (64.0 * rc.dt)
    dydc = rc.adyndif * VONKAR * VONKAR * dx * 0.25
    xkhz = rc.ckh * 1.5e-3 * dxsq / rc.dt
    psb = st["PSB"][0]
    G = geom(rc)
    pd = psc2psd(psb, G)
    with np.errstate(divide="ignore", invalid="ignore"):
        rpd = 1.0 / pd
        ud, vd = st["ATM2_U"] * rpd[None], st["ATM2_V"] * rpd[None]
        hg = _hgfact(rc, st["HT"][0], xkhz)
        duv = np.sqrt(_deformation(ud, vd))
        raw = np.where(G.box("e", False)[None], np.minimum(hg[None] + dydc * duv, xkhmax), 0.0)
    return _scale_coeff(rc, raw, psb, pd)


def nh_coeff(rc, st):
    """calc_coeff of the non-hydrostatic core (:212-230): the deformation less the vertical-velocity
    term, floored at zero, xkhz = ckh dx and twice the hydrostatic xkhmax (:110-113).  st: ATM2_U,
    ATM2_V, ATM2_W, PSB (and HT where diffu_hgtf = 1)."""
    if rc.idiffu == 3:
        return coeff6(rc, st)
    iy, jx = rc.iy, rc.jx
    dx = rc.ds * 1000.0
    dxsq = dx * dx
    xkhmax = 2.0 * (dxsq / (64.0 * rc.dt))
    dydc = rc.adyndif * VONKAR * VONKAR * dx * 0.25
    xkhz = rc.ckh * dx
    psb = st["PSB"][0]
    G = geom(rc)
    pd = psc2psd(psb, G)
    with np.errstate(divide="ignore", invalid="ignore"):
        rpd = 1.0 / pd
        ud, vd = st["ATM2_U"] * rpd[None], st["ATM2_V"] * rpd[None]
        wb = st["ATM2_W"] * (1.0 / psb)[None]
        hg = _hgfact(rc, st["HT"][0], xkhz) if rc.diffu_hgtf == 1 else np.full((iy, jx), xkhz)
        dwdz = wb[:-1] - wb[1:]
        duv = np.sqrt(np.maximum(_deformation(ud, vd) - dwdz * dwdz, 0.0))
        raw = np.where(G.box("e", False)[None], np.minimum(hg[None] + dydc * duv, xkhmax), 0.0)
    return _scale_coeff(rc, raw, psb, pd)


def nh_xkc(rc, st):
    """The scaled NH xkc on jci x ici (what the tracers and the budget read)."""
    return nh_coeff(rc, st)["xkc"]


# ------------------------------------------------------------------------------ diffusion
def tile_columns(rc, dot, tiles=None):
    """[(j, i1, i2)], 1-based and global: the one column j = jdi2 (dot) or jci2 (cross) of each tile
    with its rows idi1..idi2 / ici1..ici2, which is all that the idiffu = 3 loops visit
    (`do j = jdi2 , jdi2`, `do j = jci2 , jci2`).  tiles: [(ext, bdy)] of the decomposition, ext =
    (jde1, jde2, ide1, ide2, jce1, jce2, ice1, ice2), bdy = (left, right, bottom, top) the domain
    sides the tile touches; None is the single tile.  jdi2 = jde2 - 1 on the right side and jde2
    off it, and so on (Main/mod_atm_interface.F90:231-286)."""
    if tiles is None:
        G = geom(rc)
        tiles = [((G.jde1, G.jde2, G.ide1, G.ide2, G.jce1, G.jce2, G.ice1, G.ice2),
                  (G.left, G.right, G.bottom, G.top))]
    out = []
    for ext, (_, right, bottom, top) in tiles:
        j2, i1, i2 = (ext[1], ext[2], ext[3]) if dot else (ext[5], ext[6], ext[7])
        out.append((j2 - (1 if right else 0), i1 + (1 if bottom else 0), i2 - (1 if top else 0)))
    return out


def fluxes6(rc, fv, lv, cols, dot):
    """The four fluxes of the idiffu = 3 scheme on the columns cols: {name: (raw, limited)} for
    x_p0, x_p1, y_p0, y_p1, each (nk, iy, jx) and zero off the columns, and the mask [i, j] of the
    points.  fv: the values the fluxes difference, lv: those the limiter differences (dot: both
    u / msfd; cross: f and f / msfd(j, i), the dot-point map factor at the same indices, as the text
    has it, :621, 755, 912).  im1..ip3 and jm1..jp3 are clamped to 1 and iy / jx (dot, :415-427) or
    iym1 / jxm1 (cross, :605-617), in global indices: on an interior tile edge the clamp does not
    act.  A flux is zeroed where flux * (the limiter's difference) <= 0."""
    jmax, imax = (rc.jx, rc.iy) if dot else (rc.jx - 1, rc.iy - 1)
    names = ("x_p0", "x_p1", "y_p0", "y_p1")
    out = {n: (np.zeros_like(fv), np.zeros_like(fv)) for n in names}
    mask = np.zeros((rc.iy, rc.jx), dtype=bool)
    for j, i1, i2 in cols:
        i = np.arange(i1, i2 + 1)
        jm1, jm2, jm3 = max(j - 1, 1), max(j - 2, 1), max(j - 3, 1)
        jp1, jp2, jp3 = min(j + 1, jmax), min(j + 2, jmax), min(j + 3, jmax)
        im1, im2, im3 = np.maximum(i - 1, 1), np.maximum(i - 2, 1), np.maximum(i - 3, 1)
        ip1, ip2, ip3 = np.minimum(i + 1, imax), np.minimum(i + 2, imax), np.minimum(i + 3, imax)

        def F(jj, ii):
            return fv[:, ii - 1, jj - 1]

        def L(jj, ii):
            return lv[:, ii - 1, jj - 1]
        raw = dict(
            x_p0=(H4[0] * (F(j, i) - F(jm1, i)) + H4[1] * (F(jp1, i) - F(jm2, i)) + H4[2] * (F(jp2, i) - F(jm3, i)),
                  L(j, i) - L(jm1, i)),
            x_p1=(H4[0] * (F(jp1, i) - F(j, i)) + H4[1] * (F(jp2, i) - F(jm1, i)) + H4[2] * (F(jp3, i) - F(jm2, i)),
                  L(jp1, i) - L(j, i)),
            y_p0=(H4[0] * (F(j, i) - F(j, im1)) + H4[1] * (F(j, ip1) - F(j, im2)) + H4[2] * (F(j, ip2) - F(j, im3)),
                  L(j, i) - L(j, im1)),
            y_p1=(H4[0] * (F(j, ip1) - F(j, i)) + H4[1] * (F(j, ip2) - F(j, im1)) + H4[2] * (F(j, ip3) - F(j, im2)),
                  L(j, ip1) - L(j, i)))
        for n in names:
            fl, dl = raw[n]
            out[n][0][:, i - 1, j - 1] = fl
            out[n][1][:, i - 1, j - 1] = np.where(fl * dl <= 0.0, 0.0, fl)
        mask[i - 1, j - 1] = True
    return out, mask


def diffu6(rc, fv, lv, xk, cols, dot, fac=None):
    """The one add of an idiffu = 3 call: (fac *) xk * ((x_p1 - x_p0) + (y_p1 - y_p0)) on the columns
    (fac: diffu_x3df's alone, :646; diffu_x4d3d ignores its fac here, :937)."""
    fl, mask = fluxes6(rc, fv, lv, cols, dot)
    br = (fl["x_p1"][1] - fl["x_p0"][1]) + (fl["y_p1"][1] - fl["y_p0"][1])
    inc = xk * br if fac is None else fac * xk * br
    return [np.where(mask[None], inc, 0.0)]


def _diffu(rc, fm, xk, dot, fac=None):
    """The increments of one diffu_* call, in the order the text adds them: idiffu = 1: the
    fourth-order interior (jdii x idii / jcii x icii), then the second-order lines west, east, south,
    north on the sides that exist (`if ( ma%has_bdyleft )` .., :552-591; the corners lie on two lines
    and take two adds); idiffu = 2: the nine-point form on the whole jdi x idi / jci x ici.  A
    neighbour past the end of a periodic direction is the one at the other end; on a band the
    fourth-order form covers every j and only the south and north lines exist.  fm, xk: (nk, iy, jx);
    each increment is zero off its support.  fac: diffu_x3df's, which multiplies the coefficient
    first (fac * xkcf * (...))."""
    iy, jx = rc.iy, rc.jx
    G = geom(rc)
    if fac is not None:
        xk = fac * xk
    with np.errstate(invalid="ignore"):
        P = G.pad(fm, 2)

        def F(dj, di):
            return P[:, 2 + di:2 + di + iy, 2 + dj:2 + dj + jx]
        dom = G.box("i", dot)
        if rc.idiffu == 2:
            inc = xk * (O4[0] * (F(1, 0) + F(-1, 0) + F(0, 1) + F(0, -1)) +
                        O4[1] * (F(1, 1) + F(-1, -1) + F(-1, 1) + F(1, -1)) + O4[2] * fm)
            return [np.where(dom[None], inc, 0.0)]
        assert rc.idiffu == 1
        inner = G.box("ii", dot)
        fourth = -(xk * (Z4[0] * (F(2, 0) + F(-2, 0) + F(0, 2) + F(0, -2)) +
                         Z4[1] * (F(1, 0) + F(-1, 0) + F(0, 1) + F(0, -1)) + Z4[2] * fm))
        second = xk * (Z4[0] * (F(1, 0) + F(-1, 0) + F(0, 1) + F(0, -1)) + Z4[1] * fm)
        out = [np.where(inner[None], fourth, 0.0)]
        for line in G.lines(dot):
            out.append(np.where((dom & line)[None], second, 0.0))
        return out


def diffu_x(rc, f, xkc, msfd=None, tiles=None):
    """diffu_x3d / diffu_x4d3d (fac = 1) of the decoupled cross field f: the list of increments.
    idiffu = 3 needs msfd (its limiter) and takes the tiles of tile_columns."""
    if rc.idiffu == 3:
        with np.errstate(divide="ignore", invalid="ignore"):
            return diffu6(rc, f, f / msfd[None], xkc, tile_columns(rc, False, tiles), dot=False)
    return _diffu(rc, f, xkc, dot=False)


def diffu_d(rc, u, v, xkd, msfd, tiles=None):
    """diffu_d of ubd3d, vbd3d (each value divided by msfd at its own point): (u incs, v incs)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        um, vm = u / msfd[None], v / msfd[None]
        if rc.idiffu == 3:
            cols = tile_columns(rc, True, tiles)
            return diffu6(rc, um, um, xkd, cols, dot=True), diffu6(rc, vm, vm, xkd, cols, dot=True)
        return _diffu(rc, um, xkd, dot=True), _diffu(rc, vm, xkd, dot=True)


def apply(ften, incs):
    """ften + inc, one increment after the other (each its own rounded addition)."""
    for a in incs:
        ften = ften + a
    return ften


def total(incs):
    return apply(np.zeros_like(incs[0]), incs)


# ------------------------------------------------------------------------------ relaxation
def _lap(fg, G=None):
    """fls1 + fls2 + fls3 + fls4 - 4 fls0 (j-1, j+1, i-1, i+1), zero on the frame edge of a side that
    exists; j +- 1 (i +- 1) is the periodic neighbour in a periodic direction."""
    G = G or Geom(fg.shape[-1], fg.shape[-2])
    P = G.pad(fg, 1)
    out = P[..., 1:-1, :-2] + P[..., 1:-1, 2:] + P[..., :-2, 1:-1] + P[..., 2:, 1:-1] - 4.0 * fg
    edge = np.zeros(fg.shape[-2:], dtype=bool)
    if not G.perj:
        edge[:, 0] = edge[:, -1] = True
    if not G.peri:
        edge[0, :] = edge[-1, :] = True
    return np.where(edge, 0.0, out)


def _coef(rc, tab, dot, kind, nk):
    """(xf, xg) as (nk, iy, jx), zero off the band: iboudy 1 the linear fcx / gcx (fcd / gcd for u, v);
    iboudy 5 hefc / hegc(ib, k) for t and qv, (ib, kz) for p*, and for u, v hefc / hegc on the south
    side, hefd / hegd on the other three (:3720, 3746, 3772, 3798); each side's loop names its table,
    so on a band, which has no west or east side, the south dot points take hefc / hegc and the north
    ones hefd / hegd."""
    xf, xg = np.zeros((nk, rc.iy, rc.jx)), np.zeros((nk, rc.iy, rc.jx))
    for (j, i), (side, ib) in band_sides(rc, dot).items():
        if rc.iboudy == 1:
            f, g = (tab["fcd"][ib], tab["gcd"][ib]) if dot else (tab["fcx"][ib], tab["gcx"][ib])
        elif kind == "ps":
            f, g = tab["hefc"][ib, rc.kz - 1], tab["hegc"][ib, rc.kz - 1]
        elif dot and side != SOUTH:
            f, g = tab["hefd"][ib], tab["hegd"][ib]
        else:
            f, g = tab["hefc"][ib], tab["hegc"][ib]
        xf[:, i - 1, j - 1], xg[:, i - 1, j - 1] = f, g
    return xf, xg


def nudge(rc, f, b0, bt, xt, kind, tab=None):
    """The relaxation increments of one field (iboudy 1 or 5), in the order the text adds them.
    kind 't', 'u', 'v', 'ps': ften + xf fls0 - xg (...), two additions: [xf fls0, -(xg (...))];
    kind 'qv': ften + rfac (xf fls0 - xg (...)), one addition.  f: atm2 (coupled)."""
    tab = tab or tables(rc)
    dot = kind in ("u", "v")
    if kind == "qv":
        nfac = 1.0e3
        rfac = 1.0 / nfac
        fg = nfac * (b0 + xt * bt) - nfac * f
    else:
        fg = (b0 + xt * bt) - f
    xf, xg = _coef(rc, tab, dot, kind, f.shape[0])
    G = geom(rc)
    if kind == "qv":
        return [rfac * (xf * fg - xg * _lap(fg, G))]
    return [xf * fg, -(xg * _lap(fg, G))]


def sponge(rc, ften, bt, dot, tab=None):
    """sponge*: wgt(ib) ften + (1 - wgt(ib)) bt on the band, ften elsewhere (iboudy = 4)."""
    tab = tab or tables(rc)
    w = np.ones((rc.iy, rc.jx))
    m = np.zeros((rc.iy, rc.jx), dtype=bool)
    wgt = tab["wgtd" if dot else "wgtx"]
    for (j, i), (_, ib) in band_sides(rc, dot).items():
        w[i - 1, j - 1], m[i - 1, j - 1] = wgt[ib], True
    return np.where(m, w * ften + (1.0 - w) * bt, ften)


# ------------------------------------------------------------------------------ the hydrostatic tend
HYDRO_INPUTS = ("ATM1_U", "ATM1_V", "ATM1_T", "ATM1_QV", "ATM1_QC", "ATM2_U", "ATM2_V", "ATM2_T", "ATM2_QV",
                "ATM2_QC", "PSA", "PSB", "MSFX", "MSFD", "CORIOL", "HT", "XUB_B0", "XUB_BT", "XVB_B0", "XVB_BT",
                "XTB_B0", "XTB_BT", "XQB_B0", "XQB_BT", "XPSB_B0", "XPSB_BT")


def sh(a, dj, di):
    """sh(a)[k, i, j] = a[k, i + di, j + dj], around the end of the array (a periodic direction's
    neighbour; on a side that exists the callers never keep such a point)."""
    out = np.roll(a, shift=(-di, -dj), axis=(-2, -1))
    if not _WRAP:                                                # zero_pad_for_the_wrap
        ni, nj = a.shape[-2:]
        if di:
            out[..., (ni - di if di > 0 else 0):(ni if di > 0 else -di), :] = 0.0
        if dj:
            out[..., :, (nj - dj if dj > 0 else 0):(nj if dj > 0 else -dj)] = 0.0
    return out


class Sum:
    """A running tendency: the value after each addition and the largest |partial sum| so far."""

    def __init__(self, like):
        self.v = np.zeros_like(like)
        self.big = np.zeros_like(like)
        self.at = {}

    def add(self, incs, tag=None):
        for a in incs if isinstance(incs, list) else [incs]:
            self.v = self.v + a
            with np.errstate(invalid="ignore"):
                self.big = np.fmax(self.big, np.abs(self.v))
        if tag:
            self.at[tag] = self.v
        return self

    def put(self, v, tag):
        """Take a value formed in place by a column recurrence."""
        self.v = v
        with np.errstate(invalid="ignore"):
            self.big = np.fmax(self.big, np.abs(v))
        self.at[tag] = v


def compute_omega(rc, g):
    """compute_omega's cr x dummy (a product with the reciprocal), pten and qdot (kz + 1 levels, the
    first and the last zero) from atm1 u, v, p*a and the map factors: (cr, pten, qdot), on jce x ice
    and zero off it; j + 1 and i + 1 past the end of a periodic direction are the first points."""
    kz = rc.kz
    me = geom(rc).box("e", False)
    dsig = rc.sigma[1:] - rc.sigma[:-1]
    dx = rc.ds * 1000.0
    pa, msfx, msfd = g["PSA"][0], g["MSFX"][0], g["MSFD"][0]
    rpsa = np.divide(1.0, pa, out=np.zeros_like(pa), where=pa > 0)
    umc, vmc = g["ATM1_U"] * msfd, g["ATM1_V"] * msfd
    with np.errstate(divide="ignore", invalid="ignore"):         # frame edges: never compared
        dummy = 1.0 / ((2.0 * dx) * msfx * msfx)
        cr = ((sh(umc, 1, 1) + sh(umc, 1, 0) - sh(umc, 0, 1) - umc) +
              (sh(vmc, 1, 1) + sh(vmc, 0, 1) - sh(vmc, 1, 0) - vmc)) * dummy
        pten = np.zeros_like(pa)
        for k in range(kz):
            pten = pten - cr[k] * dsig[k]
        qdot = np.zeros((kz + 1,) + pa.shape)
        for k in range(2, kz + 1):
            qdot[k - 1] = qdot[k - 2] - (pten + cr[k - 2]) * dsig[k - 2] * rpsa
    return np.where(me[None], cr, 0.0), np.where(me, pten, 0.0), np.where(me[None], qdot, 0.0)


def decouple_uv(rc, g, psd):
    """decouple's atmx%ud, vd (Main/mod_tendency.F90:888-994): atm1 u, v times 1 / psdota; after bdyval
    the boundary slices wue .. nvi hold atm1 on their lines, so the boundary assignments change
    nothing but under iboudy 3 / 4, where an outflow edge value is the first interior line's (:908-918,
    933-943, 958-968, 983-993): west, east over idi, then south, north over jde (the corners read the
    lines just set), each only on a side that exists (`if ( ma%has_bdyleft )` ..)."""
    G = geom(rc)
    u1, v1 = g["ATM1_U"], g["ATM1_V"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rpsd = 1.0 / psd
        ud, vd = u1 * rpsd, v1 * rpsd
    if rc.iboudy in (3, 4):
        ri = slice(G.idi1 - 1, G.idi2)
        for a in (ud, vd):
            if G.left:
                a[:, ri, 0] = np.where(u1[:, ri, 0] <= 0.0, a[:, ri, 1], a[:, ri, 0])
            if G.right:
                a[:, ri, -1] = np.where(u1[:, ri, -1] >= 0.0, a[:, ri, -2], a[:, ri, -1])
            if G.bottom:
                a[:, 0, :] = np.where(v1[:, 0, :] >= 0.0, a[:, 1, :], a[:, 0, :])
            if G.top:
                a[:, -1, :] = np.where(v1[:, -1, :] <= 0.0, a[:, -2, :], a[:, -1, :])
    return ud, vd


NH_QDOT_INPUTS = ("ATM1_U", "ATM1_V", "ATM1_W", "PSA", "MSFD", "ATM0_RHOF", "ATM0_PS", "DPSDXM", "DPSDYM")


def nh_qdot(rc, g, swap_twt=False):
    """The idynamic = 2 branch of compute_omega (Main/mod_tendency.F90:1158-1178): qdot on kz + 1
    levels, the first and the last zero, on jce x ice and zero off it.

      ucc(j,i,k) = umd(j,i,k) + umd(j,i+1,k) + umd(j+1,i,k) + umd(j+1,i+1,k)          (vcc alike)
      qdot(j,i,k) = -rhof(j,i,k) egrav w(j,i,k) / ps0(j,i)
                    - sigma(k) (dpsdxm(j,i) (twt(k,1) ucc(k) + twt(k,2) ucc(k-1))
                                + dpsdym(j,i) (twt(k,1) vcc(k) + twt(k,2) vcc(k-1)))     k = 2..kz

    with atmx%umd = atmx%ud msfd (:1005-1008; ud is decouple_uv's, the inflow / outflow copies
    included) and atmx%w = atm1%w rpsa (:1051-1053).  No transcendental function.  swap_twt: a mutant
    for the tests' non-vacuity asserts (twt(k,1) and twt(k,2) exchanged)."""
    kz = rc.kz
    G = geom(rc)
    sig = rc.sigma
    twt1, twt2 = twt(rc)
    pa, msfd = g["PSA"][0], g["MSFD"][0]
    ud, vd = decouple_uv(rc, g, psc2psd(pa, G))
    qdot = np.zeros((kz + 1,) + pa.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        rpsa = 1.0 / pa
        umd, vmd = ud * msfd, vd * msfd
        xw = g["ATM1_W"] * rpsa
        ucc = (umd + sh(umd, 0, 1) + sh(umd, 1, 0) + sh(umd, 1, 1))
        vcc = (vmd + sh(vmd, 0, 1) + sh(vmd, 1, 0) + sh(vmd, 1, 1))
        for k in range(2, kz + 1):
            t1, t2 = (twt2[k], twt1[k]) if swap_twt else (twt1[k], twt2[k])
            qdot[k - 1] = (-g["ATM0_RHOF"][k - 1] * EGRAV * xw[k - 1] / g["ATM0_PS"][0] -
                           sig[k - 1] * (g["DPSDXM"][0] * (t1 * ucc[k - 1] + t2 * ucc[k - 2]) +
                                         g["DPSDYM"][0] * (t1 * vcc[k - 1] + t2 * vcc[k - 2])))
    return np.where(G.box("e", False)[None], qdot, 0.0)


def hydro_tend(rc, g, dt, xbc, relax=True, diffuse=True, revert=None, tiles=None):
    """One hydrostatic tend from the state g after bdyval (no physics tendencies), dt and xbctime
    as rcmdyn get_time returns them.  Returns the running sums of tdyn, qvdyn, qcdyn, udyn, vdyn after
    each process (`at`: adh, adv, adi / cor, bdy, dif, pgf), the increments of the relaxation and
    diffusion terms, the coefficients, pten before and after new_pressure, and the totals.
    relax / diffuse = False leave the process out (for a test's own on/off differences).
    rc.ipgf = 1 takes the reference-temperature branches of pressure_gradient_force; revert = "rtbar"
    or "phi" puts that one branch back to its ipgf = 0 form (a mutant for the tests' non-vacuity
    asserts).  tiles: the decomposition, which only idiffu = 3 depends on (tile_columns).  u_pgf / v_pgf:
    the two pressure-gradient increments, in the order they are added; phi: the geopotential."""
    from regcm_amd import constants as C
    kz = rc.kz
    sig = rc.sigma
    hsig = (sig[1:] + sig[:-1]) * 0.5
    dsig = sig[1:] - sig[:-1]
    twt1 = np.zeros(kz + 1); twt2 = np.zeros(kz + 1)
    for k in range(2, kz + 1):
        twt1[k] = (sig[k - 1] - hsig[k - 2]) / (hsig[k - 1] - hsig[k - 2])
        twt2[k] = 1.0 - twt1[k]
    dx = rc.ds * 1000.0
    ul = rc.uoffc * 0.5 * rc.dt / dx
    rgas = C.rgas
    cpd = 3.5 * rgas
    c287 = rgas / 1000.0                                         # Share/mod_constants.F90:132-134
    ptop = rc.ptop
    xt = xbc + dt
    tab = tables(rc)
    nudging = relax and rc.iboudy in (1, 5)
    sponging = relax and rc.iboudy == 4
    PGFAA1 = ALAM * rgas * REGRAV
    assert rc.ipgf in (0, 1) and rc.idynamic == 1 and revert in (None, "rtbar", "phi")

    u1, v1, t1, q1, qc1 = g["ATM1_U"], g["ATM1_V"], g["ATM1_T"], g["ATM1_QV"], g["ATM1_QC"]
    pa, pb = g["PSA"][0], g["PSB"][0]
    msfx, msfd = g["MSFX"][0], g["MSFD"][0]
    G = geom(rc)
    psd = psc2psd(pa, G)                                         # psdota, the edge lines included
    rpsa = np.divide(1.0, pa, out=np.zeros_like(pa), where=pa > 0)
    umc, vmc = u1 * msfd, v1 * msfd
    ud, vd = decouple_uv(rc, g, psd)
    old_err = np.seterr(divide="ignore", invalid="ignore")      # frame edges: never compared
    cr, pten, qdot = compute_omega(rc, g)
    # new_pressure: the boundary term of p*
    pten0 = pten.copy()                                          # on jce x ice, zero off it
    pinc = []
    if sponging:
        ptot = sponge(rc, pten0, g["XPSB_BT"][0], False, tab)
    else:
        if nudging:
            pinc = [a[0] for a in nudge(rc, g["PSB"], g["XPSB_B0"], g["XPSB_BT"], xt, "ps", tab)]
        ptot = apply(pten0, pinc)

    xtd = t1 * rpsa
    xq = np.maximum(q1 * rpsa, MINQQ)
    xc = np.maximum(qc1 * rpsa, 0.0)
    tv = xtd * (1.0 + EP1 * xq)
    u1a = sh(umc, 0, 1) + umc
    u2a = sh(umc, 1, 1) + sh(umc, 1, 0)
    v1a = sh(vmc, 1, 0) + vmc
    v2a = sh(vmc, 1, 1) + sh(vmc, 0, 1)
    f1 = 0.5 * ul * (u2a + u1a) / pa
    f2 = 0.5 * ul * (v2a + v1a) / pa
    xmsf = 1.0 / (msfx * msfx * (4.0 * dx))

    def hadv(c):
        w, e_, s_, n = sh(c, -1, 0), sh(c, 1, 0), sh(c, 0, -1), sh(c, 0, 1)
        fx1 = (1.0 + f1) * w + (1.0 - f1) * c
        fx2 = (1.0 + f1) * c + (1.0 - f1) * e_
        fy1 = (1.0 + f2) * s_ + (1.0 - f2) * c
        fy2 = (1.0 + f2) * c + (1.0 - f2) * n
        return -xmsf * (u2a * fx2 - u1a * fx1 + v2a * fy2 - v1a * fy1), w, e_, s_, n

    ub, vb, tb, qvb, qcb, pdb = b_slices(g, G)
    co = hydro_coeff(rc, g)
    if not diffuse:
        co = {k: np.zeros_like(v) for k, v in co.items()}

    # ---- t: hadvt (t_extrema limiter), vadv3d ind 1, the omega term, nudge3d, diffu_x3d
    T = Sum(t1)
    fg, w, e_, s_, n = hadv(xtd)
    for (p_, m_) in ((n, s_), (e_, w)):
        big = np.abs(p_ + m_ - 2.0 * xtd) / pa > rc.t_extrema
        fg = np.where(big & (xtd > p_) & (xtd > m_), np.minimum(fg, 0.0), fg)
        fg = np.where(big & (xtd < p_) & (xtd < m_), np.maximum(fg, 0.0), fg)
    T.add(fg, "adh")
    s2 = T.v.copy()
    pbh = (hsig[:, None, None] * pb + ptop) * 1000.0
    pbf = (sig[:, None, None] * pb + ptop) * 1000.0
    for k in range(2, kz + 1):
        dq = qdot[k - 1] * (twt1[k] * t1[k - 1] * (pbf[k - 1] / pbh[k - 1]) ** c287 +
                            twt2[k] * t1[k - 2] * (pbf[k - 1] / pbh[k - 2]) ** c287)
        s2[k - 2] = s2[k - 2] - dq * (1.0 / dsig[k - 2])
        s2[k - 1] = s2[k - 1] + dq * (1.0 / dsig[k - 1])
    T.put(s2, "adv")
    dum8 = 1.0 / (8.0 * dx * msfx)
    om = np.zeros_like(t1)
    for k in range(kz):
        om[k] = (0.5 * (qdot[k + 1] + qdot[k]) * pa + hsig[k] * (
            pten + ((ud[k] + sh(ud, 0, 1)[k] + sh(ud, 1, 1)[k] + sh(ud, 1, 0)[k]) * (sh(pa, 1, 0) - sh(pa, -1, 0)) +
                    (vd[k] + sh(vd, 0, 1)[k] + sh(vd, 1, 1)[k] + sh(vd, 1, 0)[k]) * (sh(pa, 0, 1) - sh(pa, 0, -1))) *
            dum8))
    rovcpm = rgas / (cpd * (1.0 + 0.80 * xq))
    T.add((om * rovcpm * tv) / (ptop * rpsa + hsig[:, None, None]), "adi")
    t_bdy = nudge(rc, g["ATM2_T"], g["XTB_B0"], g["XTB_BT"], xt, "t", tab) if nudging else []
    T.add(t_bdy, "bdy")
    t_dif = diffu_x(rc, tb, co["xkc"], msfd, tiles)
    T.add(t_dif, "dif")

    # ---- qv: hadvqv (q_rel_extrema limiter), vadvqv, nudge4d3d, diffu_x4d3d
    Q = Sum(t1)
    fq, w, e_, s_, n = hadv(xq)
    den = np.maximum(xq, 1.0e-20)
    for (p_, m_) in ((n, s_), (e_, w)):
        big = np.abs(p_ + m_ - 2.0 * xq) / den > rc.q_rel_extrema
        fq = np.where(big & (xq > p_) & (xq > m_), np.minimum(fq, 0.0), fq)
        fq = np.where(big & (xq < p_) & (xq < m_), np.maximum(fq, 0.0), fq)
    Q.add(fq, "adh")
    q2s = Q.v.copy()
    for k in range(2, kz + 1):
        qcon = (sig[k - 1] - hsig[k - 1]) / (hsig[k - 2] - hsig[k - 1])   # Main/mod_params.F90:2214
        fk, fkm = q1[k - 1], q1[k - 2]
        ok = (fk > MINQQ * pa) & (fkm > MINQQ * pa)
        flux = qdot[k - 1] * np.where(ok, fk * (fkm / fk) ** qcon, 0.0)
        q2s[k - 2] = q2s[k - 2] - flux * (1.0 / dsig[k - 2])
        q2s[k - 1] = q2s[k - 1] + flux * (1.0 / dsig[k - 1])
    Q.put(q2s, "adv")
    q_bdy = nudge(rc, g["ATM2_QV"], g["XQB_B0"], g["XQB_BT"], xt, "qv", tab) if nudging else []
    Q.add(q_bdy, "bdy")
    q_dif = diffu_x(rc, qvb, co["xkc"], msfd, tiles)
    Q.add(q_dif, "dif")

    # ---- qc: hadvqx, vadv4d ind 1, diffu_x4d3d (no relaxation of qc)
    Cq = Sum(t1)
    Cq.add(hadv(xc)[0], "adh")
    c2 = Cq.v.copy()
    for k in range(2, kz + 1):
        fk, fkm, svv = qc1[k - 1], qc1[k - 2], qdot[k - 1]
        thr = MINQQ * MINQQ * pa
        ok = np.where(svv > 0.0, fkm > thr, fk > thr)
        flux = np.where(ok, svv * (twt1[k] * fk + twt2[k] * fkm), 0.0)
        c2[k - 2] = c2[k - 2] - flux * (1.0 / dsig[k - 2])
        c2[k - 1] = c2[k - 1] + flux * (1.0 / dsig[k - 1])
    Cq.put(c2, "adv")
    c_dif = diffu_x(rc, qcb, co["xkc"], msfd, tiles)
    Cq.add(c_dif, "dif")

    # ---- u, v: hadvuv (hydrostatic upstream branch), vadvuv, Coriolis, nudgeuv, diffu_d, the
    # pressure-gradient force with ipgf = 0
    ucmona = sh(umc, 0, 1) + 2.0 * umc + sh(umc, 0, -1)
    ucmonb = sh(umc, 1, 1) + 2.0 * sh(umc, 1, 0) + sh(umc, 1, -1)
    ucmonc = sh(umc, -1, 1) + 2.0 * sh(umc, -1, 0) + sh(umc, -1, -1)
    vcmona = sh(vmc, 1, 0) + 2.0 * vmc + sh(vmc, -1, 0)
    vcmonb = sh(vmc, 1, 1) + 2.0 * sh(vmc, 0, 1) + sh(vmc, -1, 1)
    vcmonc = sh(vmc, 1, -1) + 2.0 * sh(vmc, 0, -1) + sh(vmc, -1, -1)
    ff1, ff2 = ul * (sh(ud, 1, 0) + ud), ul * (sh(ud, -1, 0) + ud)
    ff3, ff4 = ul * (sh(vd, 0, 1) + vd), ul * (sh(vd, 0, -1) + vd)
    ucb = (1.0 + ff1) * ucmona + (1.0 - ff1) * ucmonb
    ucc_ = (1.0 + ff2) * ucmonc + (1.0 - ff2) * ucmona
    vcb = (1.0 + ff3) * vcmona + (1.0 - ff3) * vcmonb
    vcc_ = (1.0 + ff4) * vcmonc + (1.0 - ff4) * vcmona
    dm = 1.0 / (msfd * msfd * 16.0 * dx)
    U, V = Sum(t1), Sum(t1)
    U.add(-dm * ((sh(ud, 1, 0) + ud) * ucb - (ud + sh(ud, -1, 0)) * ucc_ +
                 (sh(ud, 0, 1) + ud) * vcb - (ud + sh(ud, 0, -1)) * vcc_), "adh")
    V.add(-dm * ((sh(vd, 1, 0) + vd) * ucb - (vd + sh(vd, -1, 0)) * ucc_ +
                 (sh(vd, 0, 1) + vd) * vcb - (vd + sh(vd, 0, -1)) * vcc_), "adh")
    udyn, vdyn = U.v.copy(), V.v.copy()
    for k in range(2, kz + 1):                                   # vadvuv of atm1 u, v
        qq = 0.25 * (qdot[k - 1] + sh(qdot, 0, -1)[k - 1] + sh(qdot, -1, 0)[k - 1] + sh(qdot, -1, -1)[k - 1])
        uu = qq * (twt1[k] * u1[k - 1] + twt2[k] * u1[k - 2])
        vv = qq * (twt1[k] * v1[k - 1] + twt2[k] * v1[k - 2])
        udyn[k - 2] = udyn[k - 2] - uu / dsig[k - 2]
        udyn[k - 1] = udyn[k - 1] + uu / dsig[k - 1]
        vdyn[k - 2] = vdyn[k - 2] - vv / dsig[k - 2]
        vdyn[k - 1] = vdyn[k - 1] + vv / dsig[k - 1]
    U.put(udyn, "adv")
    V.put(vdyn, "adv")
    cor = g["CORIOL"][0]
    U.add(cor * v1, "cor")
    V.add(-(cor * u1), "cor")
    u_bdy = nudge(rc, g["ATM2_U"], g["XUB_B0"], g["XUB_BT"], xt, "u", tab) if nudging else []
    v_bdy = nudge(rc, g["ATM2_V"], g["XVB_B0"], g["XVB_BT"], xt, "v", tab) if nudging else []
    U.add(u_bdy, "bdy")
    V.add(v_bdy, "bdy")
    u_dif, v_dif = diffu_d(rc, ub, vb, co["xkd"], msfd, tiles)
    U.add(u_dif, "dif")
    V.add(v_dif, "dif")
    # pressure_gradient_force (Main/mod_tendency.F90:1886-2119).  ipgf = 1 (:1893-1964, 2039-2068)
    # takes the reference temperature t00pg ((sigma p* + ptop) / p00pg)**pgfaa1 off rtbar and off td
    # (ttld), and adds its column integral to phi(kz).
    h = hsig[:, None, None]
    rtbar = 0.25 * (sh(tv, -1, -1) + sh(tv, -1, 0) + sh(tv, 0, -1) + tv)
    if rc.ipgf == 1 and revert != "rtbar":
        rtbar = rtbar - T00PG * ((h * psd + ptop) / P00PG) ** PGFAA1           # :1937-1939
    rtbar = rgas * rtbar * psd
    u_pgf = [-(rtbar * (np.log(0.5 * (pa + sh(pa, 0, -1)) * h + ptop) -
                        np.log(0.5 * (sh(pa, -1, 0) + sh(pa, -1, -1)) * h + ptop)) / (dx * msfd))]
    v_pgf = [-(rtbar * (np.log(0.5 * (pa + sh(pa, -1, 0)) * h + ptop) -
                        np.log(0.5 * (sh(pa, -1, -1) + sh(pa, 0, -1)) * h + ptop)) / (dx * msfd))]
    U.add(u_pgf[0])
    V.add(v_pgf[0])
    # td: alpha_hyd = 0 and beta_hyd = 1 (Share/mod_constants.F90:319-320), so the interior's
    # alpha_hyd (tvc + tvb) + beta_hyd tva is tva exactly, the form of the four boundary lines
    # (:1906-1933), which read atm1 alone.  :1894 reads `do k = - 1 , kz`: td, ttld and atm1%t have
    # the lower bound 1 in k, so k = -1 and 0 lie outside every array the loop touches and hold no
    # defined value; the restatement takes k = 1..kz, the arrays' bounds and the range of the four
    # boundary loops and of every reader of td and ttld.
    td = t1 * (1.0 + EP1 * xq)
    tvfac = 1.0 / (1.0 + xc / (1.0 + xq))
    phi = np.zeros_like(t1)
    if rc.ipgf == 1 and revert != "phi":
        ttld = td - pa * T00PG * ((h * pa + ptop) / P00PG) ** PGFAA1            # :1901-1902
        phi[kz - 1] = g["HT"][0] + rgas * T00PG / PGFAA1 * ((pa + ptop) / P00PG) ** PGFAA1   # :2046-2047
        phi[kz - 1] = phi[kz - 1] - rgas * (ttld[kz - 1] * rpsa * tvfac[kz - 1]) * np.log(
            (hsig[kz - 1] + ptop * rpsa) / (1.0 + ptop * rpsa))
        td = ttld
    else:
        phi[kz - 1] = g["HT"][0] - rgas * (td[kz - 1] * rpsa * tvfac[kz - 1]) * np.log(
            (hsig[kz - 1] + ptop * rpsa) / (1.0 + ptop * rpsa))
    for lev in range(kz - 1, 0, -1):                             # 1-based lev = kz-1 .. 1
        tvavg = ((td[lev - 1] * dsig[lev - 1] + td[lev] * dsig[lev]) /
                 (pa * (dsig[lev - 1] + dsig[lev]))) * tvfac[lev - 1]
        phi[lev - 1] = phi[lev] - rgas * tvavg * np.log((hsig[lev - 1] + ptop * rpsa) / (hsig[lev] + ptop * rpsa))
    u_pgf.append(-(psd * (phi + sh(phi, 0, -1) - sh(phi, -1, 0) - sh(phi, -1, -1)) / (2.0 * dx * msfd)))
    v_pgf.append(-(psd * (phi + sh(phi, -1, 0) - sh(phi, 0, -1) - sh(phi, -1, -1)) / (2.0 * dx * msfd)))
    U.add(u_pgf[1], "pgf")
    V.add(v_pgf[1], "pgf")
    np.seterr(**old_err)

    # ---- the sums: aten(pc_total) is zero when boundary runs, so the sponge leaves (1 - wgt) bt
    # there and the dynamic sum is added to it (:285-294, 404-411)
    zero = np.zeros_like(t1)
    res = dict(T=T, Q=Q, C=Cq, U=U, V=V, coeff=co, tab=tab, pten0=pten0, p_bdy=pinc, qdot=qdot,
               t_bdy=t_bdy, q_bdy=q_bdy, u_bdy=u_bdy, v_bdy=v_bdy, t_dif=t_dif, q_dif=q_dif, c_dif=c_dif,
               u_dif=u_dif, v_dif=v_dif, u_pgf=u_pgf, v_pgf=v_pgf, phi=phi, PTEN=ptot)
    sp = {}
    for name, S, bt, dot in (("TTEN", T, "XTB_BT", False), ("QVTEN", Q, "XQB_BT", False), ("QCTEN", Cq, None, False),
                             ("UTEN", U, "XUB_BT", True), ("VTEN", V, "XVB_BT", True)):
        base = sponge(rc, zero, g[bt], dot, tab) if (sponging and bt) else zero
        sp[name] = base
        res[name] = base + S.v
    res["sponge"] = sp
    return res


def hydro_stages(rc, g, dt0, xbc):
    """The running sums of the hydrostatic t and qv tendencies after each stage (what the budget
    terms are the differences of): t after hadvt (s1), vadv3d ind 1 (s2), the omega term (s3), the
    relaxation (s4), the diffusion (s5); qv after hadvqv (q1), vadvqv (q2), the relaxation (q4),
    the diffusion (q5)."""
    r = hydro_tend(rc, g, dt0, xbc)
    t, q = r["T"].at, r["Q"].at
    return dict(s1=t["adh"], s2=t["adv"], s3=t["adi"], s4=t["bdy"], s5=t["dif"],
                q1=q["adh"], q2=q["adv"], q4=q["bdy"], q5=q["dif"])
