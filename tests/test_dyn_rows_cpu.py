"""The oracle against tests/dyn_ref.py, the NumPy statement of the reference's diffusion and
boundary-relaxation rows written from the Fortran text: hydrostatic calc_coeff, diffu_d and diffu_x
(ring rows, corners), nudge3d / nudge4d3d / nudgeuv / nudge2d under iboudy 5 and 1, the iboudy 4
sponges, and the assembled hydrostatic totals.  One tend from the state after the initial bdyval.

Grids: C1 cut to 37 x 29 (nspgx = nspgd = 7: two 32-wide block columns with the second partial,
four 8-row block rows with the last partial) and to 34 x 23 with the same band depth (the last cross
column alone in its block, the two sides' nspgx-deep zones 9 rows apart with 8 rows between).  Variants:
default (iboudy 5, idiffu 1), iboudy 1, iboudy 4, idiffu 2, diffu_hgtf 0, and the default at kz 14 and 41.

Tolerances.
 - XKC and PTEN (with its nudge2d / sponge2d term): bit for bit.  No transcendental but the exp of
   the iboudy 5 table, which both sides take from the C library; sqrt is correctly rounded.
 - A diffusion or relaxation term is read from the oracle as the difference of two runs' totals, the
   process on and off, both runs starting from identical state (asserted).  The restatement's term is
   exact; the difference carries one rounding of size <= 2**-53 * (a partial sum) per addition that
   forms or follows the term in either run, and one for the difference itself.  With n such
   additions the bound is (n + 1) * 2**-52 * (B + |term|), B the largest |partial sum| the
   restatement forms at the point (the totals included).  n, counted from the text:
     t, qv, qc diffusion   5   the line adds (2 at a corner), the sum with aten(pc_total) in each
                               run (2), the difference (1)
     t, qv relaxation      5   xf fls0 and xg (...) (2; qv 1), the sums (2), the difference (1)
     u, v diffusion        9   the line adds (2), the two pressure-gradient adds in each run (4),
                               the sums (2), the difference (1)
     u, v relaxation       9   xf fls0 and xg (...) (2), the pressure-gradient adds (4), the sums
                               (2), the difference (1)
   For u and v, B is the pressure-gradient partial sums, which largely cancel in the total.
 - Totals: rtol 1e-10, atol 1e-11 * max|want| (the tolerance of the existing restatements: libm
   pow / log), at every point of jci x ici (t, qv, qc) and jdi x idi (u, v), the band included.

ipgf = 1 ({"ipgf": 1} alone and with iboudy 1): PHI at every cross point of jce x ice and UTEN, VTEN at
every point of jdi x idi at the totals' tolerance.  Not vacuous: the restatement with either of its
two ipgf branches put back to the ipgf = 0 form misses UTEN / VTEN by more than 1000 x that tolerance
at more than half of the points, and the ipgf = 0 PHI differs from the ipgf = 1 PHI by more than 1000 x
the tolerance at every cross point.

idiffu = 3: XKC bit for bit; the diffusion of t, qv, qc, u, v as the difference from a run of idiffu = 1
with ckh = adyndif = 0 (xkc = 0) from identical state, with the counts above (the scheme makes one add
per point, so they are upper bounds).  The support is the single column jci2 / jdi2, asserted non-zero
at every row and zero off it.  From the restatement alone: each of the four fluxes is zeroed by its
limiter at 1 % or more of the column's points and kept at 1 % or more, and the rows i <= 3 and
i >= iy - 3, where the i-clamp acts, are compared and non-zero.

Each term check asserts that it is not vacuous: the oracle's term is non-zero (at some level) at
every ring point and corner (diffusion) or band point (relaxation) and zero off its support, and
the median of |term| / bound over the support is at least 2**20, so a relative error of 1e-6 in a
term cannot hide.  Nothing is cropped but the frame edge where p* is zero.
"""
import dataclasses
import functools

import numpy as np
import pytest

from tests import dyn_ref as dr
from tests.support import case, oracle, variant_id

GRIDS = {"37x29": {}, "34x23": dict(jx=34, iy=23, nspgx=7, nspgd=7)}
LEVELS = [{"kz": 14}, {"kz": 41}]          # the sigma tables beside C1's 18 levels (23 is C2's to C4's)
VARIANTS = [{}, {"iboudy": 1}, {"iboudy": 4}, {"idiffu": 2}, {"diffu_hgtf": 0}] + LEVELS
NO_DIF = dict(ckh=0.0, adyndif=0.0)
TOTALS = (("TTEN", "T", False), ("QVTEN", "Q", False), ("QCTEN", "C", False), ("UTEN", "U", True), ("VTEN", "V", True))
N_ADD = {("T", "dif"): 5, ("Q", "dif"): 5, ("C", "dif"): 5, ("U", "dif"): 9, ("V", "dif"): 9,
         ("T", "bdy"): 5, ("Q", "bdy"): 5, ("U", "bdy"): 9, ("V", "bdy"): 9}
EPS = 2.0 ** -52

grid_variant = pytest.mark.parametrize("grid,variant", [(g, v) for g in GRIDS for v in VARIANTS],
                                       ids=lambda p: p if isinstance(p, str) else variant_id(p))


def prepared(rc, state, patch=True):
    """The generated state with what the checks need and it lacks: a cloud layer (qc = 1 % of qv on
    levels 4..12), so that the qc rows are not identically zero, and (patch) a 4 x 4 patch of the
    b-level wind faster by 100 m/s (off the band on both grids), so that the deformation around it
    drives xkc onto the xkhmax clamp: dydc * duv = 2400 m * 200 m/s against xkhmax = 375000 m2/s."""
    st = dict(state)
    for a1, a2 in (("ATM1_QC", "ATM1_QV"), ("ATM2_QC", "ATM2_QV")):
        qc = np.zeros_like(st[a2])
        qc[3:12] = 0.01 * st[a2][3:12]
        st[a1] = qc
    for name in ("ATM2_U", "ATM2_V") if patch else ():
        a = st[name].copy()
        a[:, 9:13, 11:15] += 100.0 * dr.psc2psd(st["PSB"][0])[9:13, 11:15]
        st[name] = a
    return st


def start(grid, variant):
    rc, data, st = case("C", **GRIDS[grid], **variant)
    return rc, data, prepared(rc, st)


@functools.lru_cache(maxsize=None)
def _oracle_run(grid, vkey, okey):
    """One oracle tend of the variant with the options okey on top: the state after bdyval, the
    time, and what tend leaves."""
    rc, data, st = start(grid, dict(vkey))
    rcv = dataclasses.replace(rc, **dict(okey))
    o = oracle(rcv, data, st)
    g = {n: o.get(n) for n in dr.HYDRO_INPUTS}
    _, dt0, xbc = o.get_time()
    o.tend()
    out = {n: o.get(n) for n in ("TTEN", "QVTEN", "QCTEN", "UTEN", "VTEN", "XKC", "PTEN", "PHI", "QDOT")}
    o.close()
    return rcv, g, (dt0, xbc), out


def oracle_run(grid, variant, **opts):
    return _oracle_run(grid, tuple(sorted(variant.items())), tuple(sorted(opts.items())))


@functools.lru_cache(maxsize=None)
def _restated(grid, vkey, diffuse):
    rc, g, (dt0, xbc), _ = _oracle_run(grid, vkey, ())
    return dr.hydro_tend(rc, g, dt0, xbc, diffuse=diffuse)


def restated(grid, variant, diffuse=True):
    return _restated(grid, tuple(sorted(variant.items())), diffuse)


def same_state(a, b):
    for n in dr.HYDRO_INPUTS:
        assert np.array_equal(a[n], b[n]), f"{n} differs after bdyval: the difference is not the term"


def sponge_support(rc, tab, dot):
    """The band points the iboudy 4 sponge changes: wgt = 1 from ibnd 5 (cross) / 6 (dot) on, and
    there (1 - wgt) bt is exactly zero."""
    m = np.zeros((rc.iy, rc.jx), dtype=bool)
    wgt = tab["wgtd" if dot else "wgtx"]
    for (j, i), ib in dr.band(rc, dot).items():
        m[i - 1, j - 1] = wgt[ib] < 1.0
    return m


def check_term(tag, got, incs, big, n, support, everywhere):
    """got: the term as the oracle (or the engine) gives it; incs: the restatement's increments;
    big: the largest |partial sum|; support [i, j]: where the term must be non-zero at some level;
    everywhere [i, j]: the points compared (the term is zero on everywhere & ~support)."""
    want = dr.total(incs)
    bound = (n + 1) * EPS * (big + np.abs(want))
    err = np.abs(got - want)
    m3 = np.broadcast_to(everywhere, want.shape)
    with np.errstate(divide="ignore", invalid="ignore"):         # 0 / 0: a level the term does not touch
        ratio = float(np.where(err[m3] == 0.0, 0.0, err[m3] / bound[m3]).max())
    live = np.broadcast_to(support, want.shape) & (want != 0.0)
    strength = float(np.median(np.abs(want[live]) / bound[live]))
    print(f"{tag}: worst |err| / bound = {ratio:.3f}, median |term| / bound = 2**{np.log2(strength):.1f}, "
          f"max|term| = {np.abs(want[m3]).max():.3e}")
    assert (np.abs(got[:, support]).max(axis=0) > 0.0).all(), f"{tag}: zero at a point of its support"
    assert not got[:, everywhere & ~support].any(), f"{tag}: non-zero off its support"
    assert strength >= 2.0 ** 20, (tag, strength)
    assert ratio <= 1.0, (tag, ratio)
    return ratio


# ------------------------------------------------------------------------------ the band and the tables
def test_band_maps_and_tables():
    """The cross and the dot band differ (nspgd, icx = icy = 0), each side nsp - 2 lines deep, ibnd 2 on
    the first interior line; the tables at their defining points."""
    rc, _, _ = case("C")
    cr, dt = dr.band_sides(rc, False), dr.band_sides(rc, True)
    assert len(cr) == 500 and len(dt) == 520
    assert cr[(rc.jx // 2, 2)] == (dr.SOUTH, 2) and cr[(rc.jx // 2, rc.iy - 2)] == (dr.NORTH, 2)
    assert dt[(rc.jx // 2, rc.iy - 1)] == (dr.NORTH, 2) and (rc.jx // 2, rc.iy - 1) not in cr
    assert cr[(2, rc.iy // 2)] == (dr.WEST, 2) and cr[(rc.jx - 2, rc.iy // 2)] == (dr.EAST, 2)
    assert dt[(rc.jx - 1, rc.iy // 2)] == (dr.EAST, 2) and dt[(rc.jx - 2, rc.iy // 2)] == (dr.EAST, 3)
    assert max(ib for _, ib in cr.values()) == rc.nspgx - 1 and (rc.nspgx, rc.nspgx) not in cr
    t = dr.tables(rc)
    assert t["fcx"][2] == t["fnudge"] == 0.1 / rc.dt and t["fcx"][rc.nspgx - 1] == t["fnudge"] * (1.0 / (rc.nspgx - 2))
    assert t["hefc"][2, 0] == t["fnudge"] and t["hegc"][2, rc.kz - 1] == t["gnudge"] == 1.0 / (50.0 * rc.dt)
    assert t["hefc"][3, 0] > t["hefc"][3, rc.kz - 1]             # high_nudge decays slower than low_nudge
    assert list(t["wgtx"][2:6]) == [0.4, 0.7, 0.9, 1.0] and list(t["wgtd"][2:7]) == [0.20, 0.55, 0.80, 0.95, 1.0]


def test_the_two_grids_are_the_ones_described():
    """37 x 29: 36 cross columns (32 + 4) and 28 cross rows (3 x 8 + 4).  34 x 23: 33 cross columns (the
    last alone in its 32-wide block) and, with the same band depth, the nspgx-deep zones of rows 1..7
    and 16..22: 9 apart, with 8 rows between them."""
    a, _, _ = start("37x29", {})
    b, _, _ = start("34x23", {})
    assert (a.jx - 1, a.iy - 1, a.nspgx, a.nspgd) == (36, 28, 7, 7)
    assert (b.jx - 1, b.iy - 1, b.nspgx, b.nspgd) == (33, 22, 7, 7)
    rows = sorted({i for (_, i) in dr.band(b)})
    assert rows[:5] == [2, 3, 4, 5, 6] and rows[-5:] == [17, 18, 19, 20, 21]     # ibnd 2..6 on either side
    free = [i for i in range(2, b.iy - 1) if not any((j, i) in dr.band(b) for j in (b.nspgx, b.jx - b.nspgx))]
    # the nspgx-deep zones are rows 1..7 and 16..22 (8 rows between); ibnd stops at nspgx - 1, so the
    # rows without a south / north band point are 7..16
    assert free == list(range(7, 17))


# ------------------------------------------------------------------------------ XKC and PTEN, bit for bit
@grid_variant
def test_xkc_and_pten_bit_for_bit(grid, variant):
    rc, g, _, out = oracle_run(grid, variant)
    r = restated(grid, variant)
    co = r["coeff"]
    iy, jx = rc.iy, rc.jx
    dx = rc.ds * 1000.0
    xkhmax = dx * dx / (64.0 * rc.dt)
    raw = co["xkc_raw"][:, :iy - 1, :jx - 1]
    clamped = raw == xkhmax
    print(f"xkc: {clamped.mean():.3f} of the points on the xkhmax clamp")
    assert clamped.any() and not clamped.all()                   # the clamp acts, and not everywhere
    m = dr.domain_mask(rc)
    assert (co["xkc"][:, m] > 0.0).all()
    assert np.array_equal(out["XKC"][:, m], co["xkc"][:, m])
    # the frame lines keep the unscaled coefficient (the scaling loop runs over jci x ici only)
    edge = np.zeros_like(m)
    edge[:iy - 1, :jx - 1] = True
    edge &= ~m
    assert np.array_equal(out["XKC"][:, edge], co["xkc_raw"][:, edge])
    assert not out["XKC"][:, iy - 1, :].any() and not out["XKC"][:, :, jx - 1].any()
    # pten on jce x ice with the boundary term on the band
    band = dr.band_mask(rc)
    term = r["PTEN"] - r["pten0"]
    if rc.iboudy == 4:                                           # wgtx = 1 from ibnd 5 on: no change there
        band = sponge_support(rc, r["tab"], False)
    assert (term[band] != 0.0).all() and not term[~band].any()
    assert np.array_equal(out["PTEN"][0], r["PTEN"])


# ------------------------------------------------------------------------------ the terms
@grid_variant
def test_diffusion_terms(grid, variant):
    rc, g1, _, full = oracle_run(grid, variant)
    _, g0, _, nodif = oracle_run(grid, variant, **NO_DIF)
    same_state(g1, g0)
    r = restated(grid, variant)
    for name, key, dot in TOTALS:
        dom = dr.domain_mask(rc, dot)
        ring, corners = dr.ring_masks(rc, dot)
        S = r[key]
        big = np.fmax(S.big, np.abs(r[name]))
        got = full[name] - nodif[name]
        assert (np.abs(got[:, corners]).max(axis=0) > 0.0).all(), name
        assert (np.abs(got[:, ring]).max(axis=0) > 0.0).all(), name
        check_term(f"{grid} {variant_id(variant)} {name} diffusion", got, r[key.lower() + "_dif"], big,
                   N_ADD[(key, "dif")], dom, dom)


@grid_variant
def test_relaxation_terms(grid, variant):
    """iboudy 5 and 1 against iboudy 2 (no relaxation); the iboudy 4 sponge against iboudy 3, which
    shares its inflow / outflow treatment and relaxes nothing.  Diffusion off in both runs."""
    rc, g1, _, on = oracle_run(grid, variant, **NO_DIF)
    _, g0, _, off = oracle_run(grid, variant, iboudy=3 if rc.iboudy == 4 else 2, **NO_DIF)
    same_state(g1, g0)
    r = restated(grid, variant, diffuse=False)
    for name, key, dot in TOTALS:
        if key == "C":
            assert np.array_equal(on[name], off[name])           # qc is not relaxed
            continue
        dom, band = dr.domain_mask(rc, dot), dr.band_mask(rc, dot)
        S = r[key]
        big = np.fmax(S.big, np.abs(r[name]))
        incs = [r["sponge"][name]] if rc.iboudy == 4 else r[key.lower() + "_bdy"]
        got = on[name] - off[name]
        if rc.iboudy == 4:
            band = sponge_support(rc, r["tab"], dot)
        check_term(f"{grid} {variant_id(variant)} {name} relaxation", got, incs, big, N_ADD[(key, "bdy")], band, dom)


# ------------------------------------------------------------------------------ the totals
@grid_variant
def test_totals(grid, variant):
    rc, _, _, out = oracle_run(grid, variant)
    r = restated(grid, variant)
    for name, _, dot in TOTALS:
        m = dr.domain_mask(rc, dot)
        got, want = out[name][:, m], r[name][:, m]
        assert np.abs(want).max() > 0.0, name
        tol = 1e-10 * np.abs(want) + 1e-11 * np.abs(want).max()
        print(f"{grid} {variant_id(variant)} {name}: worst |err| / tolerance = {(np.abs(got - want) / tol).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg=name)


# ------------------------------------------------------------------------------ ipgf = 1
PGF_VARIANTS = [{"ipgf": 1}, {"ipgf": 1, "iboudy": 1}]
MUTANT_FACTOR = 1000.0


def totals_tol(want):
    """The totals' tolerance (libm pow / log rows) as an array: rtol 1e-10, atol 1e-11 * max|want|."""
    return 1e-10 * np.abs(want) + 1e-11 * np.abs(want).max()


def check_ipgf1(tag, rc, g, times, out, tiles=None):
    """out (the oracle's or the engine's PHI, UTEN, VTEN of one tend from g) against the restated
    ipgf = 1 branches, with the non-vacuity asserts."""
    assert rc.ipgf == 1
    r = dr.hydro_tend(rc, g, *times, tiles=tiles)
    r0 = dr.hydro_tend(dataclasses.replace(rc, ipgf=0), g, *times, tiles=tiles)
    iy, jx = rc.iy, rc.jx
    want, got, want0 = (a[:, :iy - 1, :jx - 1] for a in (r["phi"], out["PHI"], r0["phi"]))
    tol = totals_tol(want)
    print(f"{tag} PHI: worst |err| / tolerance = {(np.abs(got - want) / tol).max():.3e}, "
          f"least |ipgf 0 - ipgf 1| / tolerance = {(np.abs(want0 - want) / tol).min():.3e}")
    assert (np.abs(want0 - want) > MUTANT_FACTOR * tol).all()
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg="PHI")
    m = dr.domain_mask(rc, True)
    mutants = {rv: dr.hydro_tend(rc, g, *times, revert=rv, tiles=tiles) for rv in ("rtbar", "phi")}
    for name in ("UTEN", "VTEN"):
        want, got = r[name][:, m], out[name][:, m]
        tol = totals_tol(want)
        miss = {rv: float((np.abs(got - mu[name][:, m]) > MUTANT_FACTOR * tol).mean()) for rv, mu in mutants.items()}
        print(f"{tag} {name}: worst |err| / tolerance = {(np.abs(got - want) / tol).max():.3e}; the points a "
              f"reverted branch misses by > {MUTANT_FACTOR:g} x tolerance: {miss}")
        for rv, frac in miss.items():
            assert frac > 0.5, (name, rv, frac)
        for i, pg in enumerate(r[name[0].lower() + "_pgf"]):     # each increment carries weight of its own
            assert (np.abs(pg[:, m]) > MUTANT_FACTOR * tol).mean() > 0.5, (name, i)
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg=name)


@pytest.mark.parametrize("grid,variant", [(g, v) for g in GRIDS for v in PGF_VARIANTS],
                         ids=lambda p: p if isinstance(p, str) else variant_id(p))
def test_ipgf1_phi_and_winds(grid, variant):
    rc, g, times, out = oracle_run(grid, variant)
    check_ipgf1(f"{grid} {variant_id(variant)}", rc, g, times, out)


# ------------------------------------------------------------------------------ idiffu = 3
D6 = {"idiffu": 3}
D6_OFF = dict(idiffu=1, **NO_DIF)


def column_mask(rc, dot, tiles=None):
    """[i, j] of the points the idiffu = 3 term is added at."""
    m = np.zeros((rc.iy, rc.jx), dtype=bool)
    for j, i1, i2 in dr.tile_columns(rc, dot, tiles):
        m[i1 - 1:i2, j - 1] = True
    return m


def check_diffu6_edges(tag, rc, g, r, tiles=None):
    """From the restatement alone: the limiter zeroes and keeps each flux of each field at 1 % or more
    of the column's points, and the rows where the i-clamp acts are on the columns and non-zero."""
    ub, vb, tb, qvb, qcb, _ = dr.b_slices(g)
    msfd = g["MSFD"][0]
    with np.errstate(divide="ignore", invalid="ignore"):
        fields = (("t", tb, tb / msfd, False), ("qv", qvb, qvb / msfd, False), ("qc", qcb, qcb / msfd, False),
                  ("u", ub / msfd, ub / msfd, True), ("v", vb / msfd, vb / msfd, True))
        for name, fv, lv, dot in fields:
            fl, mask = dr.fluxes6(rc, fv, lv, dr.tile_columns(rc, dot, tiles), dot)
            assert np.array_equal(mask, column_mask(rc, dot, tiles))
            for fx, (raw, lim) in fl.items():
                live = raw[:, mask] != 0.0                       # (qc is zero off its cloud layer)
                zeroed = float(((lim[:, mask] == 0.0) & live).sum() / live.sum())
                print(f"{tag} {name} {fx}: zeroed by the limiter at {zeroed:.3f} of the column's points")
                assert 0.01 <= zeroed <= 0.99, (name, fx, zeroed)
            want = dr.total(r[{"t": "t", "qv": "q", "qc": "c", "u": "u", "v": "v"}[name] + "_dif"])
            ihi = rc.iy - 1 if dot else rc.iy - 2                # idi2 / ici2
            rows = [i for i in range(2, ihi + 1) if i <= 3 or i >= rc.iy - 3]
            assert len(rows) == (5 if dot else 4)
            for i in rows:
                assert mask[i - 1].any(), (name, i)
                assert (np.abs(want[:, i - 1, :]).max(axis=0)[mask[i - 1]] > 0.0).all(), (name, i)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_idiffu3_xkc_and_terms(grid):
    rc, g1, times, full = oracle_run(grid, D6)
    _, g0, _, off = oracle_run(grid, D6, **D6_OFF)
    same_state(g1, g0)
    r = dr.hydro_tend(rc, g1, *times)
    m = dr.domain_mask(rc)
    coef = 0.12 * 0.015625 / (2.0 * rc.dt)
    assert np.array_equal(r["coeff"]["xkc"][:, m], np.broadcast_to(coef * g1["PSB"][0][m], (rc.kz, m.sum())))
    assert np.array_equal(full["XKC"][:, m], r["coeff"]["xkc"][:, m])
    assert not off["XKC"].any()
    check_diffu6_edges(f"{grid} idiffu=3", rc, g1, r)
    for name, key, dot in TOTALS:
        dom, col = dr.domain_mask(rc, dot), column_mask(rc, dot)
        assert col.sum() == (rc.iy - 2 if dot else rc.iy - 3) and (col & dom).sum() == col.sum()
        big = np.fmax(r[key].big, np.abs(r[name]))
        check_term(f"{grid} idiffu=3 {name} diffusion", full[name] - off[name], r[key.lower() + "_dif"], big,
                   N_ADD[(key, "dif")], col, dom)
    for name, _, dot in TOTALS:                                  # and the assembled totals
        md = dr.domain_mask(rc, dot)
        np.testing.assert_allclose(full[name][:, md], r[name][:, md], rtol=1e-10,
                                   atol=1e-11 * np.abs(r[name][:, md]).max(), err_msg=name)
