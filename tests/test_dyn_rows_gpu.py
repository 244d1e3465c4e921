"""The engine against tests/dyn_ref.py, the NumPy statement of the reference's diffusion and
boundary-relaxation rows written from the Fortran text.  No oracle is involved.  Through the C-ABI
with rcmdyn_set_diagnostics and the tendency budget on at rw = 1: one tend from the state after the
initial bdyval (tests/test_dyn_rows_cpu.py's prepared state: a cloud layer, and a wind patch that
drives xkc onto its clamp).

Grids: C1 cut to 37 x 29 and to 34 x 23 (nspgx = nspgd = 7 on both), the 37 x 29 grid as 2 x 2
tiles (the second-order rows belong to the domain edge: an interior tile boundary takes the
fourth-order form), and N1 cut to 37 x 29 for the non-hydrostatic budget terms.

Tolerances.
 - XKC and PTEN: bit for bit (iboudy 5, 1, 4; diffu_hgtf 0, 1; kz 14 and 41 beside C1's 18, on both
   grids and as 2 x 2 tiles).
 - T_DIF, Q_DIF, T_BDY, Q_BDY against the restatement's terms: a budget term is the rounded
   difference of the running sum around the process, and the running sum takes one rounded addition
   per increment: n = 3 (two line adds at a corner, or xf fls0 and xg (...); the difference), bound
   (n + 1) * 2**-52 * (B + |term|).  Hydrostatic core: B is the largest |partial sum| the
   restatement forms at the point.  Non-hydrostatic core: the restatement does not hold the NH
   advection chain, so B is the sum of the |budget terms| at the point, which bounds every partial
   sum of theirs by the triangle inequality.
 - The diffusion and relaxation of u and v as engine on / off differences of UTEN and VTEN from
   identical state (asserted), n = 9 as derived in tests/test_dyn_rows_cpu.py.
 - Totals (TTEN, QVTEN, QCTEN, UTEN, VTEN; under iboudy 4 they hold the sponge): rtol 1e-10, atol
   1e-11 * max|want|, at every interior point, the band included.

ipgf = 1 (alone and with iboudy 1, both grids, 2 x 2 tiles on 37 x 29): PHI (the engine's read-only
diagnostic) at every cross point and UTEN, VTEN at every point of jdi x idi at the totals' tolerance,
with the reverted-branch asserts of tests/test_dyn_rows_cpu.py.

idiffu = 3 (both grids, 2 x 2 tiles on 37 x 29, where the term sits on each tile's last interior column
and the interior tile's clamp does not act; the tile bounds are read from the host-side decomposition):
XKC bit for bit; T_DIF and Q_DIF through the budget (n = 3); the diffusion of u, v and qc as the
difference from idiffu = 1 with ckh = adyndif = 0 from identical state (n = 9, 9, 5); T_DIF / Q_DIF of the
non-hydrostatic core on N1 cut to 37 x 29; the limiter and clamp-row asserts from the restatement.

The same non-vacuity asserts as on the CPU: each term non-zero on all of its support and zero off
it, median |term| / bound >= 2**20.
"""
import dataclasses
import functools

import numpy as np
import pytest

from regcm_amd.dycore import BUDGET_TERMS, tile_extent
from tests import dyn_ref as dr
from tests import support
from tests.support import case, variant_id
from tests.test_dyn_rows_cpu import (D6, D6_OFF, GRIDS, LEVELS, N_ADD, NO_DIF, PGF_VARIANTS, TOTALS, check_diffu6_edges,
                                     check_ipgf1, check_term, column_mask, prepared, same_state, sponge_support, start)

pytestmark = pytest.mark.gpu

ONE = (1, 1)
CASES = ([(g, v, ONE) for g in GRIDS for v in ({}, {"iboudy": 1}, {"iboudy": 4}, {"idiffu": 2}, {"diffu_hgtf": 0})] +
         [("37x29", v, (2, 2)) for v in ({}, {"iboudy": 4}, {"idiffu": 2})] +
         [(g, v, ONE) for g in GRIDS for v in LEVELS] + [("37x29", v, (2, 2)) for v in LEVELS])
N_BUDGET = 3
NH_INPUTS = ("ATM2_U", "ATM2_V", "ATM2_W", "ATM2_T", "ATM2_QV", "ATM2_QC", "PSB", "HT", "XTB_B0", "XTB_BT", "XQB_B0",
             "XQB_BT")


def _cid(p):
    return p if isinstance(p, str) else "x".join(map(str, p)) if isinstance(p, tuple) else variant_id(p)


cases = pytest.mark.parametrize("grid,variant,nproc", CASES, ids=_cid)


def _tend(rc, data, st, nproc, inputs):
    e = support.engine(rc, data, st, nproc, bdyval=False)
    e.set_diagnostics(True)
    e.set_budget(True, rw=1.0)
    e.bdyval()
    g = {n: e.get(n) for n in inputs}
    _, dt0, xbc = e.get_time()
    e.tend()
    out = {n: e.get(n) for n in ("TTEN", "QVTEN", "QCTEN", "UTEN", "VTEN", "XKC", "PTEN", "PHI")}
    out.update({n: e.get_budget(n) for n in BUDGET_TERMS})
    e.close()
    return g, (dt0, xbc), out


@functools.lru_cache(maxsize=None)
def _engine_run(grid, vkey, okey, nproc):
    rc, data, st = start(grid, dict(vkey))
    rcv = dataclasses.replace(rc, **dict(okey))
    return (rcv,) + _tend(rcv, data, st, nproc, dr.HYDRO_INPUTS)


def engine_run(grid, variant, nproc, **opts):
    return _engine_run(grid, tuple(sorted(variant.items())), tuple(sorted(opts.items())), nproc)


@functools.lru_cache(maxsize=None)
def _restated(grid, vkey, nproc, diffuse):
    rc, g, (dt0, xbc), _ = _engine_run(grid, vkey, () if diffuse else tuple(sorted(NO_DIF.items())), nproc)
    return dr.hydro_tend(rc, g, dt0, xbc, diffuse=diffuse)


def restated(grid, variant, nproc, diffuse=True):
    return _restated(grid, tuple(sorted(variant.items())), nproc, diffuse)


# ------------------------------------------------------------------------------ XKC and PTEN, bit for bit
@cases
def test_xkc_and_pten_bit_for_bit(grid, variant, nproc):
    rc, _, _, out = engine_run(grid, variant, nproc)
    r = restated(grid, variant, nproc)
    co = r["coeff"]
    iy, jx = rc.iy, rc.jx
    dx = rc.ds * 1000.0
    clamped = co["xkc_raw"][:, :iy - 1, :jx - 1] == dx * dx / (64.0 * rc.dt)
    assert clamped.any() and not clamped.all()
    m = dr.domain_mask(rc)
    assert np.array_equal(out["XKC"][:, m], co["xkc"][:, m])
    band = sponge_support(rc, r["tab"], False) if rc.iboudy == 4 else dr.band_mask(rc)
    term = r["PTEN"] - r["pten0"]
    assert (term[band] != 0.0).all() and not term[~band].any()
    assert np.array_equal(out["PTEN"][0][:iy - 1, :jx - 1], r["PTEN"][:iy - 1, :jx - 1])


# ------------------------------------------------------------------------------ the budget terms of t and qv
@cases
def test_budget_terms_match_the_restatement(grid, variant, nproc):
    rc, _, _, out = engine_run(grid, variant, nproc)
    r = restated(grid, variant, nproc)
    dom = dr.domain_mask(rc)
    band = sponge_support(rc, r["tab"], False) if rc.iboudy == 4 else dr.band_mask(rc)
    tag = f"{grid} {_cid(nproc)} {variant_id(variant)}"
    for key, total, dif, bdy in (("T", "TTEN", "T_DIF", "T_BDY"), ("Q", "QVTEN", "Q_DIF", "Q_BDY")):
        big = np.fmax(r[key].big, np.abs(r[total]))
        ring, corners = dr.ring_masks(rc)
        assert (np.abs(out[dif][:, ring]).max(axis=0) > 0.0).all() and (np.abs(out[dif][:, corners]).max(axis=0) > 0.0).all()
        check_term(f"{tag} {dif}", out[dif], r[key.lower() + "_dif"], big, N_BUDGET, dom, dom)
        incs = [r["sponge"][total]] if rc.iboudy == 4 else r[key.lower() + "_bdy"]
        check_term(f"{tag} {bdy}", out[bdy], incs, big, N_BUDGET, band, dom)


# ------------------------------------------------------------------------------ u and v, term by term
@cases
def test_wind_terms_match_the_restatement(grid, variant, nproc):
    """Diffusion: the full run less the run with ckh = adyndif = 0.  Relaxation: that run less the one
    with iboudy 2 as well (iboudy 3 under the iboudy 4 sponge, which shares its inflow / outflow
    treatment)."""
    rc, g1, _, full = engine_run(grid, variant, nproc)
    _, g0, _, nodif = engine_run(grid, variant, nproc, **NO_DIF)
    _, gb, _, nobdy = engine_run(grid, variant, nproc, iboudy=3 if rc.iboudy == 4 else 2, **NO_DIF)
    same_state(g1, g0)
    same_state(g1, gb)
    r, r0 = restated(grid, variant, nproc), restated(grid, variant, nproc, diffuse=False)
    dom = dr.domain_mask(rc, True)
    ring, corners = dr.ring_masks(rc, True)
    band = sponge_support(rc, r["tab"], True) if rc.iboudy == 4 else dr.band_mask(rc, True)
    tag = f"{grid} {_cid(nproc)} {variant_id(variant)}"
    for name, key in (("UTEN", "U"), ("VTEN", "V")):
        got = full[name] - nodif[name]
        assert (np.abs(got[:, ring]).max(axis=0) > 0.0).all() and (np.abs(got[:, corners]).max(axis=0) > 0.0).all()
        check_term(f"{tag} {name} diffusion", got, r[key.lower() + "_dif"], np.fmax(r[key].big, np.abs(r[name])),
                   N_ADD[(key, "dif")], dom, dom)
        incs = [r0["sponge"][name]] if rc.iboudy == 4 else r0[key.lower() + "_bdy"]
        check_term(f"{tag} {name} relaxation", nodif[name] - nobdy[name], incs,
                   np.fmax(r0[key].big, np.abs(r0[name])), N_ADD[(key, "bdy")], band, dom)


# ------------------------------------------------------------------------------ the totals
@cases
def test_totals_match_the_restatement(grid, variant, nproc):
    rc, _, _, out = engine_run(grid, variant, nproc)
    r = restated(grid, variant, nproc)
    for name, _, dot in TOTALS:
        m = dr.domain_mask(rc, dot)
        got, want = out[name][:, m], r[name][:, m]
        assert np.abs(want).max() > 0.0, name
        tol = 1e-10 * np.abs(want) + 1e-11 * np.abs(want).max()
        print(f"{grid} {_cid(nproc)} {variant_id(variant)} {name}: worst |err| / tolerance = "
              f"{(np.abs(got - want) / tol).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg=name)


# ------------------------------------------------------------------------------ the non-hydrostatic budget terms
def test_nh_budget_terms_match_the_restatement():
    """T_DIF / Q_DIF from the NH xkc (the vertical-velocity term, xkhz = ckh dx, twice the xkhmax) and
    T_BDY / Q_BDY at iboudy 5 on N1 cut to 37 x 29."""
    rc, data, st = case("N")
    st = prepared(rc, st, patch=False)           # the 3 km core's sound step is not given a 100 m/s jump
    g, (dt0, xbc), out = _tend(rc, data, st, ONE, NH_INPUTS)
    co = dr.nh_coeff(rc, g)
    dom, band = dr.domain_mask(rc), dr.band_mask(rc)
    ring, corners = dr.ring_masks(rc)
    _, _, tb, qvb, _, _ = dr.b_slices(g)         # (the engine exports no XKC of this core: T_DIF carries it)
    xt = xbc + dt0
    for key, dif, bdy, f, a2, b0, bt, kind in (("T", "T_DIF", "T_BDY", tb, "ATM2_T", "XTB_B0", "XTB_BT", "t"),
                                               ("Q", "Q_DIF", "Q_BDY", qvb, "ATM2_QV", "XQB_B0", "XQB_BT", "qv")):
        big = sum(np.abs(out[n]) for n in BUDGET_TERMS if n.startswith(key + "_"))
        assert (np.abs(out[dif][:, ring]).max(axis=0) > 0.0).all() and (np.abs(out[dif][:, corners]).max(axis=0) > 0.0).all()
        check_term(f"N 37x29 {dif}", out[dif], dr.diffu_x(rc, f, co["xkc"]), big, N_BUDGET, dom, dom)
        check_term(f"N 37x29 {bdy}", out[bdy], dr.nudge(rc, g[a2], g[b0], g[bt], xt, kind), big, N_BUDGET, band, dom)


# ------------------------------------------------------------------------------ ipgf = 1
def tiles_of(rc, nproc):
    """[(ext, bdy)] of the nproc = (tiles in j, tiles in i) decomposition, from the host-side geometry."""
    return [tile_extent(rc.jx, rc.iy, nproc[0], nproc[1], t) for t in range(nproc[0] * nproc[1])]


@pytest.mark.parametrize("grid,variant,nproc", [(g, v, ONE) for g in GRIDS for v in PGF_VARIANTS] +
                         [("37x29", v, (2, 2)) for v in PGF_VARIANTS], ids=_cid)
def test_ipgf1_phi_and_winds(grid, variant, nproc):
    rc, g, times, out = engine_run(grid, variant, nproc)
    check_ipgf1(f"{grid} {_cid(nproc)} {variant_id(variant)}", rc, g, times, out)


# ------------------------------------------------------------------------------ idiffu = 3
@pytest.mark.parametrize("grid,nproc", [(g, ONE) for g in GRIDS] + [("37x29", (2, 2))], ids=_cid)
def test_idiffu3_xkc_and_terms(grid, nproc):
    rc, g1, times, full = engine_run(grid, D6, nproc)
    _, g0, _, off = engine_run(grid, D6, nproc, **D6_OFF)
    same_state(g1, g0)
    tiles = tiles_of(rc, nproc)
    r = dr.hydro_tend(rc, g1, *times, tiles=tiles)
    tag = f"{grid} {_cid(nproc)} idiffu=3"
    m = dr.domain_mask(rc)
    assert np.array_equal(full["XKC"][:, m], r["coeff"]["xkc"][:, m]) and (r["coeff"]["xkc"][:, m] > 0.0).all()
    check_diffu6_edges(tag, rc, g1, r, tiles)
    for dot in (False, True):
        cols = dr.tile_columns(rc, dot, tiles)
        jmax = rc.jx if dot else rc.jx - 1
        assert len({c[0] for c in cols}) == nproc[0] and len(cols) == nproc[0] * nproc[1]
        # every tile column but the last has its three neighbours to the east: the j-clamp does not act
        assert sorted(c[0] + 3 <= jmax for c in cols) == [False] * nproc[1] + [True] * ((nproc[0] - 1) * nproc[1])
    dom, col = dr.domain_mask(rc), column_mask(rc, False, tiles)
    for key, total, dif in (("T", "TTEN", "T_DIF"), ("Q", "QVTEN", "Q_DIF")):
        check_term(f"{tag} {dif}", full[dif], r[key.lower() + "_dif"], np.fmax(r[key].big, np.abs(r[total])), N_BUDGET,
                   col, dom)
    for name, key, dot in TOTALS[2:]:
        check_term(f"{tag} {name} diffusion", full[name] - off[name], r[key.lower() + "_dif"],
                   np.fmax(r[key].big, np.abs(r[name])), N_ADD[(key, "dif")], column_mask(rc, dot, tiles),
                   dr.domain_mask(rc, dot))
    for name, _, dot in TOTALS:
        md = dr.domain_mask(rc, dot)
        np.testing.assert_allclose(full[name][:, md], r[name][:, md], rtol=1e-10,
                                   atol=1e-11 * np.abs(r[name][:, md]).max(), err_msg=name)


def test_nh_idiffu3_budget_terms_match_the_restatement():
    """T_DIF / Q_DIF of the non-hydrostatic core at idiffu = 3 on N1 cut to 37 x 29: the constant
    coefficient diff_6th_coef * p*b and the one column jci2, as test_nh_budget_terms_match_the_restatement
    holds the idiffu = 1 form."""
    rc, data, st = case("N", idiffu=3)
    st = prepared(rc, st, patch=False)
    g, _, out = _tend(rc, data, st, ONE, NH_INPUTS + ("MSFD",))
    co = dr.nh_coeff(rc, g)
    dom, col = dr.domain_mask(rc), column_mask(rc, False)
    _, _, tb, qvb, _, _ = dr.b_slices(g)
    for key, dif, f in (("T", "T_DIF", tb), ("Q", "Q_DIF", qvb)):
        big = sum(np.abs(out[n]) for n in BUDGET_TERMS if n.startswith(key + "_"))
        check_term(f"N 37x29 idiffu=3 {dif}", out[dif], dr.diffu_x(rc, f, co["xkc"], g["MSFD"][0]), big, N_BUDGET, col, dom)
