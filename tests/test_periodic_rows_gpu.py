"""The engine against tests/dyn_ref.py and tests/tke_ref.py on the periodic grids and in the
non-hydrostatic core, with the grids, inputs and checks of tests/test_periodic_rows_cpu.py (see its
docstring).  No oracle is involved.  Through the C-ABI with rcmdyn_set_diagnostics on.

Tilings: one tile on every case; 2 x 1 and 2 x 2 on the 37 x 29 cuts (the default variant; on HB's
term, budget and total tests every variant).  Two tiles in j
make a tile both neighbours of the other around the period, and 37 splits unevenly.

Rows and tolerances.
 - QDOT, then ATM1_TKE and ATM2_TKE after tend and after bdyval over two steps, bit for bit at every
   cross point of the kz + 1 levels, on HB, NL, NB and CRM; XKC and PTEN bit for bit on HB.  The engine
   exports no XKC of the non-hydrostatic core: get("XKC") succeeds there and returns a buffer that the
   non-hydrostatic step never writes, so it is not read here; the TKE diffusion and T_DIF / Q_DIF
   carry the coefficient.
 - T_DIF, Q_DIF, T_BDY, Q_BDY through the budget at rw = 1 on HB, NB and CRM, within (n + 1) * 2**-52 *
   (B + |term|), n = 3, B as tests/test_dyn_rows_gpu.py derives it for each core; on CRM T_BDY and Q_BDY
   are exactly zero.
 - On HB the diffusion and relaxation of u and v as engine on / off differences from identical state
   (n = 9), and the totals TTEN, QVTEN, QCTEN, UTEN, VTEN at rtol 1e-10, atol 1e-11 * max|want|, at every
   point of the band's interior ranges; variants iboudy 5, 1, 4 and idiffu 1, 2.

The non-vacuity asserts are those of the CPU file (supports, term sizes, mutants, boundary lines,
floor), made from the restatement on the engine's own inputs.
"""
import dataclasses
import functools

import numpy as np
import pytest

from regcm_amd.dycore import BUDGET_TERMS, tile_extent
from tests import dyn_ref as dr
from tests import support
from tests import tke_ref as tr
from tests.support import variant_id
from tests.test_dyn_rows_cpu import NO_DIF, check_term, same_state
from tests.test_periodic_rows_cpu import (CASES, GRIDS, HB_GRIDS, HB_VARIANTS, TEND_OUT, check_band_diffusion,
                                          check_band_relaxation, check_band_totals, check_pten, check_rows, check_tke,
                                          relax_support, run, start, wrap_lines)

pytestmark = pytest.mark.gpu

ONE = (1, 1)
TILED = [(g, {}, t) for g in GRIDS if g.endswith("37x29") for t in ((2, 1), (2, 2))]
N_BUDGET = 3
WINDS = (("UTEN", "U", True), ("VTEN", "V", True))
NH_BUDGET_INPUTS = tr.NH_INPUTS + ("ATM2_T", "ATM2_QV", "ATM2_QC", "XTB_B0", "XTB_BT", "XQB_B0", "XQB_BT")


def _cid(p):
    return p if isinstance(p, str) else "x".join(map(str, p)) if isinstance(p, tuple) else variant_id(p)


def _engine(grid, variant, nproc, budget=False, **opts):
    rc, data, st, extra = start(grid, variant)
    rc = dataclasses.replace(rc, **opts)
    e = support.engine(rc, data, st, nproc, bdyval=False, extra=extra)
    e.set_diagnostics(True)
    if budget:
        e.set_budget(True, rw=1.0)
    e.bdyval()
    return rc, e


def tiles_of(rc, nproc):
    return [tile_extent(rc.jx, rc.iy, nproc[0], nproc[1], t, rc.i_band, rc.i_crm) for t in range(nproc[0] * nproc[1])]


# ------------------------------------------------------------------------------ QDOT, XKC and the TKE, bit for bit
@functools.lru_cache(maxsize=None)
def _two_steps(grid, vkey, nproc):
    rc, e = _engine(grid, dict(vkey), nproc)
    return rc, run(e, rc)


@pytest.mark.parametrize("grid,variant,nproc", [(g, v, ONE) for g, v in CASES] + TILED, ids=_cid)
def test_xkc_qdot_and_tke_bit_for_bit(grid, variant, nproc):
    rc, steps = _two_steps(grid, tuple(sorted(variant.items())), nproc)
    tag = f"{grid} {_cid(nproc)} {variant_id(variant)}"
    check_rows(tag, rc, steps[0], xkc=rc.idynamic == 1)
    for n, step in enumerate(steps):
        check_tke(f"{tag} step {n + 1}", rc, step, n == 0, tiles=tiles_of(rc, nproc))


# ------------------------------------------------------------------------------ one tend with the budget
@functools.lru_cache(maxsize=None)
def _one_tend(grid, vkey, okey, nproc):
    rc, e = _engine(grid, dict(vkey), nproc, budget=True, **dict(okey))
    g = {n: e.get(n) for n in (dr.HYDRO_INPUTS if rc.idynamic == 1 else NH_BUDGET_INPUTS)}
    _, dt0, xbc = e.get_time()
    e.tend()
    out = {n: e.get(n) for n in (TEND_OUT if rc.idynamic == 1 else ())}
    out.update({n: e.get_budget(n) for n in BUDGET_TERMS})
    e.close()
    return rc, g, (dt0, xbc), out


def one_tend(grid, variant, nproc, **opts):
    return _one_tend(grid, tuple(sorted(variant.items())), tuple(sorted(opts.items())), nproc)


@functools.lru_cache(maxsize=None)
def _restated(grid, vkey, nproc, diffuse):
    rc, g, times, _ = _one_tend(grid, vkey, () if diffuse else tuple(sorted(NO_DIF.items())), nproc)
    return dr.hydro_tend(rc, g, *times, diffuse=diffuse)


def restated(grid, variant, nproc, diffuse=True):
    return _restated(grid, tuple(sorted(variant.items())), nproc, diffuse)


hb_cases = pytest.mark.parametrize("grid,variant,nproc", [(g, v, ONE) for g in HB_GRIDS for v in HB_VARIANTS] +
                                   [("HB-37x29", v, t) for v in HB_VARIANTS for t in ((2, 1), (2, 2))], ids=_cid)


@hb_cases
def test_band_pten_and_budget_terms(grid, variant, nproc):
    rc, g, times, out = one_tend(grid, variant, nproc)
    tag = f"{grid} {_cid(nproc)} {variant_id(variant)}"
    check_pten(tag, rc, g, times, out["PTEN"])
    r = restated(grid, variant, nproc)
    dom = dr.domain_mask(rc)
    ring, corners = dr.ring_masks(rc)
    band = relax_support(rc, r, False)
    assert ring.sum() == 2 * rc.jx and not corners.any() and band[:, 0].any() and band[:, rc.jx - 1].any()
    for key, total, dif, bdy in (("T", "TTEN", "T_DIF", "T_BDY"), ("Q", "QVTEN", "Q_DIF", "Q_BDY")):
        big = np.fmax(r[key].big, np.abs(r[total]))
        assert (np.abs(out[dif][:, ring]).max(axis=0) > 0.0).all()
        check_term(f"{tag} {dif}", out[dif], r[key.lower() + "_dif"], big, N_BUDGET, dom, dom)
        incs = [r["sponge"][total]] if rc.iboudy == 4 else r[key.lower() + "_bdy"]
        check_term(f"{tag} {bdy}", out[bdy], incs, big, N_BUDGET, band, dom)


@hb_cases
def test_band_wind_terms(grid, variant, nproc):
    """Diffusion: the full run less the run with ckh = adyndif = 0.  Relaxation: that run less the one
    with iboudy 2 as well (iboudy 3 under the iboudy 4 sponge)."""
    rc, g1, _, full = one_tend(grid, variant, nproc)
    _, g0, _, nodif = one_tend(grid, variant, nproc, **NO_DIF)
    _, gb, _, nobdy = one_tend(grid, variant, nproc, iboudy=3 if rc.iboudy == 4 else 2, **NO_DIF)
    same_state(g1, g0)
    same_state(g1, gb)
    tag = f"{grid} {_cid(nproc)} {variant_id(variant)}"
    check_band_diffusion(tag, rc, restated(grid, variant, nproc), full, nodif, fields=WINDS)
    check_band_relaxation(tag, rc, restated(grid, variant, nproc, diffuse=False), nodif, nobdy, fields=WINDS)


@hb_cases
def test_band_totals(grid, variant, nproc):
    rc, g, times, out = one_tend(grid, variant, nproc)
    check_band_totals(f"{grid} {_cid(nproc)} {variant_id(variant)}", rc, restated(grid, variant, nproc), out, g, times)


# ------------------------------------------------------------------------------ the non-hydrostatic budget terms
NH_GRIDS = [g for g in GRIDS if g[:2] in ("NB", "CR")]


@pytest.mark.parametrize("grid,variant,nproc", [(g, v, ONE) for g in NH_GRIDS for v in ({}, {"idiffu": 2})] +
                         [(g, {}, t) for g in NH_GRIDS if g.endswith("37x29") for t in ((2, 1), (2, 2))], ids=_cid)
def test_nh_budget_terms(grid, variant, nproc):
    """T_DIF / Q_DIF from the NH xkc of the periodic ranges and T_BDY / Q_BDY: on NB the south and north
    rows at every j, on CRM exactly zero.  B is the sum of the |budget terms| at the point
    (tests/test_dyn_rows_gpu.py)."""
    rc, g, (dt0, xbc), out = one_tend(grid, variant, nproc)
    tag = f"{grid} {_cid(nproc)} {variant_id(variant)}"
    G = dr.geom(rc)
    co = dr.nh_coeff(rc, g)
    dom, band = dr.domain_mask(rc), dr.band_mask(rc)
    ring, _ = dr.ring_masks(rc)
    assert dom[:, 0].any() and dom[:, rc.jx - 1].any() and (dom.all() if G.peri else ring.sum() == 2 * rc.jx)
    _, _, tb, qvb, _, _ = dr.b_slices(g, G)
    xt = xbc + dt0
    for key, dif, bdy, f, a2, b0, bt, kind in (("T", "T_DIF", "T_BDY", tb, "ATM2_T", "XTB_B0", "XTB_BT", "t"),
                                               ("Q", "Q_DIF", "Q_BDY", qvb, "ATM2_QV", "XQB_B0", "XQB_BT", "qv")):
        big = sum(np.abs(out[n]) for n in BUDGET_TERMS if n.startswith(key + "_"))
        assert (np.abs(out[dif][:, ring]).max(axis=0) > 0.0).all()
        want = dr.diffu_x(rc, f, co["xkc"])
        check_term(f"{tag} {dif}", out[dif], want, big, N_BUDGET, dom, dom)
        # mutant (a), from the restatement: the zero pad for the wrap misses the term by more than 1000 x
        # its bound at every value of the lines next to the wrap
        with dr.zero_pad_for_the_wrap():
            mu = dr.total(dr.diffu_x(rc, f, dr.nh_coeff(rc, g)["xkc"]))
        w = wrap_lines(rc)
        bound = (N_BUDGET + 1) * 2.0 ** -52 * (big + np.abs(dr.total(want)))
        with np.errstate(divide="ignore", invalid="ignore"):     # the unused row of a band: 0 / 0, off the lines
            ratio = (np.abs(mu - dr.total(want)) / bound)[:, w]
        print(f"{tag} {dif} with the zero pad for the wrap: least miss {ratio.min():.3e} x bound")
        assert ratio.min() > 1000.0, (dif, float(ratio.min()))
        if G.peri:
            assert not band.any() and not out[bdy].any(), bdy
        else:
            assert band[:, 0].any() and band[:, rc.jx - 1].any() and (band.sum(axis=1) % rc.jx == 0).all()
            check_term(f"{tag} {bdy}", out[bdy], dr.nudge(rc, g[a2], g[b0], g[bt], xt, kind), big, N_BUDGET, band, dom)
