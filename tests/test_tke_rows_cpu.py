"""The oracle against tests/tke_ref.py, the NumPy statement of one step of the UW-PBL TKE in the
hydrostatic core (ibltyp = 2) written from the Fortran text: hadv3d with ind = 1 in both
upstream_mode branches, tkeps, vadv3d with nk = kzp1, diffu_x3df with nuk at idiffu 1, 2 and 3, the sum
with tkephy, the forecast with its tkemin floor, the Robert-Asselin filter with gnu2, and bdyval's TKE
lines.  Two steps of tend + bdyval from the state after the initial bdyval, each restated from the
run's own state at its start (the second because bdyval's atm2 = atm1 copies change nothing in the
first, where both time levels hold tkemin on the lines).

Grids: the 37 x 29 and 34 x 23 cuts of C1 (tests/test_dyn_rows_cpu.py).  Variants: default,
upstream_mode 0, idiffu 2, idiffu 3, iboudy 4, iboudy 3.

Inputs (tke_inputs): icbc.tke_state alone is too tame, so atm1 / atm2 tke are a boundary-layer profile
times a horizontal wave pattern (different in the two time levels) plus a 4 x 4 patch, floored at
tkemin, and TKEPHY is a wave of both signs of up to 1.5 atm2 / dt, so that the forecast falls on the
floor over a part of the domain.  The zonal wind is made to reverse along the west and east lines
(reversing_flow), which the generated westerly flow does not.

Tolerance: none.  QDOT first (the restated compute_omega, so that a TKE mismatch is localised), then
ATM1_TKE and ATM2_TKE after tend and after bdyval, bit for bit at every cross point of the kz + 1
levels, boundary lines included.  The only values read from the run under test besides the inputs are
atm1 u, v after tend, of which bdyval's inflow / outflow test reads the first interior lines (they
come out of splitf, restated in tests/test_oracle_rows_cpu.py); they decide a sign, no value.

Not vacuous, asserted from the restatement: the floor is active at 1 % or more of the interior points
and inactive at 1 % or more; levels 1 and kz + 1 (no horizontal advection, dds = 0) change; every
boundary line holds inflow and outflow points; each of the advection, diffusion and physics terms
moves the forecast by more than 2**20 ulp at the median interior point, so leaving any out, or a
relative error of 1e-6 in one, cannot pass.
"""
import functools

import numpy as np
import pytest

from tests import dyn_ref as dr
from tests import tke_ref as tr
from tests.support import case, oracle, variant_id
from tests.test_dyn_rows_cpu import GRIDS, prepared

VARIANTS = [{}, {"upstream_mode": 0}, {"idiffu": 2}, {"idiffu": 3}, {"iboudy": 4}, {"iboudy": 3}]
BDY = ("XUB_B0", "XUB_BT", "XVB_B0", "XVB_BT")

grid_variant = pytest.mark.parametrize("grid,variant", [(g, v) for g in GRIDS for v in VARIANTS],
                                       ids=lambda p: p if isinstance(p, str) else variant_id(p))


def tke_inputs(rc):
    """{ATM1_TKE, ATM2_TKE, TKEPHY}: see the module docstring."""
    kz, iy, jx = rc.kz, rc.iy, rc.jx
    sig = np.asarray(rc.sigma, dtype=np.float64)[:, None, None]
    k = np.arange(kz + 1, dtype=np.float64)[:, None, None]
    i = np.arange(1, iy + 1, dtype=np.float64)[None, :, None]
    j = np.arange(1, jx + 1, dtype=np.float64)[None, None, :]
    prof = 1.5 * np.exp(-(1.0 - sig) / 0.08) + 0.05
    out = {}
    for n, name in enumerate(("ATM1_TKE", "ATM2_TKE")):
        t = prof * (1.0 + 0.5 * np.sin(2.0 * np.pi * (j + 2.0 * n) / 9.0) * np.cos(2.0 * np.pi * (i - n) / 7.0) +
                    0.2 * np.sin(0.9 * k + 0.37 * i + 0.23 * j + n))
        t[:, 9:13, 11:15] += 2.0                                 # a 4 x 4 patch, off the band on both grids
        out[name] = np.maximum(t, rc.tkemin)
    out["TKEPHY"] = out["ATM2_TKE"] / rc.dt * 1.5 * np.sin(2.0 * np.pi * (i + j) / 11.0) * np.cos(np.pi * k / 5.0)
    for a in out.values():
        a[:, iy - 1, :] = 0.0
        a[:, :, jx - 1] = 0.0
    return out


def reversing_flow(rc, st):
    """The generated flow is westerly at every level, so the whole west line blows in and the whole east
    line out.  p*u of both time levels and of the boundary value is multiplied by cos(2 pi i / 14 +
    0.35 k): the zonal wind reverses along the west and east lines, at other rows on other levels."""
    i = np.arange(1, rc.iy + 1, dtype=np.float64)[None, :, None]
    k = np.arange(rc.kz, dtype=np.float64)[:, None, None]
    w = np.cos(2.0 * np.pi * i / 14.0 + 0.35 * k)
    out = dict(st)
    for name in ("ATM1_U", "ATM2_U", "XUB_B0", "XUB_BT"):
        out[name] = st[name] * w
    return out


def start(grid, variant):
    rc, data, st = case("C", ibltyp=2, **GRIDS[grid], **variant)
    st = reversing_flow(rc, prepared(rc, st))
    tke = tke_inputs(rc)
    st.update({n: tke[n] for n in ("ATM1_TKE", "ATM2_TKE")})
    return rc, data, st, {"TKEPHY": tke["TKEPHY"]}


def two_steps(c, names=dr.HYDRO_INPUTS + tr.TKE_INPUTS, more=()):
    """Drive the started core c (oracle or engine) through tend and bdyval twice: for each step the
    inputs (names), the times, and what tend (with the fields `more`) and bdyval leave."""
    out = []
    for _ in range(2):
        g = {n: c.get(n) for n in names}
        _, dt0, _ = c.get_time()
        c.tend()
        mid = {n: c.get(n) for n in ("ATM1_TKE", "ATM2_TKE", "QDOT", "ATM1_U", "ATM1_V") + tuple(more)}
        _, dt1, xbc1 = c.get_time()
        c.bdyval()
        end = {n: c.get(n) for n in ("ATM1_TKE", "ATM2_TKE")}
        out.append((g, dt0, (dt1, xbc1), mid, end))
    c.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle_run(grid, vkey):
    rc, data, st, extra = start(grid, dict(vkey))
    return rc, two_steps(oracle(rc, data, st, extra=extra))


def ulps(a, b):
    """|a - b| in units of the spacing at b."""
    return np.abs(a - b) / np.spacing(np.abs(b))


def line_exists(rc):
    G = dr.geom(rc)
    return G.left or G.right or G.bottom or G.top


def check_tke(tag, rc, step, first, tiles=None):
    """One step's record (two_steps) against the restatement, bit for bit, with the non-vacuity asserts.
    The first bdyval past the start finds atm2 equal to atm1 on the lines (both tkemin), so that
    bdyval's atm2 = atm1 copies are seen to act in the second step only."""
    g, dt0, times1, mid, end = step
    kz = rc.kz
    G = dr.geom(rc)
    cross = (slice(None), slice(0, G.ice2), slice(0, G.jce2))
    m = tr.interior(rc)
    r = tr.tke_tend(rc, g, g["ATM1_TKE"], g["ATM2_TKE"], g["TKEPHY"], dt0, tiles=tiles)
    # qdot first: what the TKE's vertical advection reads
    assert np.abs(r["qdot"][1:kz][:, m]).min() > 0.0 and not r["qdot"][0].any() and not r["qdot"][kz].any()
    assert np.array_equal(mid["QDOT"][cross], r["qdot"][cross]), "QDOT"
    # ---- the restatement's own edges
    on_floor = (r["raw"] < rc.tkemin)[:, m]
    print(f"{tag}: the tkemin floor is active at {on_floor.mean():.3f} of the interior points")
    assert 0.01 <= on_floor.mean() <= 0.99
    for lev in (0, kz):
        assert not r["had"][lev].any() and not r["adv"][lev].any()      # no advection there: dds(1) = dds(kzp1) = 0
        assert (r["a1"][lev][m] != g["ATM1_TKE"][lev][m]).mean() > 0.5 and (r["a2"][lev][m] != g["ATM2_TKE"][lev][m]).all()
    assert (r["had"][1:kz][:, m] != 0.0).all() and ((r["adv"] - r["had"])[:, m][1:kz] != 0.0).all()
    unit = np.spacing(np.abs(r["raw"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        rpsa = np.where(g["PSA"][0] > 0, 1.0 / g["PSA"][0], 0.0)
    terms = {"hadv3d": r["had"] * rpsa, "vadv3d": (r["adv"] - r["had"]) * rpsa, "diffu_x3df": dr.total(r["dif"]) * rpsa,
             "tkephy": g["TKEPHY"]}
    for name, term in terms.items():
        sup = m
        if name == "diffu_x3df" and rc.idiffu == 3:
            sup = np.zeros_like(m)
            for jcol, i1, i2 in dr.tile_columns(rc, False, tiles):
                sup[i1 - 1:i2, jcol - 1] = True
            assert not term[:, m & ~sup].any()
        lev = slice(1, kz) if name.endswith("adv3d") else slice(None)
        strength = float(np.median((np.abs(dt0 * term) / unit)[lev][:, sup]))
        print(f"{tag}: median |dt {name}| = 2**{np.log2(strength):.1f} ulp of the forecast")
        assert strength >= 2.0 ** 20, (name, strength)
    # ---- after tend
    for name, key in (("ATM1_TKE", "a1"), ("ATM2_TKE", "a2")):
        got, want = mid[name][cross], r[key][cross]
        bad = got != want
        print(f"{tag} {name} after tend: {int(bad.sum())} of {bad.size} points differ"
              + (f", worst {ulps(got, want)[bad].max():.1f} ulp" if bad.any() else ""))
        assert not bad.any(), (name, "after tend", np.argwhere(bad)[:5].tolist())
    # ---- after bdyval
    dt1, xbc1 = times1
    b = {n: g[n] for n in BDY} if line_exists(rc) else None
    w1, w2, inflow = tr.tke_bdyval(rc, r["a1"], r["a2"], mid["ATM1_U"], mid["ATM1_V"], b, xbc1 + dt1)
    assert set(inflow) == {s for s, has in (("west", G.left), ("east", G.right), ("south", G.bottom), ("north", G.top)) if has}
    for side, flow in inflow.items():
        print(f"{tag}: {side} line, inflow at {flow.mean():.3f} of its points")
        assert flow.any() and not flow.all(), side
    line = G.box("e", False) & ~m
    if line.any():
        assert (w1[:, line] != r["a1"][:, line]).any() and (first or (w2[:, line] != r["a2"][:, line]).any())
    else:                                                        # no side, no line: bdyval changes no TKE value
        assert m.all() and np.array_equal(w1, r["a1"]) and np.array_equal(w2, r["a2"])
    assert np.array_equal(w1[:, m], r["a1"][:, m]) and np.array_equal(w2[:, m], r["a2"][:, m])
    for name, want in (("ATM1_TKE", w1), ("ATM2_TKE", w2)):
        got = end[name][cross]
        bad = got != want[cross]
        print(f"{tag} {name} after bdyval: {int(bad.sum())} of {bad.size} points differ")
        assert not bad.any(), (name, "after bdyval", np.argwhere(bad)[:5].tolist())


@grid_variant
def test_tke_step_bit_for_bit(grid, variant):
    rc, steps = _oracle_run(grid, tuple(sorted(variant.items())))
    for n, step in enumerate(steps):
        check_tke(f"{grid} {variant_id(variant)} step {n + 1}", rc, step, n == 0)


def test_tke_inputs_vary_in_every_direction():
    rc, _, st, extra = start("37x29", {})
    for name in ("ATM1_TKE", "ATM2_TKE"):
        a = st[name][:, 1:rc.iy - 2, 1:rc.jx - 2]
        assert all((np.diff(a, axis=ax) != 0.0).mean() > 0.9 for ax in (0, 1, 2)) and a.min() >= rc.tkemin
    phy = extra["TKEPHY"][:, 1:rc.iy - 2, 1:rc.jx - 2]
    assert (phy > 0.0).mean() > 0.25 and (phy < 0.0).mean() > 0.25
    assert not np.array_equal(st["ATM1_TKE"], st["ATM2_TKE"])


def test_tke_idiffu3_on_tiles():
    """idiffu = 3 depends on the decomposition: the oracle run as 2 x 2 tiles against the restatement
    given the tiles' bounds (each tile's column jci2; the interior column's clamp does not act).  The
    tiled oracle advances by whole steps, so the winds of bdyval's inflow test are read after the
    step: bdyval leaves the first interior lines, which are all the test reads of them, as tend left
    them."""
    from regcm_amd.dycore import tile_extent
    rc, data, st, extra = start("37x29", {"idiffu": 3})
    tiles = [tile_extent(rc.jx, rc.iy, 2, 2, t) for t in range(4)]
    cols = dr.tile_columns(rc, False, tiles)
    assert sorted(cols) == [(19, 2, 15), (19, 16, 27), (35, 2, 15), (35, 16, 27)]
    o = oracle(rc, data, st, tiles=(2, 2), extra=extra)
    g = {n: o.get(n) for n in dr.HYDRO_INPUTS + tr.TKE_INPUTS}
    _, dt0, xbc0 = o.get_time()
    o.step(1)
    end = {n: o.get(n) for n in ("ATM1_TKE", "ATM2_TKE", "ATM1_U", "ATM1_V")}
    o.close()
    r = tr.tke_tend(rc, g, g["ATM1_TKE"], g["ATM2_TKE"], g["TKEPHY"], dt0, tiles=tiles)
    one = tr.tke_tend(rc, g, g["ATM1_TKE"], g["ATM2_TKE"], g["TKEPHY"], dt0)
    assert not np.array_equal(r["a1"][:, :, 18], one["a1"][:, :, 18])       # the interior tiles' column
    w1, w2, _ = tr.tke_bdyval(rc, r["a1"], r["a2"], end["ATM1_U"], end["ATM1_V"], {n: g[n] for n in BDY}, xbc0 + dt0)
    cross = (slice(None), slice(0, rc.iy - 1), slice(0, rc.jx - 1))
    for name, want in (("ATM1_TKE", w1), ("ATM2_TKE", w2)):
        assert np.array_equal(end[name][cross], want[cross]), name
