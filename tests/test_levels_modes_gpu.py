"""The engine (through the C-ABI) at every nsplit and at the level counts rcmdyn_create accepts and no
other GPU test runs: nsplit 1, 3, 4 beside the default 2, kz 14, 41 and the bound 64 beside 18 and 23.

What these select.  nsplit >= 3 leaves the fused split step on any domain (2 aam(l) = 4 (nsplit - l + 1)
exceeds its 8 sub-steps): k_spstep_init, then k_spstep_grad / k_spstep_update with three exchanges per
sub-step, the rings of the forecasts exchanged instead of computed, the corrections launched by tend on
tiles, the instances k_split_correct<1|3|4> and k_split_correct_bdy<1|3|4>, DSTOR / HSTOR with nsplit
levels.  kz sets the dynamic LDS of k_columns (2048 kz bytes: 131 072 at kz = 64) and of k_split_project,
and kz = 64 is where the per-level constant arrays meet their last element.

Grids: C1 and N1 cut to 37 x 29, and C1 cut to 34 x 23 where named (tests/test_dyn_rows_cpu.py describes
both).  kz = 64 has no table in the reference, which forms sigma by formula for any kz: the 41-level table
interpolated linearly to 65 full levels stands in, registered below.

Tolerances.  Against the oracle: the initial bdyval exactly, 1 step < 1e-12 and 2 more < 1e-11 in relative
max-norm for kz <= 23 (tests/test_parity_gpu.py: libm against device ulps downstream of log / pow).  Those
bounds were derived at 18 to 23 levels; for kz >= 41 the bound is max(that, 100 spread), spread the
relative max-norm between two oracle runs whose initial ATM1_T differs by the factor 1 + 1e-14
(test_variant_parity's long leg).  Everything engine against engine is bit for bit.
"""
import functools

import numpy as np
import pytest

from regcm_amd import config
from regcm_amd.config import STATE_FIELDS
from tests.support import (NH_FIELDS, advance, case, crop, engine, oracle, pair, physics_tendencies, relerr,
                           state_names, variant_id)

pytestmark = pytest.mark.gpu

# 65 full levels from the 41-level table; cached RunConfigs read the table later, so it stays registered
config.SIGMA_TABLES.setdefault(
    64, [float(x) for x in np.interp(np.linspace(0.0, 41.0, 65), np.arange(42.0), config.SIGMA_TABLES[41])])

G34 = dict(jx=34, iy=23, nspgx=7, nspgd=7)
GRIDS = {"37x29": {}, "34x23": G34}
ONE = (1, 1)
TOL = ((1, 1e-12), (2, 1e-11))
NS3 = dict(nsplit=3)


def _id(p):
    if isinstance(p, dict):
        return variant_id(p)
    return "x".join(map(str, p)) if isinstance(p, tuple) else str(p)


def substeps(nsplit):
    """The sub-steps of one split step: the sum over the modes of 2 aam(l) = 4 (nsplit - l + 1)."""
    return 2 * nsplit * (nsplit + 1)


def base_names(kt):
    """kernel_times by base name: k_spstep_fused<8> -> k_spstep_fused, k_scalars_km<opt> -> k_scalars."""
    base = {}
    for name, v in kt.items():
        b = name.split("<")[0]
        b = b[:-3] if b.endswith("_km") else b
        base[b] = base.get(b, 0) + v[0]
    return base


def fields_of(e, names):
    return {n: e.get(n) for n in names}


def assert_same_fields(a, b, tag=""):
    assert a.keys() == b.keys()
    for n in a:
        assert np.array_equal(a[n], b[n]), (tag, n)


# ------------------------------------------------------------------------------- a. against the oracle
def check_parity(tag, rc, data, st, nproc=ONE, tiles=None):
    """The initial bdyval exactly, then 1 step and 2 more at TOL; kz >= 41: max(TOL, 100 spread)."""
    o, e = pair(rc, data, st, nproc=nproc, tiles=tiles)
    names = state_names(rc, tke=True)
    for name in names:
        assert relerr(e.get(name), o.get(name), rc, name) == 0.0, (tag, name)
    p = None
    if rc.kz >= 41:
        stp = dict(st)
        stp["ATM1_T"] = st["ATM1_T"] * (1.0 + 1e-14)
        p = oracle(rc, data, stp, tiles=tiles)
    for nsteps, tol in TOL:
        for c in (o, e) + ((p,) if p else ()):
            c.step(nsteps)
        worst = ("", 0.0, 0.0)
        for name in names:
            ref = o.get(name)
            err = relerr(e.get(name), ref, rc, name)
            spread = relerr(p.get(name), ref, rc, name) if p else 0.0
            if p:
                print(f"{tag} +{nsteps} {name}: err = {err:.3e}, spread = {spread:.3e}")
            if err >= worst[1]:
                worst = (name, err, spread)
            if p:
                assert err <= max(tol, 100.0 * spread), (tag, name, err, spread, nsteps)
            else:
                assert err < tol, (tag, name, err, nsteps)
        print(f"{tag} +{nsteps}: worst err = {worst[1]:.3e} ({worst[0]}), its spread = {worst[2]:.3e}")
    assert e.get_time() == o.get_time()


HYDRO = [(14, 2), (41, 2), (64, 2), (18, 1), (18, 3), (18, 4), (14, 4), (41, 3), (64, 1)]


@pytest.mark.parametrize("grid,kz,nsplit", [("37x29", k, n) for k, n in HYDRO] + [("34x23", 18, 3), ("34x23", 41, 2)],
                         ids=_id)
def test_hydrostatic_matches_oracle(grid, kz, nsplit):
    """With tests/test_dyn_rows_cpu.py's cloud layer, so that the qc chain and bdyval's qc inflow / outflow
    (which reads the winds the split step corrected) carry values."""
    from tests.test_dyn_rows_cpu import prepared
    rc, data, st = case("C", kz=kz, nsplit=nsplit, **GRIDS[grid])
    check_parity(f"C {grid} kz={kz} nsplit={nsplit}", rc, data, prepared(rc, st, patch=False))


@pytest.mark.parametrize("kz", [14, 23, 64])
def test_nonhydrostatic_matches_oracle(kz):
    rc, data, st = case("N", kz=kz)
    check_parity(f"N 37x29 kz={kz}", rc, data, st)


@pytest.mark.parametrize("variant", [{"iboudy": 4}, {"idiffu": 3}, {"isladvec": 1}, {"ibltyp": 2}, {"ipptls": 2},
                                     {"i_band": 1}], ids=variant_id)
def test_three_modes_variants_match_oracle(variant):
    """kz = 18, nsplit = 3.  On the band halo is true on one tile: its self-exchange runs the un-fused path."""
    rc, data, st = case("C", **NS3, **variant)
    check_parity(f"C 37x29 nsplit=3 {variant_id(variant)}", rc, data, st)


# ------------------------------------------------------------------------------- b. the path did run
@pytest.mark.parametrize("nsplit,nproc", [(1, ONE), (2, ONE), (3, ONE), (4, ONE), (3, (2, 2))], ids=_id)
def test_split_step_kernels_launched(nsplit, nproc):
    """One eager step (rcmdyn_kernel_times): which split-step kernels ran and how often, and the same state
    as step(1).  On tiles at nsplit = 3 tend launches the corrections itself (k_split_correct, then
    k_bdyval_set) where one tile runs them with the boundary lines (k_split_correct_bdy)."""
    rc, data, st = case("C", nsplit=nsplit)
    a, b = engine(rc, data, st, nproc), engine(rc, data, st, nproc)
    base = base_names(a.kernel_times(1))
    b.step(1)
    names = state_names(rc)
    assert_same_fields(fields_of(a, names), fields_of(b, names), "kernel_times against step")
    ntiles = nproc[0] * nproc[1]
    shown = {k: v for k, v in base.items() if k.startswith(("k_spstep", "k_split", "k_bdyval_set"))}
    print(f"nsplit={nsplit} {_id(nproc)}: {shown}")
    if nsplit >= 3:
        assert "k_spstep_fused" not in base, shown
        assert base.get("k_spstep_init") == ntiles, shown
        assert substeps(nsplit) == {3: 24, 4: 40}[nsplit]
        assert base.get("k_spstep_grad") == substeps(nsplit) * ntiles, shown
        assert base.get("k_spstep_update") == substeps(nsplit) * ntiles, shown
    else:
        assert base.get("k_spstep_fused") == ntiles, shown
        for k in ("k_spstep_init", "k_spstep_grad", "k_spstep_update"):
            assert k not in base, shown
    assert base.get("k_split_project") == ntiles, shown
    if nsplit >= 3 and ntiles > 1:
        assert base.get("k_split_correct") == ntiles and base.get("k_bdyval_set") == ntiles, shown
        assert "k_split_correct_bdy" not in base, shown
    else:
        assert base.get("k_split_correct_bdy") == ntiles and "k_split_correct" not in base, shown


# ------------------------------------------------------------------------------- c. exact across nsplit
def _cloudy(nsplit):
    """The generated state has no cloud: with tests/test_dyn_rows_cpu.py's layer (qc = 1 % of qv)."""
    from tests.test_dyn_rows_cpu import prepared
    rc, data, st = case("C", nsplit=nsplit)
    return rc, data, prepared(rc, st, patch=False)


@functools.lru_cache(maxsize=None)
def _hydro_one_step(nsplit, nproc):
    rc, data, st = _cloudy(nsplit)
    e = engine(rc, data, st, nproc)
    e.step(1)
    out = fields_of(e, ("ATM1_QV", "ATM2_QV", "ATM1_QC", "ATM2_QC", "ATM1_T"))
    e.close()
    return out


@pytest.mark.parametrize("nproc", [ONE, (2, 2)], ids=_id)
@pytest.mark.parametrize("nsplit", [1, 3, 4])
def test_moisture_after_one_step_ignores_nsplit(nsplit, nproc):
    """The first step's qv and qc forecasts do not see the split step.  At nsplit = 3 the tiles exchange
    the CQV / CQC ring that the nsplit = 2 tiles compute.  ATM1_T does see it: the option reached the engine.
    With cloud in the state, the boundary lines of ATM1_QC see it as well, in the engine and in the oracle:
    bdyval's qc inflow / outflow (Main/mod_bdycod.F90:2153-2223) chooses by the boundary winds, which the
    split step has corrected; ATM1_QC is therefore compared on jci x ici."""
    rc = _cloudy(nsplit)[0]
    for name in ("ATM1_QV", "ATM1_QC", "ATM1_T"):
        assert np.array_equal(_cloudy(nsplit)[2][name], _cloudy(2)[2][name]), name
    got, ref = _hydro_one_step(nsplit, nproc), _hydro_one_step(2, nproc)
    for name in ("ATM1_QV", "ATM2_QV", "ATM2_QC"):
        assert np.array_equal(got[name], ref[name]), name
        assert got[name].any(), name
    inner = (slice(None), slice(1, rc.iy - 2), slice(1, rc.jx - 2))
    assert np.array_equal(got["ATM1_QC"][inner], ref["ATM1_QC"][inner]) and got["ATM1_QC"][inner].any()
    assert not np.array_equal(got["ATM1_T"], ref["ATM1_T"])


@functools.lru_cache(maxsize=None)
def _nh_four_steps(nsplit, nproc):
    rc, data, st = case("N", nsplit=nsplit)
    e = engine(rc, data, st, nproc)
    e.step(4)
    out = fields_of(e, NH_FIELDS)
    e.close()
    return out


@pytest.mark.parametrize("nproc", [ONE, (2, 2)], ids=_id)
@pytest.mark.parametrize("nsplit", [1, 3, 4])
def test_nonhydrostatic_ignores_nsplit(nsplit, nproc):
    """The non-hydrostatic core has no split step: every prognostic field after 4 steps, bit for bit."""
    assert_same_fields(_nh_four_steps(nsplit, nproc), _nh_four_steps(2, nproc))


# ------------------------------------------------------------------------------- d. tiles on the un-fused path
@functools.lru_cache(maxsize=None)
def _six_steps(grid, vkey, nproc):
    rc, data, st = case("C", **GRIDS[grid], **dict(vkey))
    e = engine(rc, data, st, nproc)
    e.step(6)
    out = fields_of(e, state_names(rc, tke=True))
    e.close()
    return out


TILINGS = [("37x29", (2, 1)), ("37x29", (2, 2)), ("37x29", (1, 3)), ("34x23", (2, 2))]
TILED = ([(g, v, t) for v in ({}, {"iboudy": 4}, {"isladvec": 1, "ibltyp": 2}) for g, t in TILINGS] +
         [("37x29", {"i_band": 1}, t) for t in ((2, 1), (3, 1))])


@pytest.mark.parametrize("grid,variant,nproc", TILED, ids=_id)
def test_three_modes_tiles_bit_identical(grid, variant, nproc):
    key = tuple(sorted(dict(variant, **NS3).items()))
    assert_same_fields(_six_steps(grid, key, ONE), _six_steps(grid, key, nproc))


@pytest.mark.parametrize("nproc", [(2, 2), (1, 3)], ids=_id)
@pytest.mark.parametrize("variant", [{"ipptls": 2}, {"idiffu": 3}], ids=variant_id)
def test_three_modes_tiles_match_oracle_tiles(variant, nproc):
    """ipptls = 2 (the moisture fix's in-tile sweep) and idiffu = 3 (each tile's last column) depend on the
    tiling as the reference's do: against the oracle run as the same tiles."""
    rc, data, st = case("C", **NS3, **variant)
    check_parity(f"C 37x29 nsplit=3 {variant_id(variant)} {_id(nproc)}", rc, data, st, nproc=nproc, tiles=nproc)


def _tracer_run(rc, data, st, nproc, tracers):
    from tests.test_tracers_gpu import nudge_tables, put_tracers, tracer_fields
    e = engine(rc, data, st, nproc)
    e.set_tracers(len(tracers))
    put_tracers(e, tracers)
    e.put_tracer_nudge(*nudge_tables(rc))
    e.step(2)
    return tracer_fields(e, len(tracers))


def test_three_modes_tracers_tiles_bit_identical():
    """Four tracers on 2 x 2 tiles: the chi ring is exchanged only when the split step is not fused."""
    from tests.test_tracers_gpu import smooth_tracers
    rc, data, st = case("C", **NS3)
    tracers = smooth_tracers(rc, st, 4)
    one, til = _tracer_run(rc, data, st, ONE, tracers), _tracer_run(rc, data, st, (2, 2), tracers)
    for key, a in one.items():
        assert not np.array_equal(a, tracers[key[1] - 1][key[0]]), key          # the chain ran
    assert_same_fields(one, til)


def test_three_modes_tiles_over_rccl(monkeypatch):
    """The per-sub-step messages (delh's slot, uu / vv, dhsum) through RCCL's self communicator
    (RCMDYN_FORCE_RCCL) are the device copies' bit for bit."""
    rc, data, st = case("C", **NS3)
    names = state_names(rc)
    ref = _six_steps("37x29", tuple(sorted(NS3.items())), (2, 2))
    monkeypatch.setenv("RCMDYN_FORCE_RCCL", "1")
    e = engine(rc, data, st, (2, 2))
    e.step(6)
    assert_same_fields(fields_of(e, names), ref)


def test_forty_one_levels_tiles_bit_identical():
    """kz = 41, nsplit = 2 on 2 x 2 tiles: parts 1 and 2 of k_columns with its 83 968-byte LDS block."""
    key = (("kz", 41),)
    assert_same_fields(_six_steps("37x29", key, ONE), _six_steps("37x29", key, (2, 2)))


# ------------------------------------------------------------------------------- e. call paths
@pytest.mark.parametrize("nproc", [ONE, (2, 2)], ids=_id)
@pytest.mark.parametrize("kz,nsplit", [(18, 3), (41, 2)])
def test_call_paths_bit_identical(kz, nsplit, nproc):
    """rcmdyn_step, the tend + bdyval pair and the physics seam, each holding the same *PHY tendencies,
    over 5 steps.  (On tiles at nsplit = 3 the pair's tend cannot defer its corrections:
    test_split_step_kernels_launched sees them launched.)"""
    rc, data, st = case("C", kz=kz, nsplit=nsplit)
    phy = physics_tendencies(rc)
    names = state_names(rc)
    runs = {}
    for path in ("step", "pair", "physics"):
        e = engine(rc, data, st, nproc, extra=phy)
        advance(e, path, 5, phy)
        runs[path] = (fields_of(e, names), e.get_time())
        e.close()
    for path in ("pair", "physics"):
        assert_same_fields(runs[path][0], runs["step"][0], path)
        assert runs[path][1] == runs["step"][1]
    plain = engine(rc, data, st, nproc)
    plain.step(5)
    assert not np.array_equal(plain.get("ATM1_T"), runs["step"][0]["ATM1_T"])       # the tendencies did act


# ------------------------------------------------------------------------------- f. state transfer
@pytest.mark.parametrize("nsplit", [1, 3, 4])
def test_dstor_hstor_levels(nsplit):
    """DSTOR / HSTOR carry nsplit levels: a put followed by a get returns the array, and after a step
    every level holds something."""
    rc, data, st = case("C", nsplit=nsplit)
    e = engine(rc, data, st)
    rng = np.random.default_rng(5)
    for name in ("DSTOR", "HSTOR"):
        a = rng.standard_normal((nsplit, rc.iy, rc.jx))
        assert e.get(name).shape == a.shape
        e.put(name, a)
        assert np.array_equal(crop(e.get(name), rc, name), crop(a, rc, name)), name
        e.put(name, st[name])
    e.step(1)
    for name in ("DSTOR", "HSTOR"):
        a = e.get(name)
        assert all(a[l].any() for l in range(nsplit)), name
        if nsplit > 1:
            assert not np.array_equal(a[0], a[nsplit - 1]), name


@pytest.mark.parametrize("over,nproc", [(NS3, ONE), (NS3, (2, 2)), ({"kz": 14}, ONE)], ids=_id)
def test_restart_bit_identical(over, nproc):
    """tests/test_restart_gpu.py's form: every state field and the clock into a fresh engine."""
    rc, data, st = case("C", **over)
    ref = engine(rc, data, st)
    ref.step(7)
    run = engine(rc, data, st)
    run.step(4)
    sav = fields_of(run, STATE_FIELDS)
    clock = run.get_time()
    run.close()
    rst = engine(rc, data, st, nproc=nproc, bdyval=False)
    for name, a in sav.items():
        rst.put(name, a)
    rst.set_time(*clock)
    rst.step(3)
    assert_same_fields(fields_of(rst, STATE_FIELDS), fields_of(ref, STATE_FIELDS))
    assert rst.get_time() == ref.get_time()
