"""Chemical tracers on the device (rcmdyn_set_tracers; the chi chain of tend and bdyval, species.hip's
FamTr instances) against two references.

A, the hydrometeor twin: with ipptls = 2 the engine and the oracle carry qi, qr, qs through the
chain a tracer takes, term for term, where the two families' formulas coincide: no forecast is
negative (the fix factors differ), no coupled value lies in (mintr * ps, minqq^2 * ps] (vadv4d's
thresholds differ), no decoupled value is negative (the tracers have no floor), both relaxation
tables are zero, and the core is hydrostatic: the non-hydrostatic core adds atmx%qx * cr to the
moisture species only (Main/mod_tendency.F90:1615-1617 runs n = 1..nqx), so there a tracer differs
from a hydrometeor by design and reference B checks it.  The twin fields are smooth and strictly
positive; both conditions are asserted from the oracle before anything is compared.

B, tests/tracer_ref.py: a NumPy statement of one tend + one bdyval of chi on one tile, both cores, bit
for bit at every cross point (the chain has no transcendental function; QDOT and, in the hydrostatic
core, XKC of the same tend are exact inputs; the NH diffusion coefficient is restated by the
reference).  It is the only value check of the non-hydrostatic chain.

Then the invariants: passivity, decomposition, the split tend, restart, the refusals, and a Fortran
host.
"""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from regcm_amd.config import QX_PHY_FIELDS, STATE_FIELDS
from tests import tracer_ref as tr
from tests.support import NH_FIELDS, case, engine, oracle, variant_id

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIES = ("QI", "QR", "QS")
MINTR, MINQQ = 1.0e-30, 1.0e-8


def interior(a, rc):
    """jci x ici of a (k, i, j) array; a band keeps every j."""
    return a[:, 1:rc.iy - 2, :] if rc.i_band else a[:, 1:rc.iy - 2, 1:rc.jx - 2]


# ------------------------------------------------------------------------------- A: the twin
def twin_state(rc, st, rough=False):
    """Smooth, strictly positive qi, qr, qs: 1e-6 * ps * a bump + 1e-9 * ps, a bump per species.
    rough: with level-to-level structure (a factor in [0.6, 1.4] per point), so the PBL-top rule of
    vadv4d ind = 3 takes its slope branches."""
    rng = np.random.default_rng(23)
    out = dict(st)
    ps = st["PSA"][0]
    hs = 0.5 * (rc.sigma[1:] + rc.sigma[:-1])
    i, j = np.meshgrid(np.arange(rc.iy), np.arange(rc.jx), indexing="ij")
    for n, sp in enumerate(SPECIES):
        bump = (np.exp(-0.5 * ((hs - (0.35 + 0.2 * n)) / 0.15) ** 2)[:, None, None] *
                (1.0 + 0.5 * np.sin(2 * np.pi * (i + 3 * n) / rc.iy) * np.cos(2 * np.pi * (j - 2 * n) / rc.jx))[None])
        out[f"ATM1_{sp}"] = (1e-6 * bump + 1e-9) * ps[None]
        if rough:
            out[f"ATM1_{sp}"] = out[f"ATM1_{sp}"] * rng.uniform(0.6, 1.4, out[f"ATM1_{sp}"].shape)
        out[f"ATM2_{sp}"] = 0.98 * out[f"ATM1_{sp}"]
    return out


def twin_phy(rc, st):
    rng = np.random.default_rng(5)
    return {n: np.abs(rng.normal(0.0, 1e-10, (rc.kz, rc.iy, rc.jx))) * st["PSA"][0][None] for n in QX_PHY_FIELDS}


def uw_extra(rc):
    """ibltyp = 2: the UW TKE state and, with iuwvadv = 1, a PBL-top field (most columns >= 4)."""
    from regcm_amd import icbc
    if rc.ibltyp != 2:
        return {}
    extra = dict(icbc.tke_state(rc))
    if rc.iuwvadv == 1:
        extra["KPBL"] = np.random.default_rng(5).integers(1, rc.kz + 1, size=(1, rc.iy, rc.jx)).astype(np.float64)
    return extra


def twin_engine(rc, data, st, phy):
    """The engine after its initial bdyval, the tracers put equal to the species as it then holds them
    (that bdyval has set the species' inflow / outflow lines, which the first interior line reads)."""
    e = engine(rc, data, st, extra=phy)
    e.set_tracers(3)
    for n, sp in enumerate(SPECIES):
        e.put_tracer("ATM1", n + 1, e.get(f"ATM1_{sp}"))
        e.put_tracer("ATM2", n + 1, e.get(f"ATM2_{sp}"))
        e.put_tracer("PHY", n + 1, phy[QX_PHY_FIELDS[n]])
    return e


def assert_twin_conditions(rc, st, o, dt):
    """From the oracle alone: no forecast is negative, no coupled value between the two thresholds."""
    ps = st["PSA"][0][None]
    for nm, sp in (("qteni", "QI"), ("qtenr", "QR"), ("qtens", "QS")):
        cq = interior(st[f"ATM2_{sp}"] + dt * o.get_work(nm), rc)
        assert (cq >= 0.0).all(), sp
        a1 = st[f"ATM1_{sp}"][:, :rc.iy - 1, :rc.jx - (0 if rc.i_band else 1)]
        p = ps[:, :rc.iy - 1, :rc.jx - (0 if rc.i_band else 1)]
        assert not ((a1 > MINTR * p) & (a1 <= MINQQ * MINQQ * p)).any(), sp
        assert (a1 >= 0.0).all(), sp


TWIN_VARIANTS = [{}, {"iboudy": 4}, {"upstream_mode": 0}, {"i_band": 1}, {"ibltyp": 2, "iuwvadv": 0},
                 {"ibltyp": 2, "iuwvadv": 1}]


@pytest.mark.parametrize("variant", TWIN_VARIANTS, ids=variant_id)
def test_twin_hydrostatic(variant):
    """C1 (and its band), one tend: tracers 1..3 put equal to qi, qr, qs equal the engine's own
    species and the oracle's on jci x ici, bit for bit (the boundary lines differ by design:
    chem_bdyval against qx's bdyval)."""
    rc, data, st0 = case("C1", ipptls=2, **variant)
    st = twin_state(rc, st0, rough=rc.ibltyp == 2)
    phy = dict(twin_phy(rc, st), **uw_extra(rc))        # iuwvadv = 1: itrvadv = iqxvadv = 3, the rule is shared
    o = oracle(rc, data, st, extra=phy)
    e = twin_engine(rc, data, st, phy)
    dt = o.get_time()[1]
    o.tend()
    assert_twin_conditions(rc, st, o, dt)
    e.tend()
    for n, sp in enumerate(SPECIES):
        for lev in ("ATM1", "ATM2"):
            t = interior(e.get_tracer(lev, n + 1), rc)
            own = interior(e.get(f"{lev}_{sp}"), rc)
            orc = interior(o.get(f"{lev}_{sp}"), rc)
            print(f"twin {variant_id(variant)} {lev}_{sp}: {int((t != own).sum())} differ from the species, "
                  f"{int((t != orc).sum())} from the oracle")
            assert np.array_equal(t, own), (lev, sp)
            assert np.array_equal(t, orc), (lev, sp)
            assert not np.array_equal(t, interior(st[f"{lev}_{sp}"], rc)), (lev, sp)      # the chain ran


# ------------------------------------------------------------------------------- B: the NumPy reference
def patchy_tracers(rc, st, ntr, seed=3):
    """ntr tracers (ATM1, ATM2, PHY, B0, BT per tracer) that exercise every tracer-specific branch:
    patchy fields whose forecasts go negative, serially dependent negatives among them; coupled values
    just under and just over mintr * ps; one negative atm1 value (no decoupling floor)."""
    rng = np.random.default_rng(seed)
    ps = st["PSA"][0][None]
    shape = (rc.kz, rc.iy, rc.jx)
    out = []
    for n in range(ntr):
        pat = rng.uniform(0.0, 2.0e-6, shape) * (rng.uniform(size=shape) < 0.5)
        a1 = pat * ps
        a2 = (0.9 * pat + 1e-8 * (rng.uniform(size=shape) < 0.3)) * ps
        # the vadv4d threshold, both sides: a column of values around mintr * ps
        jj, ii = 7 + n, 9 + 2 * n
        a1[2, ii, jj] = 0.5 * MINTR * ps[0, ii, jj]
        a1[3, ii, jj] = 2.0 * MINTR * ps[0, ii, jj]
        a1[4, ii, jj] = MINTR * ps[0, ii, jj]
        # one negative atm1 value: atmx%chi keeps its sign (no floor)
        a1[5, ii + 2, jj + 3] = -3.0e-7 * ps[0, ii + 2, jj + 3]
        phy = rng.normal(0.0, 2e-10, shape) * ps
        b0 = (1.0e-6 * (1.0 + 0.3 * np.sin(0.3 * np.arange(rc.jx))[None, None, :]) * np.ones(shape)) * ps
        bt = rng.normal(0.0, 1e-12, shape) * ps
        out.append({"ATM1": a1, "ATM2": a2, "PHY": phy, "B0": b0, "BT": bt})
    return out


def nudge_tables(rc):
    """Smooth positive tables of the size and shape of the engine's own hefc / hegc (Main/mod_bdycod.F90:
    204-256): fnudge = 0.1 / dt and gnudge = 1 / (50 dt) times exp(-(ib - 2) / an), an by level."""
    hs = 0.5 * (rc.sigma[1:] + rc.sigma[:-1])
    an = np.where(hs < 0.4, rc.high_nudge, np.where(hs < 0.8, rc.medium_nudge, rc.low_nudge))
    ib = np.arange(1, rc.nspgx + 1, dtype=np.float64)
    w = np.exp(-(ib[None, :] - 2.0) / an[:, None])
    return (0.1 / rc.dt) * w, (1.0 / (rc.dt * 50.0)) * w


def put_tracers(e, tracers):
    for n, t in enumerate(tracers):
        for name, a in t.items():
            e.put_tracer(name, n + 1, a)


def reference_run(rc, st, tracers, tables, e, clock0, clock1, kpbl=None):
    """The reference's result of one tend + bdyval for every tracer, from the pre-step state and the
    engine's QDOT / XKC of the same tend; also the count of serially dependent negatives.  clock0,
    clock1: (lcount, dt, xbctime) before the tend and after it."""
    cefc, cegc = tables
    xkc = tr.nh_xkc(rc, st) if rc.idynamic == 2 else e.get("XKC")
    step = tr.StepInputs.from_state(rc, st, e.get("QDOT"), xkc, clock0[1], clock0[2] + clock0[1],
                                    clock1[2] + clock1[1], kpbl=kpbl)
    res, dep = [], 0
    for t in tracers:
        r = tr.tend_bdyval(rc, step, t["ATM1"], t["ATM2"], t["PHY"], t["B0"], t["BT"], cefc, cegc)
        dep += r.ndependent
        res.append(r)
    return res, dep


REF_CASES = [("C1", {}, 4), ("C1", {}, 1), ("G4", {}, 4), ("C1", {"iboudy": 1}, 2), ("C1", {"iboudy": 3}, 2),
             ("C1", {"idiffu": 2}, 2), ("C1", {"upstream_mode": 0}, 2), ("C1", {"ibltyp": 2, "iuwvadv": 1}, 2),
             ("N1", {}, 4), ("N1", {"ibltyp": 2, "iuwvadv": 1}, 2), ("N1", {"idiffu": 2, "iboudy": 1}, 1)]


@pytest.mark.parametrize("grid,variant,ntr", REF_CASES, ids=lambda v: variant_id(v) if isinstance(v, dict) else str(v))
def test_reference(grid, variant, ntr):
    """One tend + bdyval of either core (C1, a 70 x 68 grid; N1: the non-hydrostatic chain without the
    cr term, its diffusion coefficient restated by the reference; ibltyp = 2 with iuwvadv = 1: the
    PBL-top rule of vadv4d ind = 3 with the host's kpbl) against tests/tracer_ref.py at every cross
    point, boundary lines included:
    ntr = 4 crosses a group of three; non-zero cefc / cegc, TR_PHY, B0 / BT that differ from the
    state; patchy tracers with serially dependent negatives (counted by the reference, asserted
    above zero); values on both sides of mintr * ps; one negative atm1 value."""
    if grid == "G4":
        rc, data, st = case("C1", jx=70, iy=68, nspgx=None, nspgd=None, **variant)
    else:
        rc, data, st = case(grid, **variant)
    tracers = patchy_tracers(rc, st, ntr)
    tables = nudge_tables(rc)
    extra = uw_extra(rc)
    e = engine(rc, data, st, extra=extra)
    e.set_diagnostics(True)           # QDOT and XKC of the tend are read back
    e.set_tracers(ntr)
    put_tracers(e, tracers)
    e.put_tracer_nudge(*tables)
    # the state the tend starts from: the engine's initial bdyval has set the boundary lines of u, v, p*
    held = dict(st)
    held.update({name: e.get(name) for name in ("ATM1_U", "ATM1_V", "PSA", "PSB", "ATM2_U", "ATM2_V")})
    if rc.idynamic == 2:
        held["ATM2_W"] = e.get("ATM2_W")
    clock0 = e.get_time()
    e.tend()
    clock1 = e.get_time()
    e.bdyval()
    ref, dep = reference_run(rc, held, tracers, tables, e, clock0, clock1, extra["KPBL"][0] if "KPBL" in extra else None)
    print(f"ref {grid} {variant_id(variant)} ntr={ntr}: {sum(r.nnegative for r in ref)} negative forecasts, "
          f"{dep} serially dependent")
    assert dep > 0
    for n in range(ntr):
        for lev, want in (("ATM1", ref[n].atm1), ("ATM2", ref[n].atm2)):
            got = e.get_tracer(lev, n + 1)[:, :rc.iy - 1, :rc.jx - 1]
            nd = int((got != want[:, :rc.iy - 1, :rc.jx - 1]).sum())
            print(f"ref {grid} {variant_id(variant)} ntr={ntr} tracer {n + 1} {lev}: {nd} points differ")
            assert nd == 0, (n + 1, lev, nd)


# ------------------------------------------------------------------------------- invariants
def smooth_tracers(rc, st, ntr):
    """Smooth positive tracers (no negative forecast meets a tile edge, where the reference's own fix
    depends on the decomposition), with B0 / BT that differ from the state."""
    ps = st["PSA"][0][None]
    hs = 0.5 * (rc.sigma[1:] + rc.sigma[:-1])
    i, j = np.meshgrid(np.arange(rc.iy), np.arange(rc.jx), indexing="ij")
    rng = np.random.default_rng(17)
    out = []
    for n in range(ntr):
        f = (0.3 + np.exp(-0.5 * ((hs - (0.3 + 0.15 * n)) / 0.2) ** 2)[:, None, None] *
             (1.0 + 0.4 * np.sin(2 * np.pi * (i + n) / rc.iy) * np.cos(2 * np.pi * j / rc.jx))[None])
        a1 = 1e-6 * f * ps
        out.append({"ATM1": a1, "ATM2": 0.97 * a1, "PHY": np.abs(rng.normal(0.0, 1e-10, a1.shape)) * ps,
                    "B0": 1.1 * a1, "BT": 1e-6 * a1})
    return out


def tracer_fields(e, ntr):
    return {(lev, n): e.get_tracer(lev, n) for n in range(1, ntr + 1) for lev in ("ATM1", "ATM2")}


@pytest.mark.parametrize("core", ["C1", "N1"])
def test_passive(core):
    """ntr = 2 declared and filled: every other state field after 3 steps is bit-identical to a run
    that never called set_tracers; with ntr = 0 the step launches the same kernels."""
    rc, data, st = case(core)
    names = NH_FIELDS if rc.idynamic == 2 else STATE_FIELDS
    ref = engine(rc, data, st)
    trc = engine(rc, data, st)
    trc.set_tracers(2)
    put_tracers(trc, patchy_tracers(rc, st, 2))
    trc.put_tracer_nudge(*nudge_tables(rc))
    ref.step(3)
    trc.step(3)
    for name in names:
        assert np.array_equal(ref.get(name), trc.get(name)), name
    assert not np.array_equal(trc.get_tracer("ATM1", 1), patchy_tracers(rc, st, 1)[0]["ATM1"])
    off = engine(rc, data, st)
    off.set_tracers(2)
    off.set_tracers(0)
    plain = engine(rc, data, st)
    assert sorted(off.kernel_times(1)) == sorted(plain.kernel_times(1))
    assert any(k.startswith("k_tr_") or k.startswith("k_nh_tr_") for k in trc.kernel_times(1))


DECOMP = [("C1", (2, 2), None), ("C1", (1, 3), None), ("N1", (2, 2), None), ("C1", (2, 2), "RCMDYN_NO_GRAPH"),
          ("C1", (2, 2), "RCMDYN_FORCE_RCCL"), ("N1", (2, 2), "RCMDYN_NO_GRAPH")]


@pytest.mark.parametrize("core,nproc,env", DECOMP, ids=str)
def test_decomposition(monkeypatch, core, nproc, env):
    """In-process tiles, 2 steps, non-zero tables: every tracer field bit-identical to one tile; the
    same eagerly and with the halos sent over RCCL to self."""
    rc, data, st = case(core)
    tracers = smooth_tracers(rc, st, 4)
    runs = []
    for np_ in ((1, 1), nproc):
        if np_ != (1, 1) and env:
            monkeypatch.setenv(env, "1")
        e = engine(rc, data, st, np_)
        e.set_tracers(4)
        put_tracers(e, tracers)
        e.put_tracer_nudge(*nudge_tables(rc))
        e.step(2)
        runs.append(tracer_fields(e, 4))
    for key in runs[0]:
        assert np.array_equal(runs[0][key], runs[1][key]), key


def test_many_tracers_decomposed():
    """ntr = 34 (twelve groups, the last of one tracer) on 2 x 2 tiles: the grouped prologue exchange
    carries 68 more fields than one k_pack_segs launch holds and the staging grows by 5 field-widths
    per tracer; every tracer bit-identical to one tile after 2 steps."""
    rc, data, st = case("C1")
    ntr = 34
    base = smooth_tracers(rc, st, 4)
    runs = []
    for np_ in ((1, 1), (2, 2)):
        e = engine(rc, data, st, np_)
        e.set_tracers(ntr)
        for n in range(ntr):
            t = base[n % 4]
            for name in ("ATM1", "ATM2", "B0"):
                e.put_tracer(name, n + 1, (1.0 + 0.01 * n) * t[name])
        e.put_tracer_nudge(*nudge_tables(rc))
        e.step(2)
        runs.append(tracer_fields(e, ntr))
    for key in runs[0]:
        assert np.array_equal(runs[0][key], runs[1][key]), key
    assert not np.array_equal(runs[0][("ATM1", 34)], runs[0][("ATM1", 30)])


def test_band_bdyval():
    """chem_bdyval_coupled on the band (no west / east line): after tend + bdyval the south and north
    rows hold chib = chia of the tend over every j and chia = chib0 + xt * chibt; every other point,
    the periodic sides among them, is what the tend left."""
    rc, data, st = case("C1", i_band=1)
    tracers = smooth_tracers(rc, st, 2)
    a, b = engine(rc, data, st), engine(rc, data, st)
    for e in (a, b):
        e.set_tracers(2)
        put_tracers(e, tracers)
        e.tend()
    clock = b.get_time()
    b.bdyval()
    xt = clock[2] + clock[1]
    for n, t in enumerate(tracers):
        a1, a2 = a.get_tracer("ATM1", n + 1), a.get_tracer("ATM2", n + 1)
        want1, want2 = a1.copy(), a2.copy()
        for row in (0, rc.iy - 2):
            want2[:, row, :] = a1[:, row, :]
            want1[:, row, :] = (t["B0"] + xt * t["BT"])[:, row, :]
        assert np.array_equal(b.get_tracer("ATM1", n + 1)[:, :rc.iy - 1], want1[:, :rc.iy - 1]), n + 1
        assert np.array_equal(b.get_tracer("ATM2", n + 1)[:, :rc.iy - 1], want2[:, :rc.iy - 1]), n + 1
        assert not np.array_equal(want1, a1)


@pytest.mark.parametrize("core", ["C1", "N1"])
def test_split_tend(core):
    """tend_pre_physics, put TR_PHY, tend_post_physics equals tend with the same TR_PHY; TR_CHIB3D
    is max(atm2 * rpsb, 0) as the reference module states it."""
    rc, data, st = case(core)
    tracers = patchy_tracers(rc, st, 2)
    whole = engine(rc, data, st)
    split = engine(rc, data, st)
    for e in (whole, split):
        e.set_tracers(2)
        put_tracers(e, [{k: v for k, v in t.items() if k != "PHY" or e is whole} for t in tracers])
    whole.tend()
    split.tend_pre_physics()
    for n, t in enumerate(tracers):
        want = tr.chib3d(t["ATM2"], st["PSB"][0])
        got = split.get_tracer("CHIB3D", n + 1)
        assert np.array_equal(got[:, :rc.iy - 1, :rc.jx - 1], want[:, :rc.iy - 1, :rc.jx - 1]), n + 1
        split.put_tracer("PHY", n + 1, t["PHY"])
    split.tend_post_physics()
    a, b = tracer_fields(whole, 2), tracer_fields(split, 2)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def test_restart():
    """2 steps, the tracers' SAV fields with the rest of the state into a fresh engine, 2 more: the
    same bits as 4 straight steps."""
    from regcm_amd.dycore import DynCore
    rc, data, st = case("C1")
    tracers = smooth_tracers(rc, st, 2)
    ref = engine(rc, data, st)
    ref.set_tracers(2)
    put_tracers(ref, tracers)
    ref.put_tracer_nudge(*nudge_tables(rc))
    ref.step(2)
    sav = {n: ref.get(n) for n in STATE_FIELDS}
    tsav = tracer_fields(ref, 2)
    rst = DynCore(rc, data["split"])
    for n in ("MSFX", "MSFD", "CORIOL", "HT", "XUB_B0", "XUB_BT", "XVB_B0", "XVB_BT", "XTB_B0", "XTB_BT",
              "XQB_B0", "XQB_BT", "XPSB_B0", "XPSB_BT"):
        rst.put(n, st[n])
    for n, a in sav.items():
        rst.put(n, a)
    rst.set_tracers(2)
    for (lev, n), a in tsav.items():
        rst.put_tracer(lev, n, a)
    for n, t in enumerate(tracers):
        for name in ("PHY", "B0", "BT"):
            rst.put_tracer(name, n + 1, t[name])
    rst.put_tracer_nudge(*nudge_tables(rc))
    rst.set_time(*ref.get_time())
    ref.step(2)
    rst.step(2)
    a, b = tracer_fields(ref, 2), tracer_fields(rst, 2)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def test_refusals():
    """Every refusal names its option and leaves the engine usable."""
    from regcm_amd.config import MAXTR
    from regcm_amd.dycore import DynCore, EngineError
    rc, data, st = case("C1")
    z = np.zeros((rc.kz, rc.iy, rc.jx))
    e = engine(rc, data, st)
    with pytest.raises(EngineError, match="no tracers are declared"):
        e.put_tracer("ATM1", 1, z)
    with pytest.raises(EngineError, match="RCMDYN_MAXTR"):
        e.set_tracers(MAXTR + 1)
    with pytest.raises(EngineError, match="ichebdy"):
        e.set_tracers(2, ichebdy=0)
    e.set_tracers(2)
    for itr in (0, 3):
        with pytest.raises(EngineError, match="itr"):
            e.put_tracer("ATM1", itr, z)
        with pytest.raises(EngineError, match="itr"):
            e.get_tracer("ATM1", itr)
    with pytest.raises(EngineError, match="read-only"):
        e.put_tracer("CHIB3D", 1, z)
    with pytest.raises(EngineError, match="put-only"):
        e.get_tracer("PHY", 1)
    with pytest.raises(EngineError, match="rcmdyn_tend_pre_physics"):
        e.get_tracer("CHIB3D", 1)
    with pytest.raises(EngineError, match="unknown tracer field"):
        e.put_tracer(17, 1, z)
    e.set_tracers(0)
    with pytest.raises(EngineError, match="no tracers are declared"):
        e.put_tracer("ATM1", 1, z)
    with pytest.raises(EngineError, match="no tracers are declared"):
        e.put_tracer_nudge(np.zeros((rc.kz, rc.nspgx)), np.zeros((rc.kz, rc.nspgx)))
    e.step(1)                              # still usable
    for opt, msg in (({"idiffu": 3}, "idiffu = 3"), ({"isladvec": 1}, "isladvec = 1")):
        rcv, datav, stv = case("C1", **opt)
        ev = engine(rcv, datav, stv)
        with pytest.raises(EngineError, match=msg):
            ev.set_tracers(1)
        ev.step(1)
    with pytest.raises(EngineError, match="ichem.*rcmdyn_set_tracers"):
        DynCore(dataclasses.replace(rc, ichem=1), data["split"])


# ------------------------------------------------------------------------------- a Fortran host
DRIVER = r"""
program tracer_host
  use iso_c_binding
  use mod_gpu_dyn
  implicit none
  type(rcmdyn_config) :: cfg
  type(c_ptr) :: h
  integer :: u, nf, q, f, nk, n, jx, iy, kz, itr
  real(c_double), allocatable :: a(:)
  character(len=256) :: dir
  integer(c_int8_t), allocatable :: raw(:)
  call get_command_argument(1, dir)
  allocate(raw(c_sizeof(cfg)))
  open(newunit=u, file=trim(dir)//'/cfg.bin', access='stream', form='unformatted', status='old')
  read(u) raw
  close(u)
  cfg = transfer(raw, cfg)
  jx = cfg%jx; iy = cfg%iy; kz = cfg%kz
  call gpu_dyn_check(c_null_ptr, rcmdyn_create(cfg, h), 'create')
  open(newunit=u, file=trim(dir)//'/fields.bin', access='stream', form='unformatted', status='old')
  read(u) nf
  do q = 1, nf
    read(u) f, nk
    allocate(a(jx*iy*nk))
    read(u) a
    call gpu_dyn_check(h, rcmdyn_put(h, f, a, 1, jx, 1, iy, 1, nk), 'put')
    deallocate(a)
  end do
  call gpu_dyn_check(h, rcmdyn_bdyval(h), 'bdyval')
  call gpu_dyn_check(h, rcmdyn_set_tracers(h, 2, 1), 'set_tracers')
  allocate(a(jx*iy*kz))
  do itr = 1, 2
    do f = tr_atm1, tr_bt
      read(u) a
      call gpu_dyn_check(h, rcmdyn_put_tracer(h, f, itr, a, 1, jx, 1, iy, 1, kz), 'put_tracer')
    end do
  end do
  deallocate(a)
  allocate(a(2*cfg%nspgx*kz))
  read(u) a
  close(u)
  n = cfg%nspgx*kz
  call gpu_dyn_check(h, rcmdyn_put_tracer_nudge(h, a(1:n), a(n+1:2*n)), 'put_tracer_nudge')
  deallocate(a)
  call gpu_dyn_check(h, rcmdyn_step(h, 2), 'step')
  allocate(a(jx*iy*kz))
  open(newunit=u, file=trim(dir)//'/out.bin', access='stream', form='unformatted', status='replace')
  do itr = 1, 2
    do f = tr_atm1, tr_atm2
      call gpu_dyn_check(h, rcmdyn_get_tracer(h, f, itr, a, 1, jx, 1, iy, 1, kz), 'get_tracer')
      write(u) a
    end do
  end do
  close(u)
  call gpu_dyn_check(h, rcmdyn_destroy(h), 'destroy')
end program tracer_host
"""


def test_fortran_host(tmp_path):
    """A Fortran host with ntr = 2 through mod_gpu_dyn is bit-identical to the Python host after 2
    steps of C1."""
    import ctypes
    from regcm_amd.config import FIELD, build_config, field_levels
    rc, data, st = case("C1")
    tracers = smooth_tracers(rc, st, 2)
    tables = nudge_tables(rc)
    fdir = os.path.join(ROOT, "regcm_amd", "fortran")
    src = tmp_path / "tracer_host.f90"
    src.write_text(DRIVER)
    exe = tmp_path / "tracer_host"
    subprocess.run(["/opt/rocm/bin/amdflang", "-O1", "-module-dir", str(tmp_path), os.path.join(fdir, "mod_gpu_dyn.F90"),
                    str(src), "-o", str(exe), "-L", os.path.join(ROOT, "regcm_amd"), "-lrcmdyn",
                    "-Wl,-rpath," + os.path.join(ROOT, "regcm_amd")], check=True, cwd=tmp_path)
    cfg = build_config(rc, data["split"])
    (tmp_path / "cfg.bin").write_bytes(bytes(ctypes.string_at(ctypes.byref(cfg), ctypes.sizeof(cfg))))
    with open(tmp_path / "fields.bin", "wb") as fh:
        fh.write(np.int32(len(st)).tobytes())
        for name, a in st.items():
            fh.write(np.array([FIELD[name], field_levels(name, rc.kz, rc.nsplit)], dtype=np.int32).tobytes())
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for t in tracers:
            for name in ("ATM1", "ATM2", "PHY", "B0", "BT"):
                fh.write(np.ascontiguousarray(t[name], dtype=np.float64).tobytes())
        for tab in tables:
            fh.write(np.ascontiguousarray(tab, dtype=np.float64).tobytes())
    subprocess.run([str(exe), str(tmp_path)], check=True)
    out = np.fromfile(tmp_path / "out.bin").reshape(2, 2, rc.kz, rc.iy, rc.jx)
    e = engine(rc, data, st)
    e.set_tracers(2)
    put_tracers(e, tracers)
    e.put_tracer_nudge(*tables)
    e.step(2)
    for n in range(2):
        for q, lev in enumerate(("ATM1", "ATM2")):
            assert np.array_equal(out[n, q], e.get_tracer(lev, n + 1)), (n + 1, lev)
