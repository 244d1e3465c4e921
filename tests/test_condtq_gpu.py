"""GPU tests of the SUBEX condensation inside tend (rcmdyn_set_condtq; condtq.hpp, the condtq
instances of k_scalars / k_update and k_nh_tend_c).

The yardstick is tests/condtq_ref.py: a NumPy transcription of the Fortran text and the two-pass
oracle built on it (the oracle stubs condtq but accepts TPHY / QVPHY / QCPHY).  condtq has no
transcendental function, so wherever its inputs are the engine's own the tests ask for equal
bits.  Against the oracle, the bound after one tend + bdyval is the one the parity tests hold the
same case to without condtq (tests/test_parity_gpu.py: 1e-12 for C1; tests/test_nh_gpu.py: 1e-11
for N1), with the points within 1e-9 of a cloud-cover threshold on the oracle's side left out (at
most 0.1 % of a level).

After ten more steps those bounds (1e-10, 1e-9) cannot hold, for a cause that lies in the
reference: where a cloud evaporates, tmp2 = -qccs / dt leaves a qc forecast of rounding noise of
either sign, and the negative-moisture fix (Main/mod_tendency.F90:382-393) replaces a negative one,
however small, by 0.01 x the mean of |qc| of its nine neighbours.  From the second step on the qc
totals carry the ulp differences of the condensing points (their tmp1 follows t and qv, which are
downstream of pow / log), so the sign of that noise, and with it a qc of 1e-3 of the field's
maximum, differs at single points; the difference then spreads through the latent heating.  The
two-pass reference alone shows the same growth under a 1e-14 perturbation of its initial
temperature (tests/test_condtq_cpu.py; 1.7e-3 in qc after two steps in both).  TEN holds the
errors measured after the eleventh step (engine against two-pass oracle, the larger of one tile
and 2 x 2 tiles); the bound is 4 x that.  The exact-placement test after three warm
steps is the tight multi-step check.
"""
import dataclasses

import numpy as np
import pytest

from regcm_amd import icbc
from regcm_amd.config import CONFIGS
from regcm_amd.dycore import CONDTQ_TERMS, EngineError
from tests import condtq_ref as cq
from tests.support import CROSS, case, engine, oracle, relerr, state_names

pytestmark = pytest.mark.gpu

TENS = ["TTEN", "QVTEN", "QCTEN"]
INCS = ["T", "QV", "QC"]
# one tend + bdyval: the bounds of the parity tests without condtq
ONE = {"C": 1e-12, "N": 1e-11}
# after the eleventh step: the measured relative max-norm errors (see above); the bound is 4 x
TEN = {
    "C": {"ATM1_U": 9.46e-05, "ATM1_V": 2.28e-04, "ATM1_T": 8.45e-05, "ATM1_QV": 5.06e-03, "ATM1_QC": 1.40e-02,
          "ATM2_U": 1.01e-04, "ATM2_V": 2.51e-04, "ATM2_T": 5.16e-05, "ATM2_QV": 4.97e-03, "ATM2_QC": 8.99e-03,
          "PSA": 5.00e-06, "PSB": 4.72e-06, "DSTOR": 6.14e-04, "HSTOR": 4.57e-07},
    "N": {"ATM1_U": 1.99e-05, "ATM1_V": 1.03e-04, "ATM1_T": 1.88e-05, "ATM1_QV": 1.70e-04, "ATM1_QC": 4.60e-03,
          "ATM2_U": 1.00e-05, "ATM2_V": 7.27e-05, "ATM2_T": 1.68e-05, "ATM2_QV": 1.55e-04, "ATM2_QC": 3.26e-03,
          "PSA": 0.0, "PSB": 0.0, "ATM1_PP": 1.66e-04, "ATM2_PP": 1.80e-04, "ATM1_W": 6.60e-04, "ATM2_W": 3.95e-04},
}


def setup(name, **over):
    """(rc, data, the moistened state, rh0adj) of a 37 x 29 cut."""
    if name == "N":
        over.setdefault("ifrayd", 0)
    rc, data, st0 = case(name, **over)
    return rc, data, cq.moist_state(rc, st0), cq.rh0adj_field(rc)


def odd_grid():
    """34 x 23: the 31 x 20 interior ends inside the last 32 x 8 block of both directions."""
    rc = dataclasses.replace(CONFIGS["C1"], jx=34, iy=23, nspgx=None, nspgd=None)
    data = icbc.generate(rc)
    return rc, data, cq.moist_state(rc, data["state"]), cq.rh0adj_field(rc)


def on_engine(rc, data, st, rh0, nproc=(1, 1), conf=1.0, diag=False):
    e = engine(rc, data, st, nproc=nproc)
    if diag:
        e.set_diagnostics(True)
    e.set_condtq(True, conf)
    e.put_rh0adj(rh0)
    return e


def same(a, b, what):
    assert np.array_equal(a, b), (what, int((a != b).sum()))


def same_state(a, b, names):
    assert a.get_time() == b.get_time()
    for n in names:
        same(a.get(n), b.get(n), n)


def increments(e):
    return {n: e.get_condtq(n) for n in INCS}


# ------------------------------------------------------------------ 1. off by default, refusals
@pytest.mark.parametrize("name", ["C", "N"])
def test_off_is_the_engine_without_condtq(name):
    rc, data, st, rh0 = setup(name)
    names = state_names(rc)
    a, b = engine(rc, data, st), engine(rc, data, st)
    b.set_condtq(True, 0.5)                  # on, fed, and off again: nothing is left of it
    b.put_rh0adj(rh0)
    b.set_condtq(False)
    for e in (a, b):
        e.set_diagnostics(True)
        e.step(3)
        e.tend()
    for n in TENS:
        same(a.get(n), b.get(n), n)
    for e in (a, b):
        e.bdyval()
    same_state(a, b, names)
    ka, kb = a.kernel_times(2), b.kernel_times(2)
    assert {k: v[0] for k, v in ka.items()} == {k: v[0] for k, v in kb.items()}
    with pytest.raises(EngineError, match="condtq is off"):
        b.get_condtq("T")


def test_refusals():
    rc, data, st, rh0 = setup("C")
    e = engine(rc, data, st)
    for conf in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(EngineError, match="conf"):
            e.set_condtq(True, conf)
    with pytest.raises(EngineError, match="condtq is off"):      # the refused calls left it off
        e.get_condtq("RH0ADJ")
    with pytest.raises(EngineError, match="condtq is off"):
        e.put_rh0adj(rh0)
    e.set_condtq(True, 1.0)
    for call in (e.tend, lambda: e.step(1), e.tend_post_physics):
        with pytest.raises(EngineError, match="no rh0adj was put"):
            call()
    for bad in (-1e-9, 0.999991, float("nan")):
        r = rh0.copy()
        r[3, 7, 9] = bad
        with pytest.raises(EngineError, match=r"\[0, 0.99999\]"):
            e.put_rh0adj(r)
    with pytest.raises(EngineError, match="no rh0adj was put"):  # a refused put is no put
        e.tend()
    e.put_rh0adj(rh0)
    same(e.get_condtq("RH0ADJ")[cq.interior(rc)], rh0[cq.interior(rc)], "rh0adj")
    with pytest.raises(EngineError, match="conf"):               # refused: the switch stays on
        e.set_condtq(True, 2.0)
    e.tend()
    e.bdyval()
    with pytest.raises(EngineError, match="unknown term"):
        e.get_condtq(len(CONDTQ_TERMS))
    # ipptls = 2: the reference does not call condtq
    rc2, data2, st2 = case("C", ipptls=2)
    e2 = engine(rc2, data2, st2)
    with pytest.raises(EngineError, match="ipptls = 1"):
        e2.set_condtq(True, 1.0)
    e2.step(1)


@pytest.mark.parametrize("nproc", [(1, 1), (2, 2)], ids=["one-tile", "2x2"])
def test_tend_waits_for_a_put_that_covers_the_interior(nproc):
    """Boxes that leave out a level, a row or a column of the interior are stored but do not arm
    tend, before the first covering put and after an off / on cycle (whose buffer still holds
    the earlier values); after the covering put a smaller box updates the buffer."""
    rc, data, st, rh0 = setup("C")
    e = engine(rc, data, st, nproc=nproc)
    e.set_condtq(True, 1.0)
    c = cq.interior(rc)
    inner = rh0[c]                                           # (kz, ici1:ici2, jci1:jci2), at j1 = i1 = 2
    for box, at in ((inner[1:], dict(j1=2, i1=2, k1=2)), (inner[:, 1:], dict(j1=2, i1=3)),
                    (inner[:, :, :-1], dict(j1=2, i1=2))):
        e.put_rh0adj(np.ascontiguousarray(box), **at)
        with pytest.raises(EngineError, match="no rh0adj was put"):
            e.tend()
    e.put_rh0adj(np.ascontiguousarray(inner), j1=2, i1=2)    # the interior alone covers it
    e.tend()
    e.bdyval()
    e.set_condtq(False)
    e.set_condtq(True, 1.0)
    e.put_rh0adj(np.ascontiguousarray(inner[1:]), j1=2, i1=2, k1=2)
    with pytest.raises(EngineError, match="no rh0adj was put"):
        e.step(1)
    e.put_rh0adj(rh0)
    half = np.full_like(inner[:, :5, :7], 0.5)
    e.put_rh0adj(half, j1=2, i1=2)
    want = rh0.copy()
    want[:, 1:6, 1:8] = 0.5
    same(e.get_condtq("RH0ADJ")[c], want[c], "rh0adj")
    e.step(1)


# ------------------------------------------------------------------ 2. exact placement
def transcription_on_twin(rc, data, st, rh0, conf, warm):
    """One tend of a twin engine with condtq off for that tend (on for the warm steps before it),
    split at the physics seam for ATMS_QSB3D (pre + post is bit-identical to tend): the
    transcription on its totals."""
    t = on_engine(rc, data, st, rh0, conf=conf, diag=True)
    t.step(warm)
    t.set_condtq(False)
    before = {n: t.get(n) for n in ("ATM2_T", "ATM2_QV", "ATM2_QC")}
    dt = t.get_time()[1]
    t.tend_pre_physics()
    t.tend_post_physics()
    psc = t.get("PSC")[0]
    c = cq.interior(rc)
    pres = (cq.hsigma(rc)[:, None, None] * psc + rc.ptop) * 1000.0
    off = {n: t.get(n) for n in TENS}
    out = cq.condtq(before["ATM2_T"][c], before["ATM2_QV"][c], before["ATM2_QC"][c], off["TTEN"][c], off["QVTEN"][c],
                    off["QCTEN"][c], psc[c[1:]], pres[c], t.get("ATMS_QSB3D")[c], rh0[c], dt, conf)
    return off, out


@pytest.mark.parametrize("grid,warm", [("37x29", 0), ("37x29", 3), ("34x23", 0)])
def test_exact_placement_hydrostatic(grid, warm):
    """warm = 3: after the start-up steps (the dt switch, filtered levels, noise-level qc left by
    evaporated cloud)."""
    rc, data, st, rh0 = setup("C") if grid == "37x29" else odd_grid()
    conf = 0.8
    c = cq.interior(rc)
    names = state_names(rc)
    off, out = transcription_on_twin(rc, data, st, rh0, conf, warm)
    npts = out["on"].size
    for key in ("low", "high", "part"):
        assert out[key].sum() >= 0.01 * npts, key
    assert (~out["left"]).sum() >= 0.01 * npts and (~out["on"]).sum() > 0
    e = on_engine(rc, data, st, rh0, conf=conf, diag=True)
    e.step(warm)
    e.tend()
    inc = increments(e)
    for key, n, ten in (("it", "T", "TTEN"), ("iqv", "QV", "QVTEN"), ("iqc", "QC", "QCTEN")):
        want = np.zeros_like(inc[n])
        want[c] = out[key]
        same(inc[n], want, "increment of " + n)
        total = off[ten].copy()
        total[c] = off[ten][c] + out[key]
        same(e.get(ten)[c], total[c], ten)
    # the forecast state: an engine with condtq off that is given the transcription's increments
    # as the host's physics tendencies, ((x + 0) + d) = (x + (0 + d))
    p = on_engine(rc, data, st, rh0, conf=conf)
    p.step(warm)
    p.set_condtq(False)
    for key, n in (("it", "TPHY"), ("iqv", "QVPHY"), ("iqc", "QCPHY")):
        a = np.zeros((rc.kz, rc.iy, rc.jx))
        a[c] = out[key]
        p.put(n, a)
    p.tend()
    same_state(e, p, names)
    e.bdyval()
    p.bdyval()
    same_state(e, p, names)


# ------------------------------------------------------------------ 3. against the two-pass oracle
def masked(a, b, near, rc, name):
    """a with b's values at the interior points the reference leaves out (3-D cross fields)."""
    if name not in CROSS or a.shape[0] != rc.kz or not near.any():
        return a
    a = a.copy()
    v = a[cq.interior(rc)]
    v[near] = b[cq.interior(rc)][near]
    a[cq.interior(rc)] = v
    return a


def run_against_two_pass(name, nproc=(1, 1), tiles=None, more=10, probe_over=None, **over):
    """From the start state, which the engine and the oracle hold bit for bit after the same puts
    and the (exact) initial bdyval (an oracle cannot take a state over in mid-run: bdyval's
    boundary slices are not among the put fields): one tend + bdyval, then `more` steps.
    over: the case's option overrides; probe_over: those of the first step's probe, where it
    needs its own (cq.TwoPass)."""
    rc, data, st, rh0 = setup(name, **over)
    names = state_names(rc)
    e = on_engine(rc, data, st, rh0, nproc=nproc)
    probe = None
    if probe_over is not None:
        prc, pdata, _ = case(name, **probe_over)
        probe = lambda: oracle(prc, pdata, st, tiles=tiles)
    tp = cq.TwoPass(lambda: oracle(rc, data, st, tiles=tiles), rc, names, rh0, probe=probe)
    R = tp.R
    for n in names:
        assert relerr(e.get(n), R.get(n), rc, n) == 0.0, n
    assert e.get_time() == R.get_time()
    inc, out = tp.step()
    e.tend()
    near = out["near"]
    assert np.all(near.sum(axis=(1, 2)) <= 0.001 * near[0].size)
    got = increments(e)
    # the increments, to the bound of the state: where a cloud evaporates dt x the qc increment
    # is the cloud water itself, so max |dt x increment| is of the size of max |qc|, and the
    # forecast qc2 + dt x (total + increment) holds its bound only if the increment does
    ierr = {n: relerr(masked(got[n], inc[key], near, rc, "ATM1_T"), inc[key], rc, "ATM1_T")
            for n, key in (("T", "TPHY"), ("QV", "QVPHY"), ("QC", "QCPHY"))}
    print(name, over, "increments", ierr)
    for n in INCS:
        assert ierr[n] < ONE[name], (n, ierr[n])
    e.bdyval()
    assert e.get_time() == R.get_time()
    errs = {n: relerr(masked(e.get(n), R.get(n), near, rc, n), R.get(n), rc, n) for n in names}
    print(name, "one step", errs)
    for n in names:
        assert errs[n] < ONE[name], (n, errs[n])
    if not more:
        return
    for s in range(more):
        inc, out = tp.step()
        near = near | out["near"]
        e.step(1)
        errs = {n: relerr(masked(e.get(n), R.get(n), near, rc, n), R.get(n), rc, n) for n in names}
        print(name, "step", s + 2, {k: float(f"{v:.2e}") for k, v in errs.items()})
    assert np.all(near.sum(axis=(1, 2)) <= 0.001 * near[0].size)
    assert e.get_time() == R.get_time()
    for n in names:
        assert errs[n] <= 4.0 * TEN[name][n], (n, errs[n])


@pytest.mark.parametrize("name", ["C", "N"])
def test_two_pass_oracle(name):
    run_against_two_pass(name)


@pytest.mark.parametrize("nproc", [(1, 1), (2, 2)], ids=["one-tile", "2x2"])
def test_two_pass_oracle_band(nproc):
    """A tropical band (i_band = 1): the grid is periodic in j, so the ghost columns of even one
    tile are interior points of the far side; the step computes their forecasts as their owners
    do, and the negative-moisture fix reads them.  rh0adj must reach them from the wrapped
    column.  cq.moist_state lays cloud across the period's seam for this.  One tend + bdyval."""
    run_against_two_pass("C", nproc=nproc, tiles=None if nproc == (1, 1) else nproc, more=0, i_band=1)


def test_two_pass_oracle_nh_before_the_rayleigh_damping():
    """ifrayd = 1: condtq runs before the Rayleigh damping of t and qv, with pres from the total
    of pp before its damping (Main/mod_tendency.F90:336-364, 466-470).  The probe of the step
    runs with ifrayd = 0 (cq.TwoPass).  One tend + bdyval."""
    rc, _, _ = case("N", ifrayd=1)
    assert rc.ifrayd == 1 and rc.rayndamp >= 1
    run_against_two_pass("N", more=0, probe_over={"ifrayd": 0}, ifrayd=1)


@pytest.mark.parametrize("name", ["C", "N"])
def test_qc_total_and_psc_equal_the_oracles_bit_for_bit(name):
    """What the evaporating branch tmp2 = -qccs / dt rests on: without condtq the first tend's
    total of qc and psc are the oracle's bits at every interior point (neither chain has a
    transcendental function), so qccs is, and a sign disagreement of the evaporated qc forecast
    after later steps is no operation-order difference in them."""
    rc, data, st, _ = setup(name)
    c = cq.interior(rc)
    e, o = engine(rc, data, st), oracle(rc, data, st)
    e.set_diagnostics(True)
    e.tend()
    o.step(1)
    same(e.get("QCTEN")[c], o.get("QCTEN")[c], "QCTEN")
    if name == "C":                          # the NH core's psc is its psa, a put field
        same(e.get("PSC")[0][c[1:]], o.get("PSC")[0][c[1:]], "PSC")


# ------------------------------------------------------------------ 4. every path agrees
@pytest.mark.parametrize("name", ["C", "N"])
def test_every_path_bit_for_bit(name):
    rc, data, st, rh0 = setup(name)
    names = state_names(rc)
    rh1 = cq.rh0adj_field(rc, seed=23)
    eager, graph, split = (on_engine(rc, data, st, rh0) for _ in range(3))
    nsteps = 5                               # the one- and the two-step graphs, both parities
    for s in range(nsteps):
        eager.tend()
        eager.bdyval()
    graph.step(nsteps)
    for s in range(nsteps):
        split.tend_pre_physics()
        split.put_rh0adj(rh0)                # the host's cldfrac runs between the halves
        split.tend_post_physics()
        split.bdyval()
    ie = increments(eager)
    assert all(ie[n].any() for n in INCS)
    for other in (graph, split):
        same_state(eager, other, names)
        io = increments(other)
        for n in INCS:
            same(ie[n], io[n], n)
    # a new rh0adj between two replays is read by the captured graphs as they are
    keep = {n: graph.get(n) for n in names}
    for e in (eager, graph):
        e.put_rh0adj(rh1)
    eager.tend()
    eager.bdyval()
    graph.step(1)
    same_state(eager, graph, names)
    for n in INCS:
        same(eager.get_condtq(n), graph.get_condtq(n), n)
    old = on_engine(rc, data, st, rh0)
    old.step(nsteps + 1)
    assert any(not np.array_equal(old.get(n), graph.get(n)) for n in names) and keep


# ------------------------------------------------------------------ 5. tiles
@pytest.mark.parametrize("transport", ["copy", "rccl"])
def test_tiles_against_two_pass_oracle_tiles(transport, monkeypatch):
    if transport == "rccl":
        monkeypatch.setenv("RCMDYN_FORCE_RCCL", "1")
    run_against_two_pass("C", nproc=(2, 2), tiles=(2, 2))


@pytest.mark.parametrize("name", ["C", "N"])
def test_tiles_first_tend_equals_one_tile(name):
    """Pointwise and without an exchange: one tend on 2 x 2 tiles gives the increments of one tile
    bit for bit (the states part later, at the tile-dependent negative-moisture sweep)."""
    rc, data, st, rh0 = setup(name)
    one, dec = on_engine(rc, data, st, rh0), on_engine(rc, data, st, rh0, nproc=(2, 2))
    for e in (one, dec):
        e.tend()
    for n in INCS:
        same(one.get_condtq(n), dec.get_condtq(n), n)
    same(one.get_condtq("RH0ADJ")[cq.interior(rc)], dec.get_condtq("RH0ADJ")[cq.interior(rc)], "rh0adj")


# ------------------------------------------------------------------ 6. coexistence
@pytest.mark.parametrize("name", ["C", "N"])
def test_budget_and_massck_leave_it_unchanged(name):
    rc, data, st, rh0 = setup(name)
    names = state_names(rc)
    a, b = on_engine(rc, data, st, rh0), on_engine(rc, data, st, rh0)
    b.set_budget(True, rw=0.25)
    b.set_massck(True, 16)
    for e in (a, b):
        e.step(2)
        e.tend()
        e.bdyval()
    same_state(a, b, names)
    for n in INCS:
        same(a.get_condtq(n), b.get_condtq(n), n)
    assert b.get_budget("T_ADH").any() and len(b.get_massck()[0]) == 3
