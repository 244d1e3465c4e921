"""The tracers' cumulus mixing (rcmdyn_set_cumtran; k_tr_cumtran) and their budget
(rcmdyn_set_tracer_budget; the TrBudget instances of k_qx_tend / k_nh_qx_tend) on the device.

cumtran needs no chain reference: tracers are passive, so two engines from one state, one with the
switch off and one with it on, hold the same fields up to the first acting tend, and after it the
second holds tests/cumtran_ref.py applied to the first's, bit for bit (no transcendental function).
The four stage terms of the budget are compared with tests/tracer_diag_ref.py as test_tracers_gpu's
test_reference compares the state: QDOT and the scaled XKC of the same tend are exact inputs.

All cases run on the 37 x 29 x 18 cuts case("C") / case("N") (odd, no multiple of the wave or the
block) with ntr = 4 (two groups, 3 + 1) unless said otherwise.
"""
import os
import subprocess

import numpy as np
import pytest

from regcm_amd.config import TRACER_DIAG_TERMS
from tests import cumtran_ref as cu
from tests import tracer_diag_ref as td
from tests import tracer_ref as tr
from tests.support import case, engine, variant_id
from tests.test_tracers_gpu import (nudge_tables, patchy_tracers, put_tracers, smooth_tracers, tracer_fields,
                                    uw_extra)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTR = 4
STAGES = ("ADVH", "ADVV", "BDY", "DIFH")


def tracer_engine(rc, data, st, tracers, nproc=(1, 1), extra=None):
    e = engine(rc, data, st, nproc, extra=extra)
    e.set_tracers(len(tracers))
    put_tracers(e, tracers)
    e.put_tracer_nudge(*nudge_tables(rc))
    return e


def put_cumtran(e, inp):
    for name, a in zip(("DOTRAN", "KTOP", "CLDFRA"), inp):
        e.put_cumtran(name, a)


def same_tracers(a, b, ntr, what):
    fa, fb = tracer_fields(a, ntr), tracer_fields(b, ntr)
    for key in fa:
        nd = int((fa[key] != fb[key]).sum())
        assert nd == 0, (what, key, nd)


def mixed(rc, a, inp, ntr):
    """cumtran_ref applied to engine a's tracers: {(level, n): array}."""
    out = {}
    for n in range(1, ntr + 1):
        out[("ATM1", n)], out[("ATM2", n)], _ = cu.cumtran2(rc, a.get_tracer("ATM1", n), a.get_tracer("ATM2", n), *inp)
    return out


def interior_mask(rc):
    m = np.zeros((rc.kz, rc.iy, rc.jx), dtype=bool)
    m[:, 1:rc.iy - 2, 1:rc.jx - 2] = True
    return m


# ------------------------------------------------------------------------------- off by default
@pytest.mark.parametrize("core", ["C", "N"])
def test_off_by_default(core):
    """With tracers declared and nothing switched on the step launches no new kernel, and after both
    switches went on and off again the same names and counts as before; on, the new launches show.
    cumtran on with kcumtop = 0 everywhere leaves every tracer field as with cumtran off."""
    rc, data, st = case(core)
    tracers = patchy_tracers(rc, st, NTR)
    plain, back, on, idle = (tracer_engine(rc, data, st, tracers) for _ in range(4))
    back.set_cumtran(True, 1)
    back.set_tracer_budget(True, 0.5, 0.25)
    back.set_cumtran(False)
    back.set_tracer_budget(False)
    kp, kb = plain.kernel_times(2), back.kernel_times(2)
    assert not any("cumtran" in k or "budget" in k for k in kp), sorted(kp)
    assert {k: v[0] for k, v in kp.items()} == {k: v[0] for k, v in kb.items()}
    on.set_cumtran(True, 1)
    on.set_tracer_budget(True, 0.5, 0.25)
    ko = on.kernel_times(2)
    tend = "k_nh_tr_tend" if rc.idynamic == 2 else "k_tr_tend"
    assert ko["k_tr_cumtran"][0] == 2 and ko[tend + "<budget>"][0] == 2 and tend not in ko and tend in kp
    assert {k: v[0] for k, v in ko.items() if k not in ("k_tr_cumtran", tend + "<budget>")} == \
           {k: v[0] for k, v in kp.items() if k != tend}
    idle.set_cumtran(True, 1)
    dotran, ktop, frc = cu.inputs(rc)
    put_cumtran(idle, (dotran, np.zeros_like(ktop), frc))
    ref = tracer_engine(rc, data, st, tracers)
    for e in (ref, idle):
        e.step(3)
    same_tracers(ref, idle, NTR, "kcumtop = 0")


# ------------------------------------------------------------------------------- cumtran bit for bit
@pytest.mark.parametrize("path", ["pair", "step"])
@pytest.mark.parametrize("core", ["C", "N"])
def test_cumtran_bit_for_bit(core, path):
    """A off, B on with ncum = 2.  Through the tends at lcount 0 and 1 the tracers are equal (0 % 2 == 0
    must not act: rcmtimer%integrating); after the tend at lcount 2, before its bdyval, B's ATM1 / ATM2
    equal cumtran_ref applied to A's on jci x ici and A's everywhere else.  With rcmdyn_step the compare
    comes after bdyval, on the interior (bdyval writes boundary lines only)."""
    rc, data, st = case(core)
    tracers = patchy_tracers(rc, st, NTR)
    inp = cu.inputs(rc)
    a, b = tracer_engine(rc, data, st, tracers), tracer_engine(rc, data, st, tracers)
    b.set_cumtran(True, 2)
    put_cumtran(b, inp)
    for name, x in zip(("DOTRAN", "KTOP", "CLDFRA"), inp):
        assert np.array_equal(b.get_cumtran(name), x.reshape((-1, rc.iy, rc.jx))), name
    m = interior_mask(rc)
    if path == "pair":
        for lcount in (0, 1):
            for e in (a, b):
                assert e.get_time()[0] == lcount
                e.tend()
            same_tracers(a, b, NTR, f"tend at lcount {lcount}")
            for e in (a, b):
                e.bdyval()
        for e in (a, b):
            e.tend()
    else:
        for e in (a, b):
            e.step(2)
        same_tracers(a, b, NTR, "two steps")
        for e in (a, b):
            e.step(1)
    want, got, base = mixed(rc, a, inp, NTR), tracer_fields(b, NTR), tracer_fields(a, NTR)
    changed = 0
    for key in want:
        nd = int((got[key][m] != want[key][m]).sum())
        print(f"cumtran {core} {path} {key}: {nd} interior points differ from cumtran_ref, "
              f"{int((want[key] != base[key]).sum())} mixed")
        assert nd == 0, (key, nd)
        assert np.array_equal(got[key][~m], base[key][~m]), key
        changed += int((want[key] != base[key]).sum())
    assert changed > 1000


# ------------------------------------------------------------------------------- every path
@pytest.mark.parametrize("core", ["C", "N"])
def test_every_path_bit_for_bit(core, monkeypatch):
    """ncum = 2, five steps (cumtran acts at lcount 2 and 4), the budget on: eager launches, the one- and
    two-step graphs, the drop-in pair with its lazy tend and the physics split hold the same tracers and
    the same five sums.  A new KTOP between replays is read by the captured graphs as they are."""
    rc, data, st = case(core)
    tracers = patchy_tracers(rc, st, NTR)
    inp = cu.inputs(rc)

    def start():
        e = tracer_engine(rc, data, st, tracers)
        e.set_cumtran(True, 2)
        e.set_tracer_budget(True, 0.5, 0.25)
        put_cumtran(e, inp)
        return e
    monkeypatch.setenv("RCMDYN_NO_GRAPH", "1")
    eager = start()
    monkeypatch.delenv("RCMDYN_NO_GRAPH")
    graph, pair, split = start(), start(), start()
    eager.step(5)
    graph.step(5)
    for _ in range(5):
        pair.tend()
        pair.bdyval()
        split.tend_pre_physics()
        split.tend_post_physics()
        split.bdyval()

    def sums(e):
        return {(t, n): e.get_tracer_budget(t, n) for t in TRACER_DIAG_TERMS for n in range(1, NTR + 1)}
    se = sums(eager)
    assert all(se[(t, 1)].any() for t in ("ADVH", "ADVV", "DIFH", "CONV"))
    for other, name in ((graph, "graph"), (pair, "pair"), (split, "split")):
        same_tracers(eager, other, NTR, name)
        so = sums(other)
        for key in se:
            assert np.array_equal(se[key], so[key]), (name, key)
    ktop2 = np.where(inp[1] > 0, np.maximum(inp[1] - 2.0, 0.0), float(rc.kz - 3))
    old = start()
    old.step(7)
    for e in (eager, graph):
        e.put_cumtran("KTOP", ktop2)
        e.step(2)                                # the tends at lcount 5 and 6: the second acts
    same_tracers(eager, graph, NTR, "new KTOP")
    assert any(not np.array_equal(old.get_tracer("ATM1", n), graph.get_tracer("ATM1", n)) for n in range(1, NTR + 1))


# ------------------------------------------------------------------------------- decomposition
@pytest.mark.parametrize("transport", ["copy", "rccl"])
@pytest.mark.parametrize("core", ["C", "N"])
def test_decomposition(core, transport, monkeypatch):
    """2 x 2 in-process tiles, halos by device copy and over RCCL to self: after 3 steps with cumtran
    acting in the second and third tend and the budget on, every tracer field and every sum of the
    budget is bit-identical to one tile (smooth tracers: the reference's own negative-value fix
    depends on the decomposition where a negative forecast meets a tile edge)."""
    rc, data, st = case(core)
    tracers = smooth_tracers(rc, st, NTR)
    inp = cu.inputs(rc)
    runs = []
    for nproc in ((1, 1), (2, 2)):
        if nproc != (1, 1) and transport == "rccl":
            monkeypatch.setenv("RCMDYN_FORCE_RCCL", "1")
        e = tracer_engine(rc, data, st, tracers, nproc)
        e.set_cumtran(True, 1)
        e.set_tracer_budget(True, 0.5, 0.25)
        put_cumtran(e, inp)
        e.step(3)
        runs.append((tracer_fields(e, NTR), {(t, n): e.get_tracer_budget(t, n) for t in TRACER_DIAG_TERMS
                                             for n in range(1, NTR + 1)}))
    for part in (0, 1):
        for key in runs[0][part]:
            assert np.array_equal(runs[0][part][key], runs[1][part][key]), key
    assert all(runs[0][1][(t, NTR)].any() for t in ("ADVH", "ADVV", "BDY", "DIFH", "CONV"))


# ------------------------------------------------------------------------------- the budget against the reference
BUDGET_CASES = [("C", {}, NTR), ("N", {}, NTR), ("C", {"iboudy": 3}, 1), ("C", {"idiffu": 2, "iboudy": 1}, 1),
                ("C", {"upstream_mode": 0}, 1), ("C", {"ibltyp": 2, "iuwvadv": 1}, 1), ("C", {}, 1)]


@pytest.mark.parametrize("grid,variant,ntr", BUDGET_CASES, ids=lambda v: variant_id(v) if isinstance(v, dict) else str(v))
def test_budget_against_reference(grid, variant, ntr):
    """ADVH, ADVV, BDY, DIFH after one tend against tests/tracer_diag_ref.py at every cross point, bit for
    bit, with non-zero nudge tables and TR_PHY; the state after the bdyval equals the reference's (the
    budget changes no prognostic result).  iboudy = 3: BDY is exactly + 0.0."""
    rc, data, st = case(grid, **variant)
    tracers = patchy_tracers(rc, st, ntr)
    tables = nudge_tables(rc)
    extra = uw_extra(rc)
    e = engine(rc, data, st, extra=extra)
    e.set_diagnostics(True)           # QDOT and XKC of the tend are read back
    e.set_tracers(ntr)
    put_tracers(e, tracers)
    e.put_tracer_nudge(*tables)
    rw = 1.0 / 7.0
    e.set_tracer_budget(True, rw, 0.25)
    held = dict(st)
    held.update({name: e.get(name) for name in ("ATM1_U", "ATM1_V", "PSA", "PSB", "ATM2_U", "ATM2_V")})
    if rc.idynamic == 2:
        held["ATM2_W"] = e.get("ATM2_W")
    clock0 = e.get_time()
    e.tend()
    clock1 = e.get_time()
    got = {(t, n): e.get_tracer_budget(t, n) for t in TRACER_DIAG_TERMS for n in range(1, ntr + 1)}
    e.bdyval()
    xkc = tr.nh_xkc(rc, held) if rc.idynamic == 2 else e.get("XKC")
    step = td.StepInputs.from_state(rc, held, e.get("QDOT"), xkc, clock0[1], clock0[2] + clock0[1],
                                    clock1[2] + clock1[1], kpbl=extra["KPBL"][0] if "KPBL" in extra else None)
    for n, t in enumerate(tracers):
        terms, res = td.tend_bdyval(rc, step, t["ATM1"], t["ATM2"], t["PHY"], t["B0"], t["BT"], *tables, rw)
        for name in STAGES:
            nd = int((got[(name, n + 1)] != terms[name]).sum())
            print(f"budget {grid} {variant_id(variant)} tracer {n + 1} {name}: {nd} points differ, "
                  f"{int((terms[name] != 0.0).sum())} non-zero")
            assert nd == 0, (n + 1, name, nd)
        assert all(terms[name].any() for name in ("ADVH", "ADVV", "DIFH"))
        bdy = got[("BDY", n + 1)]
        if rc.iboudy == 3:
            assert not bdy.any() and not np.signbit(bdy).any()
        else:
            assert bdy.any()
        assert not got[("CONV", n + 1)].any()                  # cumtran is off
        for lev, want in (("ATM1", res.atm1), ("ATM2", res.atm2)):
            assert np.array_equal(e.get_tracer(lev, n + 1)[:, :rc.iy - 1, :rc.jx - 1], want[:, :rc.iy - 1, :rc.jx - 1])


@pytest.mark.parametrize("core", ["C", "N"])
def test_budget_accumulates_resets_and_scales(core):
    """The sum after two tends equals (the sum after the first) + (the second tend's term, read after a
    reset), bit for bit; a reset gives zeros; a changed rw scales the next term only; the state is
    bit-identical with the budget on and off."""
    rc, data, st = case(core)
    tracers = patchy_tracers(rc, st, NTR)
    off, two, one = (tracer_engine(rc, data, st, tracers) for _ in range(3))
    for e in (two, one):
        e.set_tracer_budget(True, 0.5, 0.25)

    def sums(e):
        return {(t, n): e.get_tracer_budget(t, n) for t in STAGES for n in range(1, NTR + 1)}
    for e in (off, two, one):
        e.tend()
        e.bdyval()
    first = sums(one)
    one.reset_tracer_budget()
    assert not any(v.any() for v in sums(one).values())
    for e in (off, two, one):
        e.tend()
        e.bdyval()
    second, both = sums(one), sums(two)
    for key in both:
        assert np.array_equal(both[key], first[key] + second[key]), key
        assert first[key].any() or key[0] == "BDY"
    same_tracers(off, two, NTR, "budget on")
    same_tracers(off, one, NTR, "budget on, reset")
    # rw: 0.5 -> 2.0 scales the third tend's term by four exactly (a power of two), the held sum not
    keep = sums(two)
    two.set_tracer_budget(True, 2.0, 0.25)
    one.reset_tracer_budget()
    for e in (two, one):
        e.tend()
        e.bdyval()
    third, total = sums(one), sums(two)
    for key in total:
        assert np.array_equal(total[key], keep[key] + 4.0 * third[key]), key


# ------------------------------------------------------------------------------- CONV
@pytest.mark.parametrize("core", ["C", "N"])
def test_conv_term(core):
    """A: the budget on, cumtran off; B: both on, ncum = 2.  CONV stays zero through the tends at lcount 0
    and 1 (on A for good); in the acting tend at lcount 2 it gains cumtran_ref's term of A's ATM2 with the
    tend's dt, at every level of jci x ici, which is also (B's ATM2 - A's) / dt * 2 * cfdout; the next,
    idle, tend leaves it untouched."""
    rc, data, st = case(core)
    tracers = patchy_tracers(rc, st, NTR)
    inp = cu.inputs(rc)
    cfdout = 1.0 / 3.0
    a, b = tracer_engine(rc, data, st, tracers), tracer_engine(rc, data, st, tracers)
    for e in (a, b):
        e.set_tracer_budget(True, 0.5, cfdout)
    b.set_cumtran(True, 2)
    put_cumtran(b, inp)
    for e in (a, b):
        e.step(2)
    for n in range(1, NTR + 1):
        assert not b.get_tracer_budget("CONV", n).any(), n
    dt = b.get_time()[1]
    for e in (a, b):
        e.tend()
    held = {}
    for n in range(1, NTR + 1):
        a2 = a.get_tracer("ATM2", n)
        _, bn, conv = cu.cumtran2(rc, a.get_tracer("ATM1", n), a2, *inp, dt=dt, cfdout=cfdout)
        got = b.get_tracer_budget("CONV", n)
        nd = int((got != conv).sum())
        print(f"conv {core} tracer {n}: {nd} points differ, {int((conv != 0.0).sum())} non-zero, dt = {dt}")
        assert nd == 0 and conv.any(), (n, nd)
        m = interior_mask(rc)
        assert np.array_equal(got[m], ((b.get_tracer("ATM2", n) - a2) / dt * 2.0 * cfdout)[m]), n
        assert not a.get_tracer_budget("CONV", n).any(), n
        held[n] = got
    b.bdyval()
    b.tend()                                         # lcount 3: idle
    for n in range(1, NTR + 1):
        assert np.array_equal(b.get_tracer_budget("CONV", n), held[n]), n


# ------------------------------------------------------------------------------- refusals
def test_refusals():
    """Every refusal names its argument and leaves the engine usable."""
    from regcm_amd.dycore import EngineError
    rc, data, st = case("C")
    z2, z3 = np.zeros((rc.iy, rc.jx)), np.zeros((rc.kz, rc.iy, rc.jx))
    e = engine(rc, data, st)
    for call in (lambda: e.set_cumtran(True, 1), lambda: e.set_tracer_budget(True, 1.0, 1.0)):
        with pytest.raises(EngineError, match="no tracers are declared"):
            call()
    for call in (lambda: e.put_cumtran("KTOP", z2), lambda: e.get_cumtran("KTOP")):
        with pytest.raises(EngineError, match="cumtran is off"):
            call()
    for call in (lambda: e.get_tracer_budget("ADVH", 1), e.reset_tracer_budget):
        with pytest.raises(EngineError, match="tracer budget is off"):
            call()
    e.set_tracers(2)
    with pytest.raises(EngineError, match="ncum"):
        e.set_cumtran(True, 0)
    with pytest.raises(EngineError, match="cumtran is off"):
        e.put_cumtran("KTOP", z2)
    for rw, cf, msg in ((np.nan, 1.0, "rw"), (np.inf, 1.0, "rw"), (1.0, np.nan, "cfdout")):
        with pytest.raises(EngineError, match=msg):
            e.set_tracer_budget(True, rw, cf)
    with pytest.raises(EngineError, match="tracer budget is off"):
        e.get_tracer_budget("ADVH", 1)
    e.set_cumtran(True, 3)
    e.set_tracer_budget(True, 1.0, 1.0)
    for bad in (2.5, -1.0, rc.kz + 1.0, np.nan):
        k = z2.copy()
        k[5, 7] = bad
        with pytest.raises(EngineError, match="CUM_KTOP"):
            e.put_cumtran("KTOP", k)
    for bad in (1.5, np.nan, -0.25):
        f = z3.copy()
        f[3, 5, 7] = bad
        with pytest.raises(EngineError, match="CUM_CLDFRA"):
            e.put_cumtran("CLDFRA", f)
    d = z2.copy()
    d[5, 7] = 2.0
    with pytest.raises(EngineError, match="CUM_DOTRAN"):
        e.put_cumtran("DOTRAN", d)
    assert not e.get_cumtran("KTOP").any() and not e.get_cumtran("DOTRAN").any()      # a refused put wrote nothing
    for call in (lambda: e.put_cumtran(7, z2), lambda: e.get_cumtran(-1)):
        with pytest.raises(EngineError, match="unknown cumtran field"):
            call()
    with pytest.raises(EngineError, match="unknown budget term"):
        e.get_tracer_budget(5, 1)
    for itr in (0, 3):
        with pytest.raises(EngineError, match="itr"):
            e.get_tracer_budget("ADVH", itr)
    e.step(1)                                          # still usable
    for count in (3, 0):
        e.set_cumtran(True, 3)
        e.set_tracer_budget(True, 1.0, 1.0)
        e.set_tracers(count)                           # another count: both features are off
        with pytest.raises(EngineError, match="cumtran is off"):
            e.put_cumtran("KTOP", z2)
        with pytest.raises(EngineError, match="tracer budget is off"):
            e.get_tracer_budget("ADVH", 1)
        e.step(1)
        assert not any("cumtran" in k or "budget" in k for k in e.kernel_times(1))


# ------------------------------------------------------------------------------- a Fortran host
DRIVER = r"""
program tracer_diag_host
  use iso_c_binding
  use mod_gpu_dyn
  implicit none
  type(rcmdyn_config) :: cfg
  type(c_ptr) :: h
  integer :: u, nf, q, f, nk, jx, iy, kz, itr, term
  real(c_double), allocatable :: a(:)
  real(c_double) :: fac(2)
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
  read(u) fac
  call gpu_dyn_check(h, rcmdyn_set_cumtran(h, 1, 2), 'set_cumtran')
  call gpu_dyn_check(h, rcmdyn_set_tracer_budget(h, 1, fac(1), fac(2)), 'set_tracer_budget')
  read(u) a(1:jx*iy)
  call gpu_dyn_check(h, rcmdyn_put_cumtran(h, cum_dotran, a, 1, jx, 1, iy, 1, 1), 'put dotran')
  read(u) a(1:jx*iy)
  call gpu_dyn_check(h, rcmdyn_put_cumtran(h, cum_ktop, a, 1, jx, 1, iy, 1, 1), 'put ktop')
  read(u) a
  call gpu_dyn_check(h, rcmdyn_put_cumtran(h, cum_cldfra, a, 1, jx, 1, iy, 1, kz), 'put cldfra')
  close(u)
  call gpu_dyn_check(h, rcmdyn_step(h, 3), 'step')
  open(newunit=u, file=trim(dir)//'/out.bin', access='stream', form='unformatted', status='replace')
  do itr = 1, 2
    do term = trdiag_advh, trdiag_conv
      call gpu_dyn_check(h, rcmdyn_get_tracer_budget(h, term, itr, a, 1, jx, 1, iy, 1, kz), 'get_tracer_budget')
      write(u) a
    end do
    do f = tr_atm1, tr_atm2
      call gpu_dyn_check(h, rcmdyn_get_tracer(h, f, itr, a, 1, jx, 1, iy, 1, kz), 'get_tracer')
      write(u) a
    end do
  end do
  call gpu_dyn_check(h, rcmdyn_get_cumtran(h, cum_ktop, a, 1, jx, 1, iy, 1, 1), 'get ktop')
  write(u) a(1:jx*iy)
  call gpu_dyn_check(h, rcmdyn_reset_tracer_budget(h), 'reset')
  close(u)
  call gpu_dyn_check(h, rcmdyn_destroy(h), 'destroy')
end program tracer_diag_host
"""


def test_fortran_host(tmp_path):
    """A Fortran host through mod_gpu_dyn sets both switches, puts the three inputs, steps past the acting
    tend at lcount 2 and reads the five terms: bit-identical to the Python host."""
    import ctypes
    from regcm_amd.config import FIELD, build_config, field_levels
    rc, data, st = case("C")
    tracers = smooth_tracers(rc, st, 2)
    inp = cu.inputs(rc)
    fac = (1.0 / 7.0, 1.0 / 3.0)
    fdir = os.path.join(ROOT, "regcm_amd", "fortran")
    src = tmp_path / "tracer_diag_host.f90"
    src.write_text(DRIVER)
    exe = tmp_path / "tracer_diag_host"
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
        fh.write(np.array(fac, dtype=np.float64).tobytes())
        for a in inp:
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    subprocess.run([str(exe), str(tmp_path)], check=True)
    raw = np.fromfile(tmp_path / "out.bin")
    n3 = rc.kz * rc.iy * rc.jx
    out = raw[:2 * 7 * n3].reshape(2, 7, rc.kz, rc.iy, rc.jx)
    assert np.array_equal(raw[2 * 7 * n3:].reshape(rc.iy, rc.jx), inp[1])
    e = engine(rc, data, st)
    e.set_tracers(2)
    put_tracers(e, tracers)
    e.set_cumtran(True, 2)
    e.set_tracer_budget(True, *fac)
    put_cumtran(e, inp)
    e.step(3)
    for n in range(2):
        for q, term in enumerate(TRACER_DIAG_TERMS):
            assert np.array_equal(out[n, q], e.get_tracer_budget(term, n + 1)), (n + 1, term)
            assert out[n, q].any() or term == "BDY", (n + 1, term)
        for q, lev in enumerate(("ATM1", "ATM2")):
            assert np.array_equal(out[n, 5 + q], e.get_tracer(lev, n + 1)), (n + 1, lev)
