"""GPU tests of the tracers' device output stream (rcmdyn_set_output_che / rcmdyn_output_che /
rcmdyn_get_output_che, regcm_amd/csrc/che_output.hip): the CHE file's dyn-owned fields against
tests/che_output_ref.py, the NumPy transcription of the Fortran lines (the oracle has no tracers and
no output), applied to the state the engine itself returns through the existing gets.

Every field is + - * / only, so every comparison is bit for bit, at every interior cross point.
All cases run on the 37 x 29 x 18 cuts case("C") / case("N") (odd, no multiple of the wave or the
block) and the band case("C1", i_band=1), with ntr = 4 patchy tracers (two groups, 3 + 1), non-zero
nudging tables and cumtran on with ncum = 2, so that CONV is non-zero after the tend at lcount 2.
On the NH core atms%dzq is the constant atm0%dzf (Main/mod_atm_interface.F90:977), which the
transcription takes from ATM0_ZF (rcmdyn_get serves no ATMS_DZQ there).  The tile tests use smooth
tracers, as tests/test_tracer_diag_gpu.py's do: the reference's own negative-value fix depends on the
decomposition where a negative forecast meets a tile edge.
"""
import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from regcm_amd.config import CHE_FIELD, CHE_FIELDS, TRACER_DIAG_TERMS, TRACER_FIELD
from tests import che_output_ref as cr
from tests import cumtran_ref as cu
from tests.output_ref import interior
from tests.support import advance, case, engine, state_names
from tests.test_fortran_shim import BDYVAL, CREATE, EXE, POST, PRE, PUT, STEP, Script
from tests.test_tracers_gpu import nudge_tables, patchy_tracers, put_tracers, smooth_tracers, tracer_fields

pytestmark = pytest.mark.gpu

NTR = 4
ALL = list(CHE_FIELDS)
STATE_ONLY = ["MIXRAT", "BURDEN"]
CASES = {"C": lambda: case("C"), "N": lambda: case("N"), "band": lambda: case("C1", i_band=1)}


def che_engine(rc, data, st, tracers, nproc=(1, 1), budget=True, prec=8, nbatch=NTR, stage=True):
    """An engine with the tracers, the nudging tables, cumtran (ncum = 2), the budget and the stage."""
    e = engine(rc, data, st, nproc)
    e.set_tracers(len(tracers))
    put_tracers(e, tracers)
    e.put_tracer_nudge(*nudge_tables(rc))
    e.set_cumtran(True, 2)
    for name, a in zip(("DOTRAN", "KTOP", "CLDFRA"), cu.inputs(rc)):
        e.put_cumtran(name, a)
    if budget:
        e.set_tracer_budget(True, 0.5, 0.25)
    if stage:
        e.set_output_che(True, prec, nbatch)
    return e


def start(name, **kw):
    rc, data, st = CASES[name]()
    return rc, che_engine(rc, data, st, patchy_tracers(rc, st, NTR), **kw)


def run(e, path, nsteps=2):
    """One step by the physics seam (the slice exists from it on), then nsteps on the path."""
    advance(e, "physics", 1)
    advance(e, path, nsteps)


def sums_of(e, itrs=range(1, NTR + 1)):
    return {(t, n): e.get_tracer_budget(t, n) for t in TRACER_DIAG_TERMS for n in itrs}


def transcription(e, rc, itrs, names=ALL):
    """{(field, itr)}: the Fortran lines applied to what the existing gets return now."""
    cpsb = e.get("PSB")
    out = {}
    if "BURDEN" in names:
        dzq = cr.nh_dzq(e.get("ATM0_ZF")) if rc.idynamic == 2 else e.get("ATMS_DZQ")
        rhob = e.get("ATMS_RHOB3D")
    for n in itrs:
        if "MIXRAT" in names:
            out[("MIXRAT", n)] = cr.mixrat(rc, e.get_tracer("ATM1", n), cpsb)
        if "BURDEN" in names:
            out[("BURDEN", n)] = cr.burden(rc, e.get_tracer("CHIB3D", n), dzq, rhob)
        for t in cr.TERMS:
            if t in names:
                out[(t, n)] = cr.term(rc, e.get_tracer_budget(t, n), cpsb)
    return out


def fetch(e, names, itr1, itr2):
    e.output_che(names, itr1, itr2)
    return {(f, n): e.get_output_che(f, n) for f in names for n in range(itr1, itr2 + 1)}


def same(got, ref):
    assert sorted(got) == sorted(ref)
    for key in ref:
        a, b = got[key], ref[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        nd = int((a != b).sum())
        print(f"{key}: {nd} points differ, max |a - b| = {float(np.max(np.abs(a - b))):.3e}")
        assert np.array_equal(a, b), (key, nd)


# ------------------------------------------------------------------------------- values
@pytest.mark.parametrize("path", ["step", "pair", "physics"])
@pytest.mark.parametrize("name", list(CASES))
def test_fields_match_the_transcription(name, path):
    """Every field of every tracer equals the transcription bit for bit at every interior cross point
    after one physics-split step plus two more on the path, and is non-constant on the interior."""
    rc, e = start(name)
    run(e, path)
    ref = transcription(e, rc, range(1, NTR + 1))
    same(fetch(e, ALL, 1, NTR), ref)
    is_, js = interior(rc)
    for key, b in ref.items():
        assert np.unique(b[:, is_, js]).size > 1, key
        outside = np.ones(b.shape, dtype=bool)
        outside[:, is_, js] = False
        assert not b[outside].any(), key


@pytest.mark.parametrize("name", ["C", "N"])
def test_burden_is_a_leftover(name):
    """New tracers put after the split step: BURDEN is still the column sum of the old CHIB3D, MIXRAT
    follows the new state."""
    rc, e = start(name, budget=False)
    advance(e, "physics", 1)
    old = transcription(e, rc, range(1, NTR + 1), STATE_ONLY)
    st = CASES[name]()[2]
    put_tracers(e, [{k: 1.5 * v for k, v in t.items()} for t in patchy_tracers(rc, st, NTR, seed=9)])
    new = transcription(e, rc, range(1, NTR + 1), STATE_ONLY)
    got = fetch(e, STATE_ONLY, 1, NTR)
    same(got, new)
    for n in range(1, NTR + 1):
        assert np.array_equal(new[("BURDEN", n)], old[("BURDEN", n)])
        assert not np.array_equal(new[("MIXRAT", n)], old[("MIXRAT", n)])
    e.tend_pre_physics()                          # mkslice of the new tracers
    assert not np.array_equal(transcription(e, rc, [1], ["BURDEN"])[("BURDEN", 1)], old[("BURDEN", 1)])


# ------------------------------------------------------------------------------- read-and-zero
@pytest.mark.parametrize("mask", [ALL, ["MIXRAT"]], ids=["all", "mixrat-only"])
@pytest.mark.parametrize("name", ["C", "N"])
def test_read_and_zero(name, mask):
    """output_che(mask, 2, 3) with the budget on: all five sums of tracers 2 and 3 are exactly + 0.0,
    whatever the mask; those of 1 and 4 keep their bits; after two more steps the sums of tracer 2
    equal those of a twin that called reset_tracer_budget at the same point."""
    rc, e = start(name)
    _, twin = start(name, stage=False)
    for x in (e, twin):
        run(x, "step")
    before = sums_of(e)
    assert all(before[(t, n)].any() for t in ("ADVH", "ADVV", "DIFH", "CONV") for n in range(1, NTR + 1))
    e.output_che(mask, 2, 3)
    after = sums_of(e)
    for (t, n), a in after.items():
        if n in (2, 3):
            assert not a.any() and not np.signbit(a).any(), (t, n)
        else:
            assert np.array_equal(a.view(np.uint64), before[(t, n)].view(np.uint64)), (t, n)
    twin.reset_tracer_budget()
    for x in (e, twin):
        x.step(2)
    se, st = sums_of(e, [2]), sums_of(twin, [2])
    for key in se:
        assert np.array_equal(se[key], st[key]) and (se[key].any() or key[0] == "BDY"), key


@pytest.mark.parametrize("name", ["C", "N"])
def test_budget_off_changes_nothing(name):
    """With the budget off a MIXRAT-only call changes no tracer field; switched on afterwards the sums
    start from zero as on an engine that never made the call."""
    rc, e = start(name, budget=False)
    _, twin = start(name, budget=False, stage=False)
    for x in (e, twin):
        run(x, "step")
    before = tracer_fields(e, NTR)
    got = fetch(e, ["MIXRAT"], 1, NTR)
    assert all(a.any() for a in got.values())
    after = tracer_fields(e, NTR)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    for x in (e, twin):
        x.set_tracer_budget(True, 0.5, 0.25)
        x.step(2)
    se, st = sums_of(e), sums_of(twin)
    for key in se:
        assert np.array_equal(se[key], st[key]), key


# ------------------------------------------------------------------------------- fp32
@pytest.mark.parametrize("name", ["C", "N"])
def test_fp32_is_one_rounding_of_fp64(name):
    """Two engines from one state, prec 8 and prec 4 (a call zeroes the sums it reads)."""
    rc, d = start(name, prec=8)
    _, f = start(name, prec=4)
    for x in (d, f):
        run(x, "step")
    gd, gf = fetch(d, ALL, 1, NTR), fetch(f, ALL, 1, NTR)
    for key in gd:
        assert gf[key].dtype == np.float32 and gd[key].dtype == np.float64, key
        assert np.array_equal(gf[key].view(np.uint32), gd[key].astype(np.float32).view(np.uint32)), key
        assert gf[key].any(), key


# ------------------------------------------------------------------------------- two slots
@pytest.mark.parametrize("name", ["C", "N"])
def test_two_slots_hold_the_state_of_their_calls(name):
    """nbatch = 2: output_che(1, 2), a step, output_che(3, 4), step(3), then the gets: each batch is the
    transcription of the state at its own call.  A third call takes the first one's place."""
    from regcm_amd.dycore import EngineError
    rc, e = start(name, nbatch=2)
    run(e, "step")
    ref = transcription(e, rc, [1, 2])
    e.output_che(ALL, 1, 2)
    e.step(1)
    ref.update(transcription(e, rc, [3, 4]))
    e.output_che(ALL, 3, 4)
    e.step(3)
    got = {(f, n): e.get_output_che(f, n) for f in ALL for n in range(1, NTR + 1)}
    same(got, ref)
    later = transcription(e, rc, [1], ["MIXRAT"])
    assert not np.array_equal(later[("MIXRAT", 1)], ref[("MIXRAT", 1)])
    ref3 = transcription(e, rc, [3], ["MIXRAT"])
    e.output_che(["MIXRAT"], 3, 3)                 # takes the slot of the first call
    with pytest.raises(EngineError, match="CHE_MIXRAT of tracer 1 is in neither of the two held snapshots"):
        e.get_output_che("MIXRAT", 1)
    with pytest.raises(EngineError, match="CHE_ADVH of tracer 2 is in neither"):
        e.get_output_che("ADVH", 2)
    assert np.array_equal(e.get_output_che("MIXRAT", 3), ref3[("MIXRAT", 3)])     # the newer of the two
    assert np.array_equal(e.get_output_che("MIXRAT", 4), ref[("MIXRAT", 4)])
    assert np.array_equal(e.get_output_che("ADVH", 3), ref[("ADVH", 3)])          # only the older has it


# ------------------------------------------------------------------------------- passivity
@pytest.mark.parametrize("name", ["C", "N"])
def test_stage_is_passive(name):
    """With the stage on and used every step (budget off) the state and the tracers after 5 steps are
    those of an engine without it; with the stage off the profile of a step lists the same kernel
    names and counts, and no launch of the stage."""
    rc, a = start(name, budget=False, stage=False)
    _, b = start(name, budget=False, prec=4, nbatch=3)
    for q in range(5):
        for e in (a, b):
            advance(e, ("physics", "step", "pair")[q % 3], 1)
        b.output_che(STATE_ONLY, 1 + q % 2, 3 + q % 2)
        if q % 2:
            b.get_output_che("BURDEN", 2)
    for n in state_names(rc):
        assert np.array_equal(a.get(n), b.get(n)), n
    fa, fb = tracer_fields(a, NTR), tracer_fields(b, NTR)
    for key in fa:
        assert np.array_equal(fa[key], fb[key]), key
    assert a.get_time() == b.get_time()
    b.set_output_che(False)
    ka, kb = a.kernel_times(2), b.kernel_times(2)
    assert {k: v[0] for k, v in ka.items()} == {k: v[0] for k, v in kb.items()}
    assert not any("k_output_che" in k for k in ka)


# ------------------------------------------------------------------------------- tiles
def tiled_pair(name):
    rc, data, st = CASES[name]()
    tracers = smooth_tracers(rc, st, NTR)
    out = []
    for nproc in ((1, 1), (2, 2)):
        e = che_engine(rc, data, st, tracers, nproc=nproc, nbatch=3)
        run(e, "step")
        got = fetch(e, ALL, 1, 3)
        got.update(fetch(e, ALL, 4, 4))
        out.append(got)
    return out


@pytest.mark.parametrize("transport", ["copy", "rccl"])
@pytest.mark.parametrize("name", ["C", "N"])
def test_tiles_equal_one_tile(name, transport, monkeypatch):
    """2 x 2 tiles, halos by device copy and as RCCL sends and receives (the self-communicator): every
    field of every tracer as on one tile."""
    if transport == "rccl":
        monkeypatch.setenv("RCMDYN_FORCE_RCCL", "1")
    one, four = tiled_pair(name)
    same(four, one)
    assert all(one[(f, 1)].any() for f in ("MIXRAT", "BURDEN", "ADVH", "ADVV", "DIFH", "CONV"))


# ------------------------------------------------------------------------------- refusals
def test_refusals():
    """Each refused call names its cause, launches nothing (the sums keep their bits) and leaves the
    engine usable."""
    from regcm_amd.dycore import EngineError
    rc, data, st = CASES["C"]()

    def refused(match, fn, *a):
        with pytest.raises(EngineError, match=match):
            fn(*a)

    bare = engine(rc, data, st)
    refused("rcmdyn_set_output_che: no tracers are declared", bare.set_output_che, True, 8, 1)
    refused("CHE output stage is off", bare.output_che, ["MIXRAT"], 1, 1)
    e = che_engine(rc, data, st, patchy_tracers(rc, st, NTR), budget=False, stage=False)
    e.step(1)
    refused("CHE output stage is off", e.output_che, ["MIXRAT"], 1, 1)
    refused("CHE output stage is off", e.get_output_che, "MIXRAT", 1)
    refused("prec = 2", e.set_output_che, True, 2, 1)
    refused("nbatch = 0", e.set_output_che, True, 8, 0)
    refused("nbatch = 5 must lie in 1 .. ntr = 4", e.set_output_che, True, 8, NTR + 1)
    refused("CHE output stage is off", e.output_che, ["MIXRAT"], 1, 1)             # the refused switches left it off
    e.set_output_che(True, 8, 2)
    refused("CHE_MIXRAT of tracer 1 is in neither", e.get_output_che, "MIXRAT", 1)   # no snapshot yet
    refused("mask = 0", e.output_che, [], 1, 1)
    refused("bit beyond the last field \\(6\\)", e.output_che, 1 << 7, 1, 1)
    refused("unknown field 7", e.get_output_che, 7, 1)
    refused("itr1 = 0", e.output_che, ["MIXRAT"], 0, 1)
    refused("itr2 = 5 must satisfy .* ntr = 4", e.output_che, ["MIXRAT"], 4, 5)
    refused("itr1 = 3, itr2 = 2", e.output_che, ["MIXRAT"], 3, 2)
    refused("holds 3 tracers, more than nbatch = 2", e.output_che, ["MIXRAT"], 1, 3)
    for t in cr.TERMS:
        refused(f"CHE_{t}: the tracer budget is off", e.output_che, ["MIXRAT", t], 1, 2)
    refused("CHE_BURDEN: no slice fields yet", e.output_che, ["BURDEN"], 1, 1)
    e.output_che(["MIXRAT"], 1, 2)
    refused("CHE_MIXRAT of tracer 3 is in neither", e.get_output_che, "MIXRAT", 3)
    refused("CHE_BURDEN of tracer 1 is in neither", e.get_output_che, "BURDEN", 1)
    assert e.get_output_che("MIXRAT", 2).shape == (rc.kz, rc.iy, rc.jx)
    e.set_tracer_budget(True, 0.5, 0.25)
    advance(e, "physics", 1)
    before = sums_of(e)
    refused("itr1 = 0", e.output_che, ALL, 0, 1)
    refused("bit beyond", e.output_che, 1 << 9, 1, 2)
    after = sums_of(e)
    for key in before:
        assert np.array_equal(before[key], after[key]) and (before[key].any() or key[0] in ("BDY", "CONV")), key
    assert np.any(e.get_output_che("MIXRAT", 1) != 0.0)                     # a refused call keeps the snapshots
    e.output_che(["BURDEN"], 1, 1)
    assert e.get_output_che("BURDEN", 1).shape == (1, rc.iy, rc.jx)
    e.set_output_che(True, 8, 3)                                            # a changed nbatch forgets both
    refused("CHE_MIXRAT of tracer 1 is in neither", e.get_output_che, "MIXRAT", 1)
    e.set_tracers(2)                                                        # another count: the stage goes off
    refused("CHE output stage is off", e.output_che, ["MIXRAT"], 1, 1)
    put_tracers(e, patchy_tracers(rc, st, 2))
    e.set_output_che(True, 4, 2)
    e.step(1)
    assert fetch(e, ["MIXRAT"], 1, 2)[("MIXRAT", 2)].dtype == np.float32


# ------------------------------------------------------------------------------- Fortran host
class CheScript(Script):
    """The shim test's script with the tracer and CHE output calls (ops 31-36 of test_shim.F90)."""
    SET_TRACERS, PUT_TRACER, SET_TRBUDGET, SET_CHE, OUTPUT_CHE, GET_CHE = range(31, 37)

    def put_tracer(self, name, itr, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        nk, ni, nj = a.shape
        return self.add(self.PUT_TRACER, TRACER_FIELD[name], itr, 1, nj, 1, ni, 1, nk, a)

    def run_python(self):
        from regcm_amd.dycore import lib
        L, h, out = lib(), ctypes.c_void_p(), []
        dp = ctypes.POINTER(ctypes.c_double)
        plain = {BDYVAL: L.rcmdyn_bdyval, PRE: L.rcmdyn_tend_pre_physics, POST: L.rcmdyn_tend_post_physics}
        ints = {STEP: L.rcmdyn_step, self.SET_TRACERS: L.rcmdyn_set_tracers, self.SET_TRBUDGET: L.rcmdyn_set_tracer_budget,
                self.SET_CHE: L.rcmdyn_set_output_che, self.OUTPUT_CHE: L.rcmdyn_output_che}
        for code, a in self.ops:
            if code == CREATE:
                rc = L.rcmdyn_create(ctypes.byref(self.cfg), ctypes.byref(h))
            elif code == PUT:
                rc = L.rcmdyn_put(h, a[1], a[8].ctypes.data_as(dp), *a[2:8])
            elif code == self.PUT_TRACER:
                rc = L.rcmdyn_put_tracer(h, a[0], a[1], a[8].ctypes.data_as(dp), *a[2:8])
            elif code in plain:
                rc = plain[code](h)
            elif code in ints:
                rc = ints[code](h, *a)
            elif code == self.GET_CHE:
                f, itr, prec, j1, j2, i1, i2, k1, k2 = a
                buf = np.zeros((k2 - k1 + 1, i2 - i1 + 1, j2 - j1 + 1), dtype=np.float32 if prec == 4 else np.float64)
                rc = L.rcmdyn_get_output_che(h, f, itr, buf.ctypes.data_as(ctypes.c_void_p), j1, j2, i1, i2, k1, k2)
                out.append(buf.tobytes())
            else:
                raise ValueError(code)
            assert rc == 0, (code, L.rcmdyn_last_error(h if h.value else None).decode())
        L.rcmdyn_destroy(h)
        return out

    def run_fortran(self, timeout=300):
        subprocess.run(["make", "-s", "-C", os.path.dirname(EXE)], check=True)
        with tempfile.TemporaryDirectory() as d:
            fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(fin, "wb") as f:
                raw = bytes(self.cfg)
                f.write(struct.pack("<i", len(raw)) + raw)
                for code, a in self.ops:
                    f.write(struct.pack("<i", code))
                    if code in (PUT, self.PUT_TRACER):
                        f.write(struct.pack("<8i", *a[:8]) + a[8].tobytes())
                    elif code == self.SET_TRBUDGET:
                        f.write(struct.pack("<idd", *a))
                    elif a:
                        f.write(struct.pack(f"<{len(a)}i", *a))
                f.write(struct.pack("<i", 0))
            subprocess.run([EXE, fin, fout], check=True, timeout=timeout)
            buf = open(fout, "rb").read()
        out, pos = [], 0
        for code, a in self.ops:
            if code == self.GET_CHE:
                n = a[2] * (a[4] - a[3] + 1) * (a[6] - a[5] + 1) * (a[8] - a[7] + 1)
                out.append(buf[pos:pos + n])
                pos += n
        assert pos == len(buf)
        return out


@pytest.mark.parametrize("prec", [4, 8])
def test_fortran_host_gets_the_python_hosts_bytes(prec):
    """A Fortran host through the shim (mod_gpu_dyn's three bindings): the same script, the same bytes,
    two batches in the two slots."""
    from regcm_amd.config import build_config
    rc, data, st = CASES["C"]()
    s = CheScript(build_config(rc, data["split"]))
    s.add(CREATE)
    for n, a in st.items():
        s.put(n, a)
    s.add(BDYVAL).add(s.SET_TRACERS, NTR, 1)
    for q, t in enumerate(patchy_tracers(rc, st, NTR)):
        for name, a in t.items():
            s.put_tracer(name, q + 1, a)
    s.add(s.SET_TRBUDGET, 1, 0.5, 0.25).add(s.SET_CHE, 1, prec, 2)
    s.add(PRE).add(POST).add(BDYVAL).add(STEP, 2)
    mask = (1 << len(CHE_FIELDS)) - 1
    s.add(s.OUTPUT_CHE, mask, 1, 2).add(s.OUTPUT_CHE, mask, 3, 4).add(STEP, 1)
    keys = [(f, n) for n in range(1, NTR + 1) for f in CHE_FIELDS]
    for f, n in keys:
        s.add(s.GET_CHE, CHE_FIELD[f], n, prec, 1, rc.jx, 1, rc.iy, 1, 1 if f == "BURDEN" else rc.kz)
    py, fo = s.run_python(), s.run_fortran()
    assert len(py) == len(fo) == len(keys)
    for key, a, b in zip(keys, py, fo):
        assert a == b, key
        assert any(a) or key[0] in ("BDY", "CONV"), key         # (the script puts no tables and no cumtran)
