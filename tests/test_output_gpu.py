"""GPU tests of the device output stream (rcmdyn_set_output / rcmdyn_output_atm / rcmdyn_get_output,
regcm_amd/csrc/output.hip): the dyn-owned fields of mod_output's ATM, SRF and SHF streams against
tests/output_ref.py, the NumPy transcription of the Fortran lines (the oracle has no output).

Tolerances.  A field with only + - * / (and RH, whose pfwsat is a polynomial) equals the
transcription bit for bit at every interior cross point.  ZH and the 100 m winds carry a log: 1e-13
relative max-norm, the OCML-against-libm figure of tests/test_physics_seam_gpu.py; the level search
of the 100 m winds is discrete, so the test first shows on the reference that no interface height
lies within 1e-10 relative of 100 m.  fp32, tiles, ordering and passivity are bit-exact.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from regcm_amd import icbc
from regcm_amd.config import OUTPUT_FIELD, OUTPUT_FIELDS
from tests import output_ref
from tests.support import advance, case, engine, state_names
from tests.test_fortran_shim import BDYVAL, CREATE, EXE, POST, PRE, PUT, STEP, Script

pytestmark = pytest.mark.gpu

LOG_BEARING = ("ZH", "UA100", "VA100")
LEFTOVER = ("RH", "PF", "ZF", "ZH")
CASES = {
    "C": lambda: case("C"),
    "N": lambda: case("N"),
    "band": lambda: case("C1", i_band=1),          # the band of tests/test_band_gpu.py
    "CRM": lambda: case("CRM"),
    "nqx5": lambda: case("C", ipptls=2),
    "uw": lambda: case("C", ibltyp=2),
}


def cloudy(name):
    """The case with patchy cloud water where its state has none (QC would be constant)."""
    rc, data, st = CASES[name]()
    if not np.any(st["ATM1_QC"]):
        st = dict(st)
        st.update(icbc.hydrometeor_state(rc, st, nqx=2))
    return rc, data, st


def names_of(rc, slice_=True, diag=True):
    """The fields an engine of this configuration serves, once it has a slice / with diagnostics."""
    nh = rc.idynamic == 2
    out = []
    for n in OUTPUT_FIELDS:
        if (n in ("W", "PP") and not nh) or (n in ("ZH", "ZF") and nh) or (n in ("QI", "QR", "QS") and rc.nqx <= 2):
            continue
        if (n == "TKE" and rc.ibltyp != 2) or (n in LEFTOVER and not slice_) or (n == "OMEGA" and (nh or not diag)):
            continue
        out.append(n)
    return out


def state_of(e, rc):
    """The current state as rcmdyn_get returns it: what output_ref reads."""
    names = ["PSA", "ATM1_T", "ATM1_U", "ATM1_V", "ATM1_QV", "ATM1_QC"]
    if rc.idynamic == 2:
        names += ["ATM1_PP", "ATM1_W", "ATM0_PS", "ATM0_PF", "ATM0_Z"]
    if rc.nqx > 2:
        names += ["ATM1_QI", "ATM1_QR", "ATM1_QS"]
    if rc.ibltyp == 2:
        names += ["ATM1_TKE"]
    return {n: e.get(n) for n in names}


def pre_of(e, rc):
    """What atm1%pr of the coming tend is formed from."""
    names = ["PSA"] + (["ATM1_PP", "ATM0_PR"] if rc.idynamic == 2 else [])
    return {n: e.get(n) for n in names}


def leftovers(e, rc, pre, diag=True):
    left = {"PR": output_ref.atm1_pr(rc, rc.sigma, pre), "ATMS_PF3D": e.get("ATMS_PF3D")}
    if rc.idynamic != 2:
        left["ATMS_ZQ"] = e.get("ATMS_ZQ")
    if diag and rc.idynamic != 2:
        left["OMEGA"] = e.get("OMEGA")
    return left


def split_step(e, rc):
    """One step by the physics seam; returns the pre-step fields atm1%pr is formed from."""
    pre = pre_of(e, rc)
    advance(e, "physics", 1)
    return pre


def run(e, rc, path, nsteps):
    """One split-path step (the slice exists from it on), then nsteps on the path; returns the
    pre-step fields of the last split-path step."""
    pre = split_step(e, rc)
    if path == "physics":
        for _ in range(nsteps):
            pre = split_step(e, rc)
    else:
        advance(e, path, nsteps)
    return pre


def fetch(e, names):
    e.output_atm(names)
    return {n: e.get_output(n) for n in names}


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def hold(got, ref, rc, names):
    """Every field against the transcription: bit for bit, the log-bearing ones within 1e-13; each
    one non-constant on the interior."""
    is_, js = output_ref.interior(rc)
    if "UA100" in names:
        z = ref["_Z100"][0]
        assert np.nanmin(np.abs(z - 100.0) / 100.0) > 1e-10          # the level search is not on a knife edge
    for n in names:
        a, b = got[n], ref[n]
        assert a.shape == b.shape and a.dtype == np.float64, n
        print(f"{n}: relmax {relmax(a, b):.3e}")
        if n in LOG_BEARING:
            assert relmax(a, b) < 1e-13, (n, relmax(a, b))
        else:
            assert np.array_equal(a, b), (n, relmax(a, b))
        # (p* of the NH core is atm0%ps, a constant of the run, and the CRM domain is flat)
        assert np.unique(b[:, is_, js]).size > 1 or (n == "PS" and rc.i_crm == 1), n


@pytest.mark.parametrize("path", ["step", "pair", "physics"])
@pytest.mark.parametrize("name", list(CASES))
def test_fields_match_the_transcription(name, path):
    """Tests 1-3 of the issue: the pointwise fields and RH bit for bit, ZH and the 100 m winds within
    the log's bound, after 3 steps on each path, at every interior cross point."""
    rc, data, st = cloudy(name)
    e = engine(rc, data, st)
    e.set_diagnostics(True)
    e.set_output(True, 8)
    pre = run(e, rc, path, 3)
    names = names_of(rc)
    ref = output_ref.output_ref(rc, rc.sigma, state_of(e, rc), names, leftovers(e, rc, pre))
    hold(fetch(e, names), ref, rc, names)


@pytest.mark.parametrize("name", ["C", "N"])
def test_leftovers_are_the_last_tends(name):
    """After a split-path step RH, PF, ZF and ZH are formed with atm1%pr, zq and pf3d as that step's
    tend left them at its start, and differ from the same formulas on the new state alone."""
    rc, data, st = CASES[name]()
    e = engine(rc, data, st)
    e.set_output(True, 8)
    e.step(2)
    pre = split_step(e, rc)
    names = [n for n in LEFTOVER if n in names_of(rc)]
    cur = state_of(e, rc)
    old = output_ref.output_ref(rc, rc.sigma, cur, names, leftovers(e, rc, pre, diag=False))
    got = fetch(e, names)
    for n in names:
        assert np.array_equal(got[n], old[n]) if n != "ZH" else relmax(got[n], old[n]) < 1e-13, n
    new_pre = pre_of(e, rc)
    e.tend_pre_physics()                      # mkslice of the new state
    new = output_ref.output_ref(rc, rc.sigma, cur, names, leftovers(e, rc, new_pre, diag=False))
    for n in names:
        assert relmax(new[n], old[n]) > 1e-9, n       # the test can tell the two apart
        assert relmax(got[n], new[n]) > 1e-9, n


@pytest.mark.parametrize("name", ["C", "N", "uw"])
def test_fp32_is_one_rounding_of_fp64(name):
    rc, data, st = cloudy(name)
    e = engine(rc, data, st)
    e.set_diagnostics(True)
    e.set_output(True, 8)
    run(e, rc, "step", 2)
    names = names_of(rc)
    d = fetch(e, names)
    e.set_output(True, 4)
    f = fetch(e, names)
    for n in names:
        assert f[n].dtype == np.float32 and d[n].dtype == np.float64, n
        assert np.array_equal(f[n].view(np.uint32), d[n].astype(np.float32).view(np.uint32)), n


def tiled_pair(rc, data, st, nproc):
    out = []
    for e in (engine(rc, data, st), engine(rc, data, st, nproc=nproc)):
        e.set_diagnostics(True)
        e.set_output(True, 8)
        run(e, rc, "step", 2)
        out.append(fetch(e, names_of(rc)))
    return out


@pytest.mark.parametrize("name", ["C", "N", "band"])
def test_tiles_equal_one_tile(name):
    """2 x 2 tiles exchanging the ghost line of atm1%u, atm1%v by device copies: every field, tile
    ring rows and corners and the band's periodic j + 1 column included, as on one tile."""
    rc, data, st = CASES[name]()
    one, four = tiled_pair(rc, data, st, (2, 2))
    for n in one:
        assert np.array_equal(one[n], four[n]), n


@pytest.mark.parametrize("name", ["C", "band"])
def test_tiles_over_rccl_equal_one_tile(name, monkeypatch):
    """The same with the halo messages as RCCL sends and receives (the self-communicator)."""
    rc, data, st = CASES[name]()
    monkeypatch.setenv("RCMDYN_FORCE_RCCL", "1")
    one, four = tiled_pair(rc, data, st, (2, 2))
    for n in one:
        assert np.array_equal(one[n], four[n]), n


@pytest.mark.parametrize("name", ["C", "N"])
def test_snapshot_is_of_the_call_time(name):
    """output_atm, step(3), get_output: the state of the call; a second output_atm: the later one."""
    rc, data, st = CASES[name]()
    e = engine(rc, data, st)
    e.set_output(True, 8)
    e.step(2)
    names = names_of(rc, slice_=False, diag=False)
    ref0 = output_ref.output_ref(rc, rc.sigma, state_of(e, rc), names)
    e.output_atm(names)
    e.step(3)
    got0 = {n: e.get_output(n) for n in names}
    ref1 = output_ref.output_ref(rc, rc.sigma, state_of(e, rc), names)
    got1 = fetch(e, names)
    for n in names:
        if n in LOG_BEARING:
            assert relmax(got0[n], ref0[n]) < 1e-13 and relmax(got1[n], ref1[n]) < 1e-13, n
        else:
            assert np.array_equal(got0[n], ref0[n]) and np.array_equal(got1[n], ref1[n]), n
    assert not np.array_equal(got0["T"], got1["T"])


def test_refusals():
    """Each refused call names its argument, leaves the engine usable and the state as a twin's."""
    from regcm_amd.dycore import EngineError
    rc, data, st = CASES["C"]()
    e, twin = engine(rc, data, st), engine(rc, data, st)
    e.step(1)
    twin.step(1)

    def refused(match, fn, *a):
        with pytest.raises(EngineError, match=match):
            fn(*a)

    refused("output stage is off", e.output_atm, ["T"])
    refused("output stage is off", e.get_output, "T")
    refused("prec = 2", e.set_output, True, 2)
    refused("output stage is off", e.output_atm, ["T"])               # the refused switch left it off
    e.set_output(True, 8)
    refused("OUT_T was not in the mask", e.get_output, "T")           # no snapshot yet
    refused("mask = 0", e.output_atm, [])
    refused("bit beyond", e.output_atm, 1 << 21)
    refused("unknown field 21", e.get_output, 21)
    refused("OUT_W: non-hydrostatic", e.output_atm, ["T", "W"])
    refused("OUT_PP: non-hydrostatic", e.output_atm, ["PP"])
    refused("OUT_QI: .*nqx = 5", e.output_atm, ["QI"])
    refused("OUT_QS: .*nqx = 5", e.output_atm, ["QS"])
    refused("OUT_TKE: .*ibltyp=2", e.output_atm, ["TKE"])
    for n in LEFTOVER:
        refused(f"OUT_{n}: no slice fields yet", e.output_atm, [n])
    refused("OUT_OMEGA: tendency diagnostics are off", e.output_atm, ["OMEGA"])
    e.output_atm(["T", "PS"])
    refused("OUT_U was not in the mask", e.get_output, "U")
    assert e.get_output("T").shape == (rc.kz, rc.iy, rc.jx) and e.get_output("PS").shape == (1, rc.iy, rc.jx)
    refused("OUT_W: non-hydrostatic", e.output_atm, ["W"])
    assert np.any(e.get_output("T") != 0.0)                           # a refused call keeps the snapshot
    e.step(2)
    twin.step(2)
    for n in state_names(rc):
        assert np.array_equal(e.get(n), twin.get(n)), n
    # the NH core: ZH and ZF are the host's constants
    rcn, datan, stn = CASES["N"]()
    en = engine(rcn, datan, stn)
    en.set_output(True, 4)
    split_step(en, rcn)
    refused("OUT_ZH: .*atm0%z", en.output_atm, ["ZH"])
    refused("OUT_ZF: zq/za/dzq", en.output_atm, ["ZF"])
    en.set_diagnostics(True)
    refused("OUT_OMEGA: .*no omega on the non-hydrostatic", en.output_atm, ["OMEGA"])
    en.output_atm(["RH", "PF", "W"])
    assert en.get_output("W").dtype == np.float32


@pytest.mark.parametrize("name", ["C", "N"])
def test_output_is_passive(name):
    """Two engines, one making output calls between its steps, hold the same prognostic state after 5
    steps; the profile of a step lists no launch of the stage, on or off."""
    rc, data, st = CASES[name]()
    a, b = engine(rc, data, st), engine(rc, data, st)
    b.set_output(True, 4)
    names = names_of(rc, slice_=False, diag=False)
    for q in range(5):
        for e in (a, b):
            advance(e, ("step", "pair", "physics")[q % 3], 1)
        b.output_atm(names + (["RH", "PF"] if q >= 2 else []))
        if q % 2:
            b.get_output("U")
    for n in state_names(rc):
        assert np.array_equal(a.get(n), b.get(n)), n
    assert a.get_time() == b.get_time()
    ka, kb = a.kernel_times(2), b.kernel_times(2)
    assert {k: v[0] for k, v in ka.items()} == {k: v[0] for k, v in kb.items()}
    assert not any("k_output" in k for k in ka)


class OutScript(Script):
    """The shim test's script with the three output calls (ops 28-30 of test_shim.F90)."""
    SET_OUTPUT, OUTPUT_ATM, GET_OUTPUT = 28, 29, 30

    def run_python(self):
        from regcm_amd.dycore import lib
        import ctypes
        L, h, out = lib(), ctypes.c_void_p(), []
        dp = ctypes.POINTER(ctypes.c_double)
        plain = {BDYVAL: L.rcmdyn_bdyval, PRE: L.rcmdyn_tend_pre_physics, POST: L.rcmdyn_tend_post_physics}
        for code, a in self.ops:
            if code == CREATE:
                rc = L.rcmdyn_create(ctypes.byref(self.cfg), ctypes.byref(h))
            elif code == PUT:
                rc = L.rcmdyn_put(h, a[1], a[8].ctypes.data_as(dp), *a[2:8])
            elif code in plain:
                rc = plain[code](h)
            elif code == STEP:
                rc = L.rcmdyn_step(h, a[0])
            elif code == self.SET_OUTPUT:
                rc = L.rcmdyn_set_output(h, *a)
            elif code == self.OUTPUT_ATM:
                rc = L.rcmdyn_output_atm(h, a[0])
            elif code == self.GET_OUTPUT:
                f, prec, j1, j2, i1, i2, k1, k2 = a
                buf = np.zeros((k2 - k1 + 1, i2 - i1 + 1, j2 - j1 + 1), dtype=np.float32 if prec == 4 else np.float64)
                rc = L.rcmdyn_get_output(h, f, buf.ctypes.data_as(ctypes.c_void_p), j1, j2, i1, i2, k1, k2)
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
                    if code == PUT:
                        f.write(struct.pack("<8i", *a[:8]) + a[8].tobytes())
                    elif a:
                        f.write(struct.pack(f"<{len(a)}i", *a))
                f.write(struct.pack("<i", 0))
            subprocess.run([EXE, fin, fout], check=True, timeout=timeout)
            buf = open(fout, "rb").read()
        out, pos = [], 0
        for code, a in self.ops:
            if code == self.GET_OUTPUT:
                n = a[1] * (a[3] - a[2] + 1) * (a[5] - a[4] + 1) * (a[7] - a[6] + 1)
                out.append(buf[pos:pos + n])
                pos += n
        assert pos == len(buf)
        return out


@pytest.mark.parametrize("prec", [4, 8])
def test_fortran_host_gets_the_python_hosts_bytes(prec):
    """A Fortran host through the shim (mod_gpu_dyn's three bindings): the same script, the same bytes."""
    from regcm_amd.config import build_config
    rc, data, st = cloudy("C")
    s = OutScript(build_config(rc, data["split"]))
    s.add(CREATE)
    for n, a in st.items():
        s.put(n, a)
    s.add(BDYVAL).add(s.SET_OUTPUT, 1, prec).add(STEP, 2).add(PRE).add(POST).add(BDYVAL)
    names = names_of(rc, diag=False)
    mask = sum(1 << OUTPUT_FIELD[n] for n in names)
    s.add(s.OUTPUT_ATM, mask).add(STEP, 1)
    for n in names:
        nk = 1 if n in output_ref.TWO_D else rc.kz
        s.add(s.GET_OUTPUT, OUTPUT_FIELD[n], prec, 1, rc.jx, 1, rc.iy, 1, nk)
    py, fo = s.run_python(), s.run_fortran()
    assert len(py) == len(fo) == len(names)
    for n, a, b in zip(names, py, fo):
        assert a == b and any(a), n
