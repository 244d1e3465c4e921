"""CPU checks of the SUBEX condensation inside tend (rcmdyn_set_condtq, rcmdyn_put_rh0adj,
rcmdyn_get_condtq; regcm_amd/csrc/condtq.hpp).

The yardstick is a restatement of the Fortran text (tests/condtq_ref.py), since the oracle stubs
condtq as well: condtq has no transcendental function, so with -ffp-contract=off the header's
per-point function is held to that transcription bit for bit, over a table that populates every
branch.  The inputs of the GPU tests (tests/test_condtq_gpu.py) are checked here too, on the
oracle alone: their branch populations and the cap on the points left out at the thresholds."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from regcm_amd import dycore
from tests import condtq_ref as cq
from tests.support import case, oracle, relerr, state_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rcmdyn.h")
FDIR = os.path.join(ROOT, "regcm_amd", "fortran")
CALLS = ["rcmdyn_set_condtq", "rcmdyn_put_rh0adj", "rcmdyn_get_condtq"]


def test_condtq_calls_declared_exported_and_bound():
    src = open(HEADER).read()
    L = dycore.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dycore.LIB_PATH], capture_output=True, text=True).stdout
    for n in CALLS:
        assert re.search(rf"^int {n}\(rcmdyn_t\* h", src, re.M), n
        assert n in dycore.EXPORTED
        assert re.search(rf"\bT {n}$", nm, re.M), n
    i32, dp, P = ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    assert L.rcmdyn_set_condtq.argtypes == [P, i32, ctypes.c_double]
    assert L.rcmdyn_put_rh0adj.argtypes == [P, dp] + [i32] * 6
    assert L.rcmdyn_get_condtq.argtypes == [P, i32, dp] + [i32] * 6
    for m in ("set_condtq", "put_rh0adj", "get_condtq"):
        assert callable(getattr(dycore.DynCore, m)), m
    # no ABI bump, and one order of the terms in the header, the Python host and the Fortran shim
    assert re.search(r"#define RCMDYN_ABI_VERSION 6\b", src)
    body = src.split("enum rcmdyn_condtq_term", 1)[1].split("}", 1)[0]
    assert re.findall(r"RCMDYN_CONDTQ_(\w+)", body) == dycore.CONDTQ_TERMS
    f90 = open(os.path.join(FDIR, "mod_gpu_dyn.F90")).read()
    ids = {m.group(1).upper(): int(m.group(2)) for m in re.finditer(r"\bcondtq_(\w+)\s*=\s*(\d+)", f90.lower())}
    assert ids == {n: q for q, n in enumerate(dycore.CONDTQ_TERMS)}
    for n in CALLS:
        assert re.search(rf"bind\(c, name='{n}'\)", f90), n
        assert re.search(rf"public ::.*\b{n}\b", f90), n


def table(n=40000, seed=3):
    """Rows of (t2, qv2, qc2, tt, tqv, tqc, psc, pres, qs, rh0adj, dt, conf): realistic points, and
    blocks of rows that force each clamp and branch."""
    rng = np.random.Generator(np.random.PCG64(seed))
    psc = rng.uniform(60.0, 101.0, n)
    dt = rng.choice([30.0, 60.0, 150.0], n)
    conf = rng.choice([1.0, 0.7, 0.25], n)
    T = rng.uniform(215.0, 312.0, n)
    q = n // 20
    T[:q] = rng.uniform(374.0, 390.0, q)                 # pfesat's upper clamp
    T[q:2 * q] = rng.uniform(170.0, 198.0, q)            # and its lower one
    T[2 * q:3 * q] = rng.uniform(272.9, 273.4, q)        # around td = 0, tc = 0
    pres = (rng.uniform(0.02, 0.995, n) * psc + 5.0) * 1000.0
    pres[:q] = 106000.0                                  # above es(100 C): qvs stays positive
    qsat = cq.pfwsat(T, pres)
    rh = rng.uniform(0.05, 1.25, n)
    rh[3 * q:4 * q] = rng.uniform(0.9999, 1.00002, q)    # around the high-cover threshold
    qs = qsat * rng.uniform(0.7, 1.3, n)
    qs[4 * q:4 * q + 50] = -1.0e-6                       # qvc_cld = max(qs, 0)
    tt = rng.standard_normal(n) * 2.0e-3 * psc
    tqv = rng.standard_normal(n) * 2.0e-8 * psc
    tqc = rng.standard_normal(n) * 2.0e-9 * psc
    t2 = T * psc - dt * tt
    qv2 = rh * qsat * psc - dt * tqv
    qv2[5 * q:6 * q] = rng.uniform(-1.0e-8, 0.9e-8, q) * psc[5 * q:6 * q] - (dt * tqv)[5 * q:6 * q]   # the minqq clamp
    qc2 = np.where(rng.uniform(size=n) < 0.5, 0.0, rng.uniform(0.0, 6.0e-4, n) * psc)
    qc2[6 * q:7 * q] = rng.uniform(-2.0e-20, 2.0e-20, q) * psc[6 * q:7 * q] - (dt * tqc)[6 * q:7 * q]  # the dlowval clamp
    rh0adj = rng.uniform(0.0, cq.RH0MAX, n)
    rh0adj[7 * q:8 * q] = 0.0
    rh0adj[8 * q:9 * q] = cq.RH0MAX
    rows = [t2, qv2, qc2, tt, tqv, tqc, psc, pres, qs, rh0adj, dt, conf]
    # rhc == rh0adj exactly and no cloud water: fccc = 0, tmp1 = 0, tmp2 = 0 (|tmp2| <= dlowval)
    z = slice(9 * q, 10 * q)
    qc2[z] = 0.0
    tqc[z] = 0.0
    r = cq.condtq(*[a[z] for a in rows])
    rh0adj[z] = np.minimum(r["rhc"], cq.RH0MAX)
    return rows


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_point_function_equals_the_fortran_text_bit_for_bit(tmp_path):
    exe = tmp_path / "condtq_point"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-o", str(exe),
                    os.path.join(ROOT, "tests", "condtq", "condtq_point.cpp")], check=True)
    rows = table()
    ref = cq.condtq(*rows)
    n = len(rows[0])
    # every branch is populated
    count = {
        "rhc < rh0adj": ref["low"].sum(), "rhc > 0.99999": ref["high"].sum(), "partial cover": ref["part"].sum(),
        "exces >= 0": ref["left"].sum(), "exces < 0": (~ref["left"]).sum(),
        "|tmp2| <= dlowval": (~ref["on"]).sum(), "|tmp2| > dlowval": ref["on"].sum(),
        "minqq*psc clamp": ref["clamp_qv"].sum(), "dlowval*psc clamp": (ref["clamp_qc"] & (rows[2] + rows[10] * rows[5] != 0.0)).sum(),
        "tc > 0": (ref["tc"] > 0).sum(), "tc <= 0": (ref["tc"] <= 0).sum(),
        "td >= 0": ((ref["td"] >= 0) & (ref["td"] < 100)).sum(), "td < 0": ((ref["td"] < 0) & (ref["td"] > -75)).sum(),
        "td = 100": (ref["td"] == 100.0).sum(), "td = -75": (ref["td"] == -75.0).sum(),
        "qs < 0": (rows[8] < 0).sum(),
    }
    for what, c in count.items():
        assert c >= 50, (what, int(c))
    text = "".join(" ".join(float(a[q]).hex() for a in rows) + "\n" for q in range(n))
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split()
    got = np.array([float.fromhex(w) for w in out]).reshape(n, 5)
    for col, key in enumerate(("tmp2", "wwlh", "it", "iqv", "iqc")):
        a, b = got[:, col], np.asarray(ref[key], dtype=np.float64)
        same = a.view(np.int64) == b.view(np.int64)
        assert same.all(), (key, int((~same).sum()), a[~same][:3], b[~same][:3])


@pytest.mark.parametrize("name", ["C", "N"])
def test_gpu_inputs_populate_the_branches_on_the_oracle_alone(name):
    """The oracle-side reference of tests/test_condtq_gpu.py, first step: each cloud-cover branch
    and each exces branch holds at least 1 % of the interior points, and the continuous rh0adj
    leaves no point within 1e-9 of a threshold (the cap there is 0.1 % per level)."""
    rc, data, st0 = case(name, **({"ifrayd": 0} if name == "N" else {}))
    st = cq.moist_state(rc, st0)
    rh0 = cq.rh0adj_field(rc)
    assert rh0.min() == 0.0 and rh0.max() == cq.RH0MAX and (rh0 == 0.0).sum() > 20 and (rh0 == cq.RH0MAX).sum() > 20
    names = state_names(rc)
    tp = cq.TwoPass(lambda: oracle(rc, data, st), rc, names, rh0)
    inc, out = tp.step()
    npts = out["low"].size
    for key in ("low", "high", "part"):
        assert out[key].sum() >= 0.01 * npts, (key, int(out[key].sum()), npts)
    assert out["left"].sum() >= 0.01 * npts and (~out["left"]).sum() >= 0.01 * npts
    assert out["on"].sum() >= 0.5 * npts
    assert int(out["near"].sum()) == 0
    assert np.all(out["near"].sum(axis=(1, 2)) <= 0.001 * out["near"][0].size)
    for a in inc.values():
        assert np.all(np.isfinite(a))
    # the reference runs on with the term: ten more steps without a CFL violation or a NaN
    for _ in range(10):
        inc, out = tp.step()
        assert np.all(out["near"].sum(axis=(1, 2)) <= 0.001 * out["near"][0].size)
    for n in names:
        assert np.all(np.isfinite(tp.R.get(n))), n


@pytest.mark.parametrize("name,over,probe_over", [("C", {"i_band": 1}, None), ("N", {"ifrayd": 1}, {"ifrayd": 0})],
                         ids=["band", "nh-rayleigh"])
def test_gpu_inputs_of_the_band_and_the_rayleigh_case_on_the_oracle_alone(name, over, probe_over):
    """The first step of the two further cases of tests/test_condtq_gpu.py.  Band: the columns on
    both sides of the period's seam hold evaporated cloud (whose noise-level qc forecast meets the
    negative-moisture fix) and points below their rh0adj (which a zero rh0adj would move to
    another branch).  ifrayd = 1: the probe runs with ifrayd = 0 from the same state, and condtq
    is at work on the damped levels."""
    rc, data, st0 = case(name, **over)
    st = cq.moist_state(rc, st0)
    rh0 = cq.rh0adj_field(rc)
    probe = None
    if probe_over:
        prc, pdata, _ = case(name, **probe_over)
        probe = lambda: oracle(prc, pdata, st)
    tp = cq.TwoPass(lambda: oracle(rc, data, st), rc, state_names(rc), rh0, probe=probe)
    inc, out = tp.step()
    npts = out["low"].size
    for key in ("low", "high", "part"):
        assert out[key].sum() >= 0.01 * npts, (key, int(out[key].sum()), npts)
    assert out["left"].sum() >= 0.01 * npts and (~out["left"]).sum() >= 0.01 * npts
    assert int(out["near"].sum()) == 0
    for a in inc.values():
        assert np.all(np.isfinite(a))
    for n in state_names(rc):
        assert np.all(np.isfinite(tp.R.get(n))), n
    if rc.i_band:
        assert out["on"].shape[2] == rc.jx
        seam = [0, 1, rc.jx - 2, rc.jx - 1]
        assert (~out["left"])[:, :, seam].sum() >= 40 and out["low"][:, :, seam].sum() >= 40
    else:
        assert rc.ifrayd == 1 and out["on"][:rc.rayndamp].sum() >= 0.5 * out["on"][:rc.rayndamp].size


def test_the_reference_itself_amplifies_rounding_noise():
    """Why ten steps with condtq cannot be held to the parity bounds without it (the bounds of
    tests/test_condtq_gpu.py): under a 1e-14 perturbation of the initial temperature the two-pass
    reference departs from itself by more than 1e-4 of max |qc| at the second step, with no
    cloud-cover branch changed, while the oracle without condtq stays below 1e-11.  An
    evaporated cloud leaves a qc forecast of rounding noise of either sign, and the
    negative-moisture fix (Main/mod_tendency.F90:382-393) turns a negative one into 1 % of its
    neighbours' mean."""
    rc, data, st0 = case("C")
    st = cq.moist_state(rc, st0)
    st2 = {k: v.copy() for k, v in st.items()}
    st2["ATM1_T"] = st2["ATM1_T"] * (1.0 + 1e-14)
    rh0 = cq.rh0adj_field(rc)
    names = state_names(rc)
    a = cq.TwoPass(lambda: oracle(rc, data, st), rc, names, rh0)
    b = cq.TwoPass(lambda: oracle(rc, data, st2), rc, names, rh0)
    oa, ob = oracle(rc, data, st), oracle(rc, data, st2)
    for _ in range(2):
        outa, outb = a.step()[1], b.step()[1]
        assert all(np.array_equal(outa[k], outb[k]) for k in ("low", "high", "part"))
    oa.step(2)
    ob.step(2)
    assert relerr(b.R.get("ATM1_QC"), a.R.get("ATM1_QC"), rc, "ATM1_QC") > 1e-4
    assert relerr(b.R.get("ATM1_T"), a.R.get("ATM1_T"), rc, "ATM1_T") < 1e-12
    for n in names:
        assert relerr(ob.get(n), oa.get(n), rc, n) < 1e-11, n
