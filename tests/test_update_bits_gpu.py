"""The bits of the tendency kernels (k_columns, k_update, k_momentum, k_scalars) against the
commit that last changed their arithmetic: a sha256 of the state after bdyval() and step(3) (the
dt switch at lcount 2 lies inside), with the tendency diagnostics, the budget terms and the
condtq increments where those are on, compared with tests/golden/update_bits_parent.json.  A
change that only moves arithmetic (earlier in a block, into a helper) keeps every hash; one that
changes results on purpose records the file again and says so.

The grid is support.case("C"), 37 x 29 x 18: partial 32 x 8 blocks in j (32 + 5) and in i
(3 * 8 + 5), levels 1 and kz for the k - 1 / k + 1 guards, relaxation-band and interior points.
The generated state has no cloud water and no dry point, so both moisture thresholds of the
vertical fluxes would take one side only; the input here adds patchy cloud water
(icbc.hydrometeor_state) and seeded dry points, and the module asserts from that input that
both sides occur.

The golden file also holds a sha256 of each case's input: if the generated input differs on the
machine (another numpy, another libm), the test fails and asks for a new record from the commit
the golden file names.  Record with the library of that commit:

    RCMDYN_LIB=<library> python -m tests.test_update_bits_gpu --record
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from regcm_amd import icbc
from regcm_amd.config import QX_STATE_FIELDS, STATE_FIELDS, TKE_STATE_FIELDS
from tests.support import case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_bits_parent.json")
TEND_DIAG = ["TTEN", "UTEN", "VTEN", "QVTEN", "QCTEN", "OMEGA", "XKC"]
MINQQ = 1.0e-8            # Share/mod_constants.F90:57
NO_FUSE = {"RCMDYN_NO_FUSE_UPDATE": "1"}

# name: (RunConfig overrides, environment switches, tiles, instance switches)
CASES = {
    "default-set": ({}, {}, (1, 1), ("nodiag",)),
    "generic": ({}, {}, (1, 1), ()),
    "NO_OPTSET": ({}, {"RCMDYN_NO_OPTSET": "1"}, (1, 1), ("nodiag",)),
    "NO_FUSE_UPDATE": ({}, NO_FUSE, (1, 1), ("nodiag",)),
    "generic NO_FUSE_UPDATE": ({}, NO_FUSE, (1, 1), ()),
    "2x2": ({}, {}, (2, 2), ("nodiag",)),
    "generic 2x2": ({}, {}, (2, 2), ()),
    "iboudy=4": ({"iboudy": 4}, {}, (1, 1), ()),
    "isladvec=1": ({"isladvec": 1}, {}, (1, 1), ()),
    "ipgf=1": ({"ipgf": 1}, {}, (1, 1), ()),
    "ipptls=2": ({"ipptls": 2}, {}, (1, 1), ()),
    "ibltyp=2 iuwvadv=1": ({"ibltyp": 2, "iuwvadv": 1}, {}, (1, 1), ()),
    "budget+condtq": ({}, {}, (1, 1), ("budget", "condtq")),
    "budget+condtq NO_FUSE_UPDATE": ({}, NO_FUSE, (1, 1), ("budget", "condtq")),
}


def interior(rc, a):
    """The points jci x ici of a cross-grid field (Fortran 2..jx-2, 2..iy-2)."""
    return a[..., 1:rc.iy - 2, 1:rc.jx - 2]


_INPUT = {}


def input_state(over):
    """(rc, data, state, rh0adj) of a case: the shared "C" state (copied, never changed) with
    cloud water where the configuration has none and with dry points, qv below MINQQ p*, on one
    point in eight of atm1 and atm2 alike."""
    key = tuple(sorted(over.items()))
    if key not in _INPUT:
        rc, data, st0 = case("C", **over)
        st = dict(st0)
        if rc.nqx == 2:
            st.update(icbc.hydrometeor_state(rc, st, nqx=2))
        rng = np.random.Generator(np.random.PCG64(icbc.SEED + 12))
        dry = rng.uniform(size=(rc.kz, rc.iy, rc.jx)) < 0.125
        for n in ("ATM1_QV", "ATM2_QV"):
            st[n] = np.where(dry, 0.25 * MINQQ * st["PSA"], st[n])
        if rc.iuwvadv == 1:     # a PBL top on every level 1..kz: vadv4d ind = 3 takes each of its branches
            st["KPBL"] = rng.integers(1, rc.kz + 1, (1, rc.iy, rc.jx)).astype(np.float64)
        rh0 = rng.uniform(0.0, 0.99999, (rc.kz, rc.iy, rc.jx))
        _INPUT[key] = (rc, data, st, rh0)
    return _INPUT[key]


def input_digest(st, rh0):
    h = hashlib.sha256()
    for n in sorted(st):
        h.update(n.encode())
        h.update(np.ascontiguousarray(st[n], dtype=np.float64).tobytes())
    h.update(rh0.tobytes())
    return h.hexdigest()


def state_digest(name):
    """(sha256 of the input, sha256 of the outputs) of a case."""
    from regcm_amd.dycore import BUDGET_TERMS, DynCore
    over, env, tiles, switches = CASES[name]
    rc, data, st, rh0 = input_state(over)
    names = list(STATE_FIELDS) + (QX_STATE_FIELDS if rc.nqx > 2 else []) + (TKE_STATE_FIELDS if rc.ibltyp == 2 else [])
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = DynCore(rc, data["split"], nproc_j=tiles[0], nproc_i=tiles[1])
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        e.put_state(st)
        e.set_diagnostics("nodiag" not in switches)
        if "budget" in switches:
            e.set_budget(True)
        if "condtq" in switches:
            e.set_condtq(True, 1.0)
            e.put_rh0adj(rh0)
        e.bdyval()
        e.step(3)
        e.synchronize()
        h = hashlib.sha256()
        for n in names + (TEND_DIAG if "nodiag" not in switches else []):
            h.update(n.encode())
            h.update(np.ascontiguousarray(e.get(n)).tobytes())
        if "budget" in switches:
            for n in BUDGET_TERMS:
                h.update(str(n).encode())
                h.update(e.get_budget(n).tobytes())
        if "condtq" in switches:
            for n in ("T", "QV", "QC"):
                h.update(n.encode())
                h.update(e.get_condtq(n).tobytes())
    finally:
        e.close()
    return input_digest(st, rh0), h.hexdigest()


def test_both_sides_of_each_moisture_threshold():
    """From the input alone: among the interior points, qc1 > MINQQ^2 psa holds at some and not
    at others (vadv4d's flux select), and the qv pair of an interface, both above MINQQ psa,
    likewise (vadvqv's) - so the selects of the vertical fluxes run both branches."""
    for over in ({}, {"ipptls": 2}, {"ibltyp": 2, "iuwvadv": 1}):
        rc, _, st, _ = input_state(over)
        ps = st["PSA"]
        qc = interior(rc, st["ATM1_QC"] > MINQQ * MINQQ * ps)
        assert qc.any() and not qc.all(), over
        qv = st["ATM1_QV"] > MINQQ * ps
        pair = interior(rc, qv[1:] & qv[:-1])
        assert pair.any() and not pair.all(), over
        # each side of the pair's own two tests: the level itself dry, its neighbour dry
        assert interior(rc, qv[1:] & ~qv[:-1]).any() and interior(rc, ~qv[1:] & qv[:-1]).any(), over


@pytest.mark.parametrize("name", list(CASES))
def test_state_bits_as_recorded(name):
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    assert name in gold["cases"], f"{name}: not in {GOLDEN}: record it from commit {gold['commit']}"
    din, dout = state_digest(name)
    assert din == gold["cases"][name]["input"], (
        f"{name}: the generated input differs from the recorded one on this machine; "
        f"record {os.path.basename(GOLDEN)} again with the library of commit {gold['commit']}")
    assert dout == gold["cases"][name]["state"], f"{name}: the state after bdyval + step(3) changed bits"


def record(commit):
    cases = {}
    for name in CASES:
        din, dout = state_digest(name)
        cases[name] = {"input": din, "state": dout}
        print(f"{name:30s} {dout}", flush=True)
    with open(GOLDEN, "w") as fh:
        json.dump({"commit": commit, "cases": cases}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: RCMDYN_LIB=<library of the recorded commit> python -m tests.test_update_bits_gpu "
                 "--record [commit]")
    rest = [a for a in sys.argv[1:] if a != "--record"]
    record(rest[0] if rest else "unknown")
