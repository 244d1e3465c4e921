"""bench.py --dump-outputs: which fields are written, in what form, and that a state larger
than the byte budget is thinned to the same points in every run.  Checked on CPU with a
stand-in engine that serves known arrays."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from regcm_amd.config import CONFIGS, NH_STATE_FIELDS, STATE_FIELDS, field_levels  # noqa: E402


class _ServingEngine:
    def __init__(self, rc):
        self.rc = rc

    def get(self, name):
        nk = field_levels(name, self.rc.kz, self.rc.nsplit)
        n = nk * self.rc.iy * self.rc.jx
        seed = bench.output_fields(self.rc).index(name)
        return (np.arange(n, dtype=np.float64) + 0.5 * seed).reshape(nk, self.rc.iy, self.rc.jx)


def test_output_fields_follow_the_core():
    assert bench.output_fields(CONFIGS["C3"]) == STATE_FIELDS
    nh = bench.output_fields(CONFIGS["N1"])
    assert set(NH_STATE_FIELDS) <= set(nh) and "DSTOR" not in nh and "HSTOR" not in nh
    assert {"ATM1_TKE", "ATM2_TKE"} <= set(bench.output_fields(CONFIGS["CRM"]))


def test_small_state_is_written_whole(tmp_path):
    rc = CONFIGS["C1"]
    eng = _ServingEngine(rc)
    bench.dump_outputs(eng, rc, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in STATE_FIELDS)
    for name in STATE_FIELDS:
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float64
        assert np.array_equal(a, eng.get(name).ravel())


def test_large_state_is_thinned_to_the_same_points(tmp_path, monkeypatch):
    rc = CONFIGS["C1"]
    eng = _ServingEngine(rc)
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    bench.dump_outputs(eng, rc, str(tmp_path / "a"))
    bench.dump_outputs(eng, rc, str(tmp_path / "b"))
    total = 0
    for name in STATE_FIELDS:
        a = np.load(tmp_path / "a" / (name + ".npy"))
        b = np.load(tmp_path / "b" / (name + ".npy"))
        assert np.array_equal(a, b)
        full = eng.get(name).ravel()
        assert a.ndim == 1 and 0 < a.size < full.size
        # a sorted sample without replacement of this field's own points
        assert np.all(np.diff(a) > 0) and np.all(np.isin(a, full))
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert 0.9 * (1 << 20) < total <= (1 << 20) + 128 * len(STATE_FIELDS)
    # fields of one shape keep the same points
    u = np.load(tmp_path / "a" / "ATM1_U.npy")
    v = np.load(tmp_path / "a" / "ATM1_V.npy")
    assert np.array_equal(v - u, np.full(u.size, 0.5))


def test_boundary_is_held_at_its_first_record():
    """The bench steps far past the one boundary interval the ICBC spans: the boundary
    tendencies are zero, everything else is as generated."""
    from regcm_amd import icbc
    for cfg, gen in (("C1", icbc.generate), ("N1", icbc.generate_nh)):
        rc = CONFIGS[cfg]
        want = gen(rc)
        got = bench.hold_boundary(gen(rc))
        assert got["split"].keys() == want["split"].keys()
        assert got["state"].keys() == want["state"].keys()
        held = [n for n in want["state"] if n.endswith("_BT")]
        assert len(held) >= 5
        for name, a in want["state"].items():
            b = got["state"][name]
            assert b.shape == a.shape and b.dtype == a.dtype
            assert not b.any() if name in held else np.array_equal(a, b), name
