"""The index arithmetic behind every put and get of the engine (regcm_amd/csrc/window.hpp): a
stand-alone host program (tests/window/window_probe.cpp, built with the address and
undefined-behaviour sanitizers, every buffer a heap block of exactly its size) runs scatter() and
gather() on a table of cases and prints the arrays; this file restates both in plain loops over
every array point and compares exactly.

The shapes are the smallest at which the arithmetic can go wrong: a 9 x 7 domain of three levels
with the engine's ghost ring of 4 (so a frame reaches past both ends of a period), one tile and the
four tiles of a 2 x 2 split with their frames (row pitch a multiple of 16, larger than nj), and the
output stream's compact interior buffer with an element offset, in float and double."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JX, IY, NK, RING = 9, 7, 3, 4
PERIODS = {"none": (0, 0), "band": (1, 0), "crm": (1, 1)}
# owned dot ranges (jde1, jde2, ide1, ide2): one tile, then the 2 x 2 split at j = 5 | 6, i = 4 | 5
TILES = {"1x1": (1, JX, 1, IY), "2x2-00": (1, 5, 1, 4), "2x2-01": (1, 5, 5, IY), "2x2-10": (6, JX, 1, 4),
         "2x2-11": (6, JX, 5, IY)}
BOXES = {
    "whole": (1, JX, 1, IY, 1, NK),
    "interior": (3, 7, 2, 5, 2, 3),
    "one cell": (6, 6, 5, 5, 2, 2),
    "across the seam": (4, 7, 3, 6, 1, NK),
    "outside tile 11": (1, 1, 1, 2, 1, NK),
    "j = 1 and j = jx": (1, JX, 2, 3, 1, NK),
    "west columns": (1, 2, 1, IY, 1, NK),
    "east columns": (8, JX, 1, IY, 1, NK),
    "north rows": (3, 4, 6, IY, 1, NK),
    "k1 = 0": (2, 8, 2, 6, 0, 2),
    "k2 = nk + 2": (2, 8, 2, 6, 2, NK + 2),
    "j2 < j1": (5, 3, 1, IY, 1, NK),
    "j2 < j1 and i2 < i1": (5, 3, 6, 2, 1, NK),
}
EMPTY = ("j2 < j1", "j2 < j1 and i2 < i1")


def frame(tile):
    """A tile's frame as the engine lays it out: the owned dot points and the ghost ring, rows of a
    multiple of 16 elements: (j0, i0, nj, ni, pitch, plane, nk, off)."""
    j1, j2, i1, i2 = TILES[tile]
    nj, ni = j2 - j1 + 1 + 2 * RING, i2 - i1 + 1 + 2 * RING
    pitch = (nj + 15) // 16 * 16
    assert pitch > nj
    return (j1 - RING, i1 - RING, nj, ni, pitch, pitch * ni, NK, 0)


def interior(tile, period):
    """The tile's interior cross points (ja, jb, ia, ib): 2 .. n - 2, every point of a periodic direction."""
    j1, j2, i1, i2 = TILES[tile]
    band, crm = PERIODS[period]
    return (max(j1, 1 if band else 2), min(j2, JX if band else JX - 2),
            max(i1, 1 if crm else 2), min(i2, IY if crm else IY - 2))


def compact(tile, period, nk, off):
    """The output stream's buffer of a tile: its interior cross points alone, rows of nj elements, the
    field's first element at off."""
    ja, jb, ia, ib = interior(tile, period)
    nj, ni = jb - ja + 1, ib - ia + 1
    return (ja, ia, nj, ni, nj, nj * ni, nk, off)


def wrap(v, n, periodic):
    return v if not periodic else v + n if v < 1 else v - n if v > n else v


def cells(box):
    j1, j2, i1, i2, k1, k2 = box
    return max(0, j2 - j1 + 1) * max(0, i2 - i1 + 1) * max(0, k2 - k1 + 1)


def points(stg):
    """Every (element, k, i, j) of a staging array."""
    j0, i0, nj, ni, pitch, plane, nk, off = stg
    for k, i, j in itertools.product(range(1, nk + 1), range(i0, i0 + ni), range(j0, j0 + nj)):
        yield off + (k - 1) * plane + (i - i0) * pitch + (j - j0), k, i, j


def cell(box, k, i, j):
    """The host offset of (k, i, j), j fastest, or None outside the box."""
    j1, j2, i1, i2, k1, k2 = box
    if not (j1 <= j <= j2 and i1 <= i <= i2 and k1 <= k <= k2):
        return None
    return ((k - k1) * (i2 - i1 + 1) + (i - i1)) * (j2 - j1 + 1) + (j - j1)


def scatter_ref(stg, period, box, dtype):
    band, crm = PERIODS[period]
    a = -(np.arange(stg[7] + stg[6] * stg[5], dtype=dtype) + 1)
    for e, k, i, j in points(stg):
        q = cell(box, k, wrap(i, IY, crm), wrap(j, JX, band))
        if q is not None:
            a[e] = q + 1
    return a


def gather_ref(stg, box, rng, dtype):
    ja, jb, ia, ib = rng
    dst = np.full(cells(box), np.nan, dtype=dtype)
    for e, k, i, j in points(stg):
        q = cell(box, k, i, j)
        if q is not None and ja <= j <= jb and ia <= i <= ib:
            dst[q] = e + 1
    return dst


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("window") / "window_probe"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "window", "window_probe.cpp")], check=True)

    def run(rows):
        """rows of (op, type, staging, period, box, range): the printed array of each."""
        text = "".join(" ".join([op, ty] + [str(int(x)) for x in stg + (JX, IY) + PERIODS[per] + box + rng]) + "\n"
                       for op, ty, stg, per, box, rng in rows)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout
        lines = out.split("\n")[:-1]
        assert len(lines) == len(rows)
        return [np.array([float(x) for x in ln.split()], dtype=np.float32 if r[1] == "f" else np.float64)
                for ln, r in zip(lines, rows)]
    return run


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def test_scatter_into_frames(probe):
    """Every tile's frame takes every box under every period rule: the ghost ring, the points past
    either end of a period by their wrapped index, the level clamp; nothing else is written."""
    rows = [("s", "d", frame(t), p, BOXES[b], (0, 0, 0, 0)) for t in TILES for p in PERIODS for b in BOXES]
    got = probe(rows)
    bad = [(r[2:5]) for r, g in zip(rows, got) if not same(g, scatter_ref(r[2], r[3], r[4], np.float64))]
    assert not bad, bad
    written = {(t, p, b): int((g > 0).sum()) for (t, p, b), g in
               zip(itertools.product(TILES, PERIODS, BOXES), got)}
    for t, p in itertools.product(TILES, PERIODS):
        assert all(written[(t, p, b)] == 0 for b in EMPTY), (t, p)
    # the whole domain on one tile: the owned points, and past each periodic end the ring's 4 more
    assert written[("1x1", "none", "whole")] == NK * IY * JX
    assert written[("1x1", "band", "whole")] == NK * IY * (JX + 2 * RING)
    assert written[("1x1", "crm", "whole")] == NK * (IY + 2 * RING) * (JX + 2 * RING)
    # the wrapped ghost columns on both sides are hit, and only with the period
    assert written[("1x1", "band", "j = 1 and j = jx")] == NK * 2 * (JX + 2 * RING)
    assert written[("1x1", "band", "west columns")] == 2 * written[("1x1", "none", "west columns")]
    assert written[("1x1", "band", "east columns")] == 2 * written[("1x1", "none", "east columns")]
    assert written[("1x1", "crm", "north rows")] == 2 * written[("1x1", "band", "north rows")]
    # tile 11's frame starts at j = 2: j = 1 reaches it only round the band
    assert written[("2x2-11", "none", "outside tile 11")] == 0 and written[("2x2-11", "band", "outside tile 11")] > 0


@pytest.mark.parametrize("part", ["owned", "interior"])
def test_gather_from_frames(probe, part):
    """The owned dot points, or the interior cross points alone, of every tile into every box: dst
    starts as NaN and exactly the expected cells change; the four tiles of the split fill disjoint
    cells that together are the one tile's."""
    def rng(t, p):
        return TILES[t] if part == "owned" else interior(t, p)
    keys = list(itertools.product(TILES, PERIODS, BOXES))
    rows = [("g", "d", frame(t), p, BOXES[b], rng(t, p)) for t, p, b in keys]
    got = dict(zip(keys, probe(rows)))
    bad = [k for k, r in zip(keys, rows) if not same(got[k], gather_ref(r[2], r[4], r[5], np.float64))]
    assert not bad, bad
    for p, b in itertools.product(PERIODS, BOXES):
        filled = [~np.isnan(got[(t, p, b)]) for t in TILES]
        assert got[("1x1", p, b)].size == cells(BOXES[b])
        assert np.array_equal(sum(f.astype(int) for f in filled[1:]), filled[0].astype(int)), (p, b)
        if b in EMPTY:
            assert got[("1x1", p, b)].size == 0
    n = IY * JX if part == "owned" else (IY - 3) * (JX - 3)
    assert int((~np.isnan(got[("1x1", "none", "whole")])).sum()) == NK * n
    assert not np.isnan(got[("2x2-00", "none", "whole")]).all()
    assert np.isnan(got[("2x2-11", "none", "outside tile 11")]).all()


@pytest.mark.parametrize("ty", ["f", "d"])
def test_gather_from_the_compact_output_buffer(probe, ty):
    """The output stream's case: a tile's interior cross points alone, rows of nj elements, a field of
    one level and one of three at a non-zero element offset, as floats and as doubles."""
    dtype = np.float32 if ty == "f" else np.float64
    keys = [(t, p, b, nk) for t in TILES for p in PERIODS for b in BOXES for nk in (1, NK)]
    rows = [("g", ty, compact(t, p, nk, 7 if nk == 1 else 7 + 35), p, BOXES[b], interior(t, p)) for t, p, b, nk in keys]
    got = probe(rows)
    bad = [k for k, r, g in zip(keys, rows, got) if not same(g, gather_ref(r[2], r[4], r[5], dtype))]
    assert not bad, bad
    by = dict(zip(keys, got))
    # the first element read is the one at the offset
    assert np.nanmin(by[("1x1", "crm", "whole", 1)]) == 8 and np.nanmin(by[("1x1", "crm", "whole", NK)]) == 43
    assert int((~np.isnan(by[("1x1", "none", "whole", NK)])).sum()) == NK * (IY - 3) * (JX - 3)
    assert int((~np.isnan(by[("1x1", "none", "whole", 1)])).sum()) == (IY - 3) * (JX - 3)


def test_scatter_into_a_compact_array(probe):
    """scatter on an array with an element offset and no ghost ring, in both types: the points before
    the offset stay as they were."""
    for ty, dtype in (("f", np.float32), ("d", np.float64)):
        rows = [("s", ty, compact("1x1", p, NK, 11), p, BOXES[b], (0, 0, 0, 0)) for p in PERIODS for b in BOXES]
        got = probe(rows)
        bad = [r[3:5] for r, g in zip(rows, got) if not same(g, scatter_ref(r[2], r[3], r[4], dtype))]
        assert not bad, bad
        assert all((g[:11] < 0).all() for g in got)
