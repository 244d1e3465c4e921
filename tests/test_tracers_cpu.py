"""CPU checks of the chemical tracers' interface (rcmdyn_set_tracers, rcmdyn_put_tracer,
rcmdyn_get_tracer, rcmdyn_put_tracer_nudge; include/rcmdyn.h): declared after the field enum with the
ABI version unchanged, exported, bound in the Python host and the Fortran shim with the header's enum
order; and the self-checks of the NumPy reference (tests/tracer_ref.py) the GPU tests compare with.
"""
import dataclasses
import os
import re

import numpy as np
import pytest

from regcm_amd import dycore
from regcm_amd.config import CONFIGS, MAXTR, TRACER_FIELD, TRACER_FIELDS
from tests import tracer_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rcmdyn.h")
ENTRY_POINTS = ["rcmdyn_set_tracers", "rcmdyn_put_tracer", "rcmdyn_get_tracer", "rcmdyn_put_tracer_nudge"]


def test_header_declares_the_family_after_the_field_enum():
    src = open(HEADER).read()
    end = src.index("RCMDYN_NFIELDS")
    assert "#define RCMDYN_ABI_VERSION 6" in src
    assert src.index("enum rcmdyn_tracer_field") > end
    for name in ENTRY_POINTS:
        assert re.search(rf"^int {name}\(", src, re.M), name
        assert src.index(f"int {name}(") > end, name
    m = re.search(r"#define RCMDYN_MAXTR (\d+)", src)
    assert m and int(m.group(1)) >= 16 and int(m.group(1)) == MAXTR
    assert src.index("#define RCMDYN_MAXTR") > end


def test_enum_order_python_and_fortran():
    src = open(HEADER).read()
    body = src.split("enum rcmdyn_tracer_field", 1)[1].split("}", 1)[0]
    names = [n for n in re.findall(r"RCMDYN_TR_(\w+)", body)]
    assert names == TRACER_FIELDS
    assert TRACER_FIELD == {n: q for q, n in enumerate(names)}
    f90 = open(os.path.join(ROOT, "regcm_amd", "fortran", "mod_gpu_dyn.F90")).read()
    ids = {m.group(1).upper(): int(m.group(2)) for m in re.finditer(r"\btr_(\w+)\s*=\s*(\d+)", f90)}
    assert ids == TRACER_FIELD
    assert re.search(r"rcmdyn_maxtr\s*=\s*%d\b" % MAXTR, f90)


def test_entry_points_exported_and_bound():
    L = dycore.lib()
    f90 = open(os.path.join(ROOT, "regcm_amd", "fortran", "mod_gpu_dyn.F90")).read()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
        assert name in dycore.EXPORTED
        assert f"bind(c, name='{name}')" in f90, name
        assert re.search(rf"public ::.*\b{name}\b", f90), name
    for method in ("set_tracers", "put_tracer", "get_tracer", "put_tracer_nudge"):
        assert callable(getattr(dycore.DynCore, method))


def test_create_message_points_to_set_tracers():
    """cfg.ichem = 1 stays refused at create (the struct has no ntr), naming the way in."""
    from regcm_amd import icbc
    rc = dataclasses.replace(CONFIGS["C1"], ichem=1)
    data = icbc.generate(CONFIGS["C1"])
    with pytest.raises(dycore.EngineError, match="ichem.*rcmdyn_set_tracers"):
        dycore.DynCore(rc, data["split"])


# ------------------------------------------------------------------------------- the reference's own checks
@pytest.mark.parametrize("shape,frac", [((24, 67), 0.5), ((70, 31), 0.85), ((17, 19), 0.15)])
def test_serial_fix_equals_the_plain_loop(shape, frac):
    """The reference's vectorised fix (independent negatives at once, dependent ones walked in order)
    against the text's triple loop, on random sign patterns dense enough for long chains."""
    jx, iy = shape
    rc = dataclasses.replace(CONFIGS["C1"], jx=jx, iy=iy, nspgx=None, nspgd=None)
    rng = np.random.default_rng(jx * 1000 + iy)
    cq = rng.uniform(0.0, 1.0, (3, iy, jx)) * np.where(rng.uniform(size=(3, iy, jx)) < frac, -1.0, 1.0)
    fixed, nneg, ndep = tr.serial_fix(cq, rc)
    assert nneg > 0 and ndep > 0
    assert np.array_equal(fixed, tr.serial_fix_loops(cq, rc))
    inner = fixed[:, 1:iy - 2, 1:jx - 2]
    assert (inner >= 0.0).all()
    ring = np.ones(cq.shape, dtype=bool)
    ring[:, 1:iy - 2, 1:jx - 2] = False
    assert np.array_equal(fixed[ring], cq[ring])


def test_relaxation_band_partitions_the_frame():
    """Each side's band is nspgx - 2 lines deep, the four sides meet on the diagonals without overlap,
    and ibnd counts the lines from the boundary (2 on the first interior line)."""
    rc = CONFIGS["C1"]
    side, ibnd = tr.relaxation_band(rc)
    n = rc.nspgx
    assert (side[0] == 0).all() and (side[:, 0] == 0).all() and (side[rc.iy - 2:] == 0).all()
    mid_j, mid_i = rc.jx // 2, rc.iy // 2
    assert list(side[1:n - 1, mid_j - 1]) == [1] * (n - 2) and list(ibnd[1:n - 1, mid_j - 1]) == list(range(2, n))
    assert list(side[mid_i - 1, 1:n - 1]) == [3] * (n - 2) and list(ibnd[mid_i - 1, 1:n - 1]) == list(range(2, n))
    assert side[rc.iy - 3, mid_j - 1] == 2 and ibnd[rc.iy - 3, mid_j - 1] == 2
    assert side[mid_i - 1, rc.jx - 3] == 4 and ibnd[mid_i - 1, rc.jx - 3] == 2
    assert side[n, n] == 0 and ((side > 0) == (ibnd >= 2)).all()


def test_chem_bdyval_lines_and_corners():
    """chib = chia over ice on the west / east lines (the corners with them) and over jci on the south /
    north lines; chia = chib0 + xt * chibt over ici (west / east) and jce (south / north)."""
    rc = CONFIGS["C1"]
    rng = np.random.default_rng(2)
    shape = (2, rc.iy, rc.jx)
    a1, a2, b0, bt = (rng.uniform(1.0, 2.0, shape) for _ in range(4))
    o1, o2 = a1.copy(), a2.copy()
    tr.chem_bdyval(rc, a1, a2, b0, bt, 300.0)
    b = b0 + 300.0 * bt
    assert a2[0, 0, 0] == o1[0, 0, 0] and a2[0, rc.iy - 2, rc.jx - 2] == o1[0, rc.iy - 2, rc.jx - 2]   # corners: copied
    assert a1[0, 0, 0] == b[0, 0, 0]                                                                   # and set (jce)
    assert a2[0, 5, 0] == o1[0, 5, 0] and a1[0, 5, 0] == b[0, 5, 0]
    assert a2[0, 0, 5] == o1[0, 0, 5] and a1[0, 0, 5] == b[0, 0, 5]
    assert a1[0, 5, 5] == o1[0, 5, 5] and a2[0, 5, 5] == o2[0, 5, 5]
    a1n, a2n = o1.copy(), o2.copy()
    tr.chem_bdyval(rc, a1n, a2n, b0, bt, 300.0, integrating=False)
    assert np.array_equal(a2n, o2) and np.array_equal(a1n, a1)
