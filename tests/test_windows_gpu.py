"""Every getter of the engine asked for a window smaller than the domain (the path behind them is
one, regcm_amd/csrc/engine.hip get_window and rcmdyn_get_output over csrc/window.hpp; its index
arithmetic alone is tests/test_window_cpu.py).

One engine of the 34 x 23 cut on 2 x 2 tiles runs one tend with the budget, condtq, two tracers,
cumtran, the tracer budget and the output stage on.  Each C entry point is then called through
ctypes for the whole domain and for two windows into NaN-filled buffers: one well inside, one that
starts at 2 and ends one short of the far ends, so it still holds points the interior-only getters
do not write.  Both cross both tile seams.  A window must equal the same slice of the whole-domain
answer bit for bit, the NaN left where the entry point writes nothing included; the whole-domain
answers are what the other GPU tests pin, and must be what the DynCore wrappers return."""
import numpy as np
import pytest

from regcm_amd.config import CUMTRAN_FIELD, FIELD, OUTPUT_FIELD, TRACER_DIAG_TERM, TRACER_FIELD
from regcm_amd.dycore import BUDGET_TERMS, CONDTQ_TERMS, lib
from tests import condtq_ref as cq
from tests import cumtran_ref as cu
from tests.support import case, engine
from tests.test_tracers_gpu import nudge_tables, put_tracers, smooth_tracers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    rc, data, st0 = case("C", jx=34, iy=23, nspgx=7, nspgd=7)
    e = engine(rc, data, cq.moist_state(rc, st0), nproc=(2, 2))
    e.set_budget(True)
    e.set_condtq(True, 1.0)
    e.put_rh0adj(cq.rh0adj_field(rc))
    e.set_tracers(2)
    put_tracers(e, smooth_tracers(rc, st0, 2))
    e.put_tracer_nudge(*nudge_tables(rc))
    e.set_cumtran(True, 1)
    for name, a in zip(("DOTRAN", "KTOP", "CLDFRA"), cu.inputs(rc)):
        e.put_cumtran(name, a)
    e.set_tracer_budget(True, 0.5, 0.25)
    e.set_output(True, 8)
    e.tend()
    yield rc, e
    e.close()


def raw(e, fn, lead, box, shape, dtype=np.float64):
    """fn(h, *lead, dst, *box) into a NaN-filled buffer of the shape."""
    out = np.full(shape, np.nan, dtype=dtype)
    rc = fn(e.h, *lead, out.ctypes.data_as(fn.argtypes[1 + len(lead)]), *box)
    assert rc == 0, lib().rcmdyn_last_error(e.h).decode()
    return out


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def hold(rc, e, fn, lead, nk, wrapper, dtype=np.float64, levels=None):
    """The whole-domain answer against the wrapper's, then both windows against its slices.  levels:
    the k1, k2 the windows pass (default: 2 .. nk - 1, a one-level field 1 .. 1)."""
    whole = raw(e, fn, lead, (1, rc.jx, 1, rc.iy, 1, nk), (nk, rc.iy, rc.jx), dtype)
    assert np.isfinite(whole).any()
    assert np.array_equal(np.nan_to_num(whole, nan=0.0), wrapper) and wrapper.dtype == dtype
    k1, k2 = levels or ((1, 1) if nk == 1 else (2, nk - 1))
    ka, kb = (0, 1) if nk == 1 else (k1 - 1, k2)
    for j1, j2, i1, i2 in ((3, rc.jx - 4, 4, rc.iy - 4), (2, rc.jx - 1, 2, rc.iy - 1)):
        assert 1 < j1 <= 17 < j2 < rc.jx and 1 < i1 <= 12 < i2 < rc.iy        # the seams 17 | 18 and 12 | 13 lie inside
        got = raw(e, fn, lead, (j1, j2, i1, i2, k1, k2), (kb - ka, i2 - i1 + 1, j2 - j1 + 1), dtype)
        want = whole[ka:kb, i1 - 1:i2, j1 - 1:j2]
        nd = int((bits(got) != bits(np.ascontiguousarray(want))).sum())
        print(f"{fn.__name__}{lead} window j {j1}..{j2} i {i1}..{i2} k {k1}..{k2}: {nd} cells differ, "
              f"{int(np.isnan(want).sum())} NaN")
        assert nd == 0
    return whole


@pytest.mark.parametrize("name", ["ATM1_T", "QDOT", "PSA"])
def test_get(run, name):
    """A kz, a kz + 1 and a 2-D field."""
    rc, e = run
    nk = {"ATM1_T": rc.kz, "QDOT": rc.kz + 1, "PSA": 1}[name]
    whole = hold(rc, e, lib().rcmdyn_get, (FIELD[name],), nk, e.get(name))
    assert not np.isnan(whole).any()


def test_get_budget(run):
    rc, e = run
    hold(rc, e, lib().rcmdyn_get_budget, (BUDGET_TERMS.index("T_ADV"),), rc.kz, e.get_budget("T_ADV"))


@pytest.mark.parametrize("term", ["RH0ADJ", "T"])
def test_get_condtq(run, term):
    """rh0adj on the owned points, the increments on the interior cross points alone: the wider
    window keeps its NaN on row iy - 1 and column jx - 1."""
    rc, e = run
    whole = hold(rc, e, lib().rcmdyn_get_condtq, (CONDTQ_TERMS.index(term),), rc.kz, e.get_condtq(term))
    assert np.isnan(whole[:, rc.iy - 2, 1:rc.jx - 1]).all() == (term == "T")
    assert not np.isnan(whole[:, 1:rc.iy - 2, 1:rc.jx - 2]).any()


def test_get_tracer(run):
    rc, e = run
    hold(rc, e, lib().rcmdyn_get_tracer, (TRACER_FIELD["ATM1"], 2), rc.kz, e.get_tracer("ATM1", 2))


def test_get_cumtran(run):
    """KTOP is level 1 whatever k1, k2 say (here 3, 2); CLDFRA has kz levels."""
    rc, e = run
    hold(rc, e, lib().rcmdyn_get_cumtran, (CUMTRAN_FIELD["KTOP"],), 1, e.get_cumtran("KTOP"), levels=(3, 2))
    hold(rc, e, lib().rcmdyn_get_cumtran, (CUMTRAN_FIELD["CLDFRA"],), rc.kz, e.get_cumtran("CLDFRA"))


def test_get_tracer_budget(run):
    rc, e = run
    hold(rc, e, lib().rcmdyn_get_tracer_budget, (TRACER_DIAG_TERM["ADVH"], 1), rc.kz, e.get_tracer_budget("ADVH", 1))


@pytest.mark.parametrize("prec", [4, 8])
def test_get_output(run, prec):
    """A 2-D and a 3-D field as floats and as doubles, from the compact pinned buffer: interior cross
    points alone."""
    rc, e = run
    dtype = np.float32 if prec == 4 else np.float64
    e.set_output(True, prec)
    e.output_atm(["PS", "T"])
    for name, nk in (("PS", 1), ("T", rc.kz)):
        whole = hold(rc, e, lib().rcmdyn_get_output, (OUTPUT_FIELD[name],), nk, e.get_output(name), dtype)
        assert np.isnan(whole[:, rc.iy - 2, :]).all() and not np.isnan(whole[:, 1:rc.iy - 2, 1:rc.jx - 2]).any()
