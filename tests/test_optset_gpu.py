"""The default-set instances of k_momentum, k_scalars and k_update (compiled for the options
of C1-C4, regcm_amd/csrc/optset.hpp) against the generic instances of the same bodies
(RCMDYN_NO_OPTSET=1): the same bits in every output field, on one tile (47 cross points: a
partial last block in both directions) and on 2 x 2 tiles (interior edges, ghost rings, the
overlap parts), over 4 steps (both leapfrog dt values, both buffer parities); the change of
instance in the middle of a run; and the same kernel names and launch counts either way."""
import numpy as np
import pytest

from bench import output_fields
from tests.support import advance, case, engine, physics_tendencies

pytestmark = pytest.mark.gpu


def both(monkeypatch, rc, data, nproc):
    """(default dispatch, generic instances everywhere), started alike."""
    monkeypatch.delenv("RCMDYN_NO_OPTSET", raising=False)
    dflt = engine(rc, data, nproc=nproc)
    monkeypatch.setenv("RCMDYN_NO_OPTSET", "1")
    gen = engine(rc, data, nproc=nproc)
    monkeypatch.delenv("RCMDYN_NO_OPTSET")
    return dflt, gen


def assert_same(a, b, rc):
    for name in output_fields(rc):
        assert np.array_equal(a.get(name), b.get(name)), name


@pytest.mark.parametrize("nproc", [(1, 1), (2, 2)], ids=str)
def test_default_set_instances_bit_identical(monkeypatch, nproc):
    rc, data, _ = case("C1")
    dflt, gen = both(monkeypatch, rc, data, nproc)
    for e in (dflt, gen):
        e.step(4)
    assert_same(dflt, gen, rc)


def test_drop_in_pair_bit_identical(monkeypatch):
    """tend + bdyval (k_update's launch outside rcmdyn_step's graph) on 2 x 2 tiles."""
    rc, data, _ = case("C1")
    dflt, gen = both(monkeypatch, rc, data, (2, 2))
    for e in (dflt, gen):
        advance(e, "pair", 4)
    assert_same(dflt, gen, rc)


def test_instance_changes_mid_run(monkeypatch):
    """Default-set steps, then an export attached (generic) and detached (default set again),
    then the seam's physics tendencies attached (generic from there on: the engine keeps the
    seam's buffers once put), bit for bit against a run on the generic instances throughout.
    Every attach and detach invalidates the captured graphs, so each stretch is captured with
    the instance its arguments select."""
    rc, data, _ = case("C1")
    phy = physics_tendencies(rc)
    dflt, gen = both(monkeypatch, rc, data, (1, 1))
    exported = []
    for e in (dflt, gen):
        e.step(2)
        e.set_diagnostics(True)
        e.step(1)
        exported.append({name: e.get(name) for name in ("TTEN", "UTEN", "QVTEN", "OMEGA")})
        e.set_diagnostics(False)
        e.step(2)
        advance(e, "physics", 2, phy)
        e.step(2)
    assert_same(dflt, gen, rc)
    for name, a in exported[0].items():       # the export's own fields, written in the generic stretch
        assert np.array_equal(a, exported[1][name]), name


def test_kernel_names_and_launch_counts(monkeypatch):
    """rcmdyn_kernel_times reports either instance under the one name of its kernel."""
    rc, data, _ = case("C1")
    dflt, gen = both(monkeypatch, rc, data, (1, 1))
    kd, kg = dflt.kernel_times(2), gen.kernel_times(2)
    assert {n: c for n, (c, _) in kd.items()} == {n: c for n, (c, _) in kg.items()}
    assert "k_update" in kd and "k_columns<false>" in kd
    assert not any(n.endswith("_gen") or "_gen<" in n for n in list(kd) + list(kg))
