"""CPU checks of the CHE output stream: the NumPy transcription the GPU tests measure against
(tests/che_output_ref.py) is held to a plain quadruple loop of the same Fortran text
(Main/chemlib/mod_che_output.F90:74-83, 131-184; Main/chemlib/mod_che_tend.F90:561-571), point by
point in Python floats, on 17 x 19 x 6 and 37 x 29 x 18, plain and with a band; the engine library
exports the three entry points, the Python and Fortran hosts declare them, and the enum is the same
in the header, in Python and in Fortran.

Python's float + - * / are the IEEE double operations, as NumPy's, so the two agree bit for bit.
"""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from regcm_amd.config import CHE_FIELD, CHE_FIELDS, TRACER_DIAG_TERMS
from tests import che_output_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rcmdyn.h")
F90 = os.path.join(ROOT, "regcm_amd", "fortran", "mod_gpu_dyn.F90")
ENTRY_POINTS = ("rcmdyn_set_output_che", "rcmdyn_output_che", "rcmdyn_get_output_che")
SHAPES = {"17x19x6": dict(jx=17, iy=19, kz=6), "37x29x18": dict(jx=37, iy=29, kz=18)}
NTR = 3


def make_case(shape, band, seed=5):
    """(rc, cpsb, per-tracer inputs): seeded fields of plausible magnitudes, coupled with p*, the
    accumulators of both signs."""
    rc = SimpleNamespace(i_band=band, i_crm=0, **SHAPES[shape])
    rng = np.random.Generator(np.random.PCG64(seed))
    shp = (rc.kz, rc.iy, rc.jx)
    cpsb = rng.uniform(80.0, 97.0, (1, rc.iy, rc.jx))
    dzq = rng.uniform(40.0, 2500.0, shp)
    rhob = rng.uniform(0.1, 1.25, shp)
    tracers = []
    for _ in range(NTR):
        t = {"CHIA": rng.uniform(0.0, 2e-6, shp) * (rng.uniform(size=shp) < 0.5) * cpsb,
             "CHIB3D": rng.uniform(0.0, 2e-6, shp) * (rng.uniform(size=shp) < 0.6)}
        for n in cr.TERMS:
            t[n] = rng.normal(0.0, 1e-9, shp) * cpsb
        tracers.append(t)
    return rc, cpsb, dzq, rhob, tracers


def loops(rc, cpsb, dzq, rhob, tracers):
    """The Fortran text as a plain loop over itr, k, i, j (1-based, as written there)."""
    jci1, jci2 = (1, rc.jx) if rc.i_band else (2, rc.jx - 2)
    ici1, ici2 = 2, rc.iy - 2
    out = []
    for t in tracers:
        o = {n: np.zeros((rc.kz, rc.iy, rc.jx)) for n in ("MIXRAT",) + cr.TERMS}
        dtrace = np.zeros((rc.iy, rc.jx))
        for k in range(1, rc.kz + 1):
            for i in range(ici1, ici2 + 1):
                for j in range(jci1, jci2 + 1):
                    q = (k - 1, i - 1, j - 1)
                    ps = float(cpsb[0, i - 1, j - 1])
                    o["MIXRAT"][q] = float(t["CHIA"][q]) / ps
                    for n in cr.TERMS:
                        o[n][q] = float(t[n][q]) / ps
                    dtrace[i - 1, j - 1] = float(dtrace[i - 1, j - 1]) + \
                        float(t["CHIB3D"][q]) * float(dzq[q]) * float(rhob[q])
        o["BURDEN"] = np.zeros((1, rc.iy, rc.jx))
        for i in range(ici1, ici2 + 1):
            for j in range(jci1, jci2 + 1):
                o["BURDEN"][0, i - 1, j - 1] = float(dtrace[i - 1, j - 1]) * 1.0e6
        out.append(o)
    return out


@pytest.mark.parametrize("band", [0, 1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_transcription_equals_quadruple_loop(shape, band):
    rc, cpsb, dzq, rhob, tracers = make_case(shape, band)
    lp = loops(rc, cpsb, dzq, rhob, tracers)
    for t, want in zip(tracers, lp):
        got = {"MIXRAT": cr.mixrat(rc, t["CHIA"], cpsb), "BURDEN": cr.burden(rc, t["CHIB3D"], dzq, rhob)}
        got.update({n: cr.term(rc, t[n], cpsb) for n in cr.TERMS})
        assert sorted(got) == sorted(CHE_FIELDS)
        for n in CHE_FIELDS:
            assert got[n].shape == want[n].shape, n
            assert np.array_equal(got[n], want[n]), (n, float(np.max(np.abs(got[n] - want[n]))))
            assert np.unique(want[n][want[n] != 0.0]).size > 1, n
    # the division is not a product with the reciprocal: the two differ somewhere on these inputs
    t = tracers[0]
    assert not np.array_equal(cr.mixrat(rc, t["CHIA"], cpsb)[:, 1:-2, 1:-2], (t["CHIA"] * (1.0 / cpsb))[:, 1:-2, 1:-2])


def test_nh_dzq_is_the_difference_of_the_full_level_heights():
    zf = np.cumsum(np.arange(1.0, 8.0)[::-1])[::-1].reshape(7, 1, 1) * np.ones((7, 2, 3))
    d = cr.nh_dzq(zf)
    assert d.shape == (6, 2, 3) and np.array_equal(d[:, 0, 0], zf[:-1, 0, 0] - zf[1:, 0, 0]) and (d > 0).all()


def test_library_exports_and_hosts_declare_the_entry_points():
    """librcmdyn.so exports the three entry points the header declares; the Python host binds them and
    mod_gpu_dyn has an interface and a public statement for each."""
    from regcm_amd import dycore
    hdr, f90 = open(HEADER).read(), open(F90).read()
    lib = dycore.lib()
    for sym in ENTRY_POINTS:
        assert re.search(rf"^int {sym}\(rcmdyn_t\*", hdr, re.M), sym
        assert sym in dycore.EXPORTED, sym
        assert getattr(lib, sym) is not None, sym           # ctypes resolves the symbol or raises
        assert re.search(rf"function {sym}\(.*bind\(c, name='{sym}'\)", f90, re.S), sym
        assert re.search(rf"public ::.*\b{sym}\b", f90), sym
    for m in ("set_output_che", "output_che", "get_output_che"):
        assert callable(getattr(dycore.DynCore, m)), m
    assert lib.rcmdyn_get_output_che.argtypes[1:3] == lib.rcmdyn_get_tracer.argtypes[1:3]      # field, itr


def test_enum_is_the_same_in_header_python_and_fortran():
    hdr, f90 = open(HEADER).read(), open(F90).read()
    body = re.search(r"enum rcmdyn_che_field \{(.*?)\};", hdr, re.S).group(1)
    names = re.findall(r"RCMDYN_(\w+)", body)
    assert names[-1] == "NCHE" and "RCMDYN_CHE_MIXRAT = 0" in body
    assert [n[len("CHE_"):] for n in names[:-1]] == CHE_FIELDS
    assert [CHE_FIELD[n] for n in CHE_FIELDS] == list(range(len(CHE_FIELDS)))
    ids = {m.group(1).upper(): int(m.group(2)) for m in re.finditer(r"\bche_(\w+)\s*=\s*(\d+)", f90)}
    assert ids == CHE_FIELD
    assert int(re.search(r"rcmdyn_nche\s*=\s*(\d+)", f90).group(1)) == len(CHE_FIELDS)
    # the budget fields follow the accumulators' own order
    assert CHE_FIELDS[2:] == TRACER_DIAG_TERMS == list(cr.TERMS)
