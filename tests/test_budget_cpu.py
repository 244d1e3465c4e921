"""CPU checks of the tendency-budget entry points (rcmdyn_set_budget, rcmdyn_get_budget,
rcmdyn_reset_budget; include/rcmdyn.h): declared, exported, bound in the Python host and in the
Fortran shim, with one order of the ten terms everywhere.  No compute call is made."""
import ctypes
import os
import re
import subprocess

from regcm_amd import dycore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rcmdyn.h")
FDIR = os.path.join(ROOT, "regcm_amd", "fortran")
CALLS = ["rcmdyn_set_budget", "rcmdyn_get_budget", "rcmdyn_reset_budget"]


def test_budget_calls_declared_exported_and_bound():
    src = open(HEADER).read()
    L = dycore.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dycore.LIB_PATH], capture_output=True, text=True).stdout
    for n in CALLS:
        assert re.search(rf"^int {n}\(rcmdyn_t\* h", src, re.M), n
        assert n in dycore.EXPORTED
        assert re.search(rf"\bT {n}$", nm, re.M), n
        assert getattr(L, n).argtypes is not None, n
    i32, dp, P = ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    assert L.rcmdyn_set_budget.argtypes == [P, i32, i32, ctypes.c_double]
    assert L.rcmdyn_get_budget.argtypes == [P, i32, dp] + [i32] * 6
    assert L.rcmdyn_reset_budget.argtypes == [P]
    for m in ("set_budget", "get_budget", "reset_budget"):
        assert callable(getattr(dycore.DynCore, m)), m


def test_budget_term_order_is_one_contract():
    """enum rcmdyn_budget_term (after RCMDYN_NFIELDS, so the field enum's parsers do not see it),
    dycore.BUDGET_TERMS and the Fortran constants."""
    src = open(HEADER).read()
    assert src.index("enum rcmdyn_budget_term") > src.index("RCMDYN_NFIELDS")
    body = src.split("enum rcmdyn_budget_term", 1)[1].split("}", 1)[0]
    names = re.findall(r"RCMDYN_BUD_(\w+)", body)
    assert names == dycore.BUDGET_TERMS and len(names) == 10
    assert re.search(r"RCMDYN_BUD_T_ADH = 0\b", body) and body.rstrip().endswith("RCMDYN_NBUDGET")
    f90 = open(os.path.join(FDIR, "mod_gpu_dyn.F90")).read().lower()
    ids = {m.group(1).upper(): int(m.group(2)) for m in re.finditer(r"\bbud_(\w+)\s*=\s*(\d+)", f90)}
    assert ids == {n: q for q, n in enumerate(names)}
    assert re.search(r"rcmdyn_nbudget\s*=\s*10\b", f90)
    assert dycore.IQV == 1                      # Main/mpplib/mod_runparams.F90:38


def test_budget_calls_in_the_fortran_shim():
    f90 = open(os.path.join(FDIR, "mod_gpu_dyn.F90")).read()
    for n in CALLS:
        assert re.search(rf"bind\(c, name='{n}'\)", f90), n
        assert re.search(rf"public ::.*\b{n}\b", f90), n
    subprocess.run(["make", "-s", "-B", "-C", FDIR], check=True)      # the shim still builds
    assert os.path.exists(os.path.join(FDIR, "test_shim"))
