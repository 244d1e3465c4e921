"""The host-side selector of the hydrostatic tendency kernels' instances
(regcm_amd/csrc/optset.hpp): a stand-alone host program (tests/optset/optset_table.cpp, built
with the address and undefined-behaviour sanitizers) prints the instance for a table of
configurations.  The default option set of C1-C4 takes the default-set instances; every other
option, the budget, any export pointer, any physics-tendency pointer, kpbl and the switch
RCMDYN_NO_OPTSET take the generic ones."""
import dataclasses
import os
import shutil
import subprocess

import pytest

from regcm_amd.config import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, DEFAULT = 0, 1


def row(rc, budget=0, export=0, phys=0, kpbl=0):
    """One input line of the program for a RunConfig and the launch's optional pointers."""
    return (rc.iboudy, rc.idiffu, rc.ipgf, rc.isladvec, rc.ibltyp, rc.iuwvadv, rc.nqx - 2, budget, export,
            phys, kpbl)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("optset") / "optset_table"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "optset", "optset_table.cpp")], check=True)
    return str(exe)


def instances(program, rows, no_optset=False):
    env = {k: v for k, v in os.environ.items() if k != "RCMDYN_NO_OPTSET"}
    if no_optset:
        env["RCMDYN_NO_OPTSET"] = "1"
    text = "".join(" ".join(str(int(x)) for x in r) + "\n" for r in rows)
    out = subprocess.run([program], input=text, env=env, check=True, capture_output=True, text=True).stdout
    ids = [int(x) for x in out.split()]
    assert len(ids) == len(rows)
    return ids


def test_default_set_of_c1_to_c4(program):
    rows = [row(CONFIGS[name]) for name in ("C1", "C2", "C3", "C4")]
    assert instances(program, rows) == [DEFAULT] * 4


OTHER_OPTIONS = [{"idiffu": 2}, {"idiffu": 3}, {"iboudy": 0}, {"iboudy": 1}, {"iboudy": 3}, {"iboudy": 4},
                 {"ipgf": 1}, {"isladvec": 1}, {"ibltyp": 2, "iuwvadv": 1}, {"ibltyp": 2}, {"ipptls": 2}]


def test_every_other_option_is_generic(program):
    rows = [row(dataclasses.replace(CONFIGS["C3"], **over)) for over in OTHER_OPTIONS]
    # ibltyp = 2 with iuwvadv = 1 also as the launch sees it: xkcs exported and kpbl read
    rows.append(row(dataclasses.replace(CONFIGS["C3"], ibltyp=2, iuwvadv=1), export=7, kpbl=1))
    assert instances(program, rows) == [GENERIC] * len(rows)


def test_budget_and_optional_pointers_are_generic(program):
    rc = CONFIGS["C3"]
    rows = [row(rc, budget=1)]
    rows += [row(rc, export=n) for n in range(1, 8)]
    rows += [row(rc, phys=n) for n in range(1, 6)]
    rows += [row(rc, kpbl=1)]
    assert instances(program, rows) == [GENERIC] * len(rows)
    # and nothing attached is the default set again
    assert instances(program, [row(rc)]) == [DEFAULT]


def test_switch_gives_generic(program):
    rows = [row(CONFIGS[name]) for name in ("C1", "C2", "C3", "C4")]
    assert instances(program, rows, no_optset=True) == [GENERIC] * 4
