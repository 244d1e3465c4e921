"""CPU checks of the mass check (rcmdyn_set_massck / rcmdyn_get_massck, include/rcmdyn.h): both
calls declared, exported and bound in the Python host and the Fortran shim, and the host class
MassCheck (regcm_amd/massck.py) against a line-by-line transcription of the scalar part of the
reference's massck (Main/mod_massck.F90:309-364), bit for bit.  No compute call is made."""
import ctypes
import os
import re
import subprocess

import numpy as np

from regcm_amd import dycore
from regcm_amd.massck import MassCheck, e12_5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rcmdyn.h")
FDIR = os.path.join(ROOT, "regcm_amd", "fortran")
CALLS = ["rcmdyn_set_massck", "rcmdyn_get_massck"]


def test_massck_calls_declared_exported_and_bound():
    src = open(HEADER).read()
    L = dycore.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dycore.LIB_PATH], capture_output=True, text=True).stdout
    for n in CALLS:
        assert re.search(rf"^int {n}\(rcmdyn_t\* h", src, re.M), n
        assert n in dycore.EXPORTED
        assert re.search(rf"\bT {n}$", nm, re.M), n
    i32, dp, P = ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    assert L.rcmdyn_set_massck.argtypes == [P, i32, i32]
    assert L.rcmdyn_get_massck.argtypes == [P, dp, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_int64)]
    assert re.search(r"^int rcmdyn_set_massck\(rcmdyn_t\* h, int32_t on, int32_t cap\);", src, re.M)
    assert re.search(r"^int rcmdyn_get_massck\(rcmdyn_t\* h, double\* out, int32_t cap, int32_t\* count, "
                     r"int64_t\* lost\);", src, re.M)
    for m in ("set_massck", "get_massck"):
        assert callable(getattr(dycore.DynCore, m)), m
    assert dycore.MASSCK_COLUMNS == ("lcount", "dt", "drymass", "dryadv", "qmass", "qadv")
    assert re.search(r"^#define RCMDYN_ABI_VERSION 6$", src, re.M)          # no ABI bump


def test_massck_calls_in_the_fortran_shim():
    f90 = open(os.path.join(FDIR, "mod_gpu_dyn.F90")).read()
    for n in CALLS:
        assert re.search(rf"bind\(c, name='{n}'\)", f90), n
        assert re.search(rf"public ::.*\b{n}\b", f90), n
    shim = open(os.path.join(FDIR, "test_shim.F90")).read()
    for n in CALLS:
        assert re.search(rf"ierr = {n}\(h,", shim), n
    subprocess.run(["make", "-s", "-B", "-C", FDIR], check=True)      # the shim still builds
    assert os.path.exists(os.path.join(FDIR, "test_shim"))


class Transcription:
    """Main/mod_massck.F90:309-364 with the module variables (:47-50) and the saved means (:61-65),
    one Python statement per Fortran statement, in double precision (wrkp = rk8).  The sumall
    calls are the identity on one rank; myid == italk."""

    def __init__(self):
        self.dryini = 0.0
        self.watini = 0.0
        self.dryerror = 0.0
        self.waterror = 0.0
        self.mcrai = 0.0
        self.mncrai = 0.0
        self.mevap = 0.0
        self.mdryadv = 0.0
        self.mqadv = 0.0

    def massck(self, dt, tdrym, tdadv, tqmass, tqadv, tcrai, tncrai, tqeva, start, alarm):
        w2 = dt / 86400.0                                     # :69
        w1 = 1.0 - w2                                         # :70
        drymass = tdrym                                       # :309
        qmass = tqmass                                        # :310
        if start:                                             # :312
            self.dryerror = 0.0
            self.waterror = 0.0
            self.dryini = drymass
            self.watini = qmass
            return None                                       # :319
        qadv = tqadv                                          # :322
        dryadv = tdadv
        craim = tcrai
        ncraim = tncrai
        evapm = tqeva                                         # :326
        self.mcrai = w1 * self.mcrai + w2 * craim             # :328
        self.mncrai = w1 * self.mncrai + w2 * ncraim
        self.mevap = w1 * self.mevap + w2 * evapm
        self.mdryadv = w1 * self.mdryadv + w2 * dryadv
        self.mqadv = w1 * self.mqadv + w2 * qadv              # :332
        drymass = drymass - dryadv                            # :335
        qmass = qmass + craim + ncraim - qadv - evapm         # :336
        if self.dryini < 1.0e-20:                             # :337
            self.dryini = drymass
        if self.watini < 1.0e-20:                             # :338
            self.watini = qmass
        self.dryerror = self.dryerror + ((drymass - self.dryini) / self.dryini * 100.0) * dt / 86400.0   # :339
        self.waterror = self.waterror + ((qmass - self.watini) / self.watini * 100.0) * dt / 86400.0    # :341
        out = None
        if alarm:                                             # :343
            out = (drymass, self.dryerror, qmass, self.waterror, self.mdryadv, self.mqadv, self.mcrai,
                   self.mncrai, self.mevap)
            self.dryerror = 0.0                               # :359
            self.waterror = 0.0
        self.dryini = drymass                                 # :362
        self.watini = qmass
        return out

    def scalars(self):
        return (self.dryini, self.watini, self.dryerror, self.waterror, self.mcrai, self.mncrai, self.mevap,
                self.mdryadv, self.mqadv)


def records():
    """Ten made-up records with masses of a 3000-km domain's order, fluxes of both signs, non-zero
    rain and evaporation; the second starts from dryini = 0 (a restarted run: :337-338), the
    fifth and the last are report steps."""
    rng = np.random.Generator(np.random.PCG64(20))
    out = []
    for q in range(10):
        dt = 150.0 if q < 2 else 300.0
        rec = np.array([q, dt, 8.9e16 * (1.0 + 1e-7 * rng.standard_normal()), 3.1e11 * rng.standard_normal(),
                        2.4e14 * (1.0 + 1e-5 * rng.standard_normal()), 7.7e9 * rng.standard_normal()])
        rain = (1.3e9 * rng.random(), 2.9e9 * rng.random(), 3.3e9 * rng.random())
        out.append((rec, rain))
    return out


def test_masscheck_matches_the_transcription_bit_for_bit():
    mc, tr = MassCheck(), Transcription()
    seen_report = 0
    for q, (rec, (crai, ncrai, evap)) in enumerate(records()):
        first, report = q == 0, q in (4, 9)
        if q == 1:                                # the re-seeding branch: dryini, watini below dlowval
            mc.dryini = mc.watini = 0.0
            tr.dryini = tr.watini = 0.0
        lines = mc.update(rec, crai=crai, ncrai=ncrai, evap=evap, first=first, report=report, when="step %d" % q)
        want = tr.massck(rec[1], rec[2], rec[3], rec[4], rec[5], crai, ncrai, evap, first, report)
        got = (mc.dryini, mc.watini, mc.dryerror, mc.waterror, mc.mcrai, mc.mncrai, mc.mevap, mc.mdryadv, mc.mqadv)
        assert got == tr.scalars(), q             # float equality: bit for bit (no NaN, no -0.0 here)
        if first:
            assert lines is None and want is None
            assert mc.dryini == rec[2] and mc.watini == rec[4] and mc.mdryadv == 0.0
        elif report:
            seen_report += 1
            assert mc.dryerror == 0.0 and mc.waterror == 0.0
            assert len(lines) == 11 and "MASS CHECK" in lines[0] and lines[1] == " At step %d" % q
            assert lines[2] == " Total dry air   =%s kg, error = %9.5f %%" % (e12_5(want[0]), want[1])
            assert lines[3] == " Total water     =%s kg, error = %9.5f %%" % (e12_5(want[2]), want[3])
            for line, v in zip(lines[5:10], want[4:]):
                assert line.endswith("= %s kg." % e12_5(v)), line
        else:
            assert lines is None and want is None
            if q > 1:
                assert mc.dryerror != 0.0 and mc.waterror != 0.0       # the errors accumulate
    assert seen_report == 2 and mc.mcrai > 0.0 and mc.mevap > 0.0


def test_e12_5_is_the_fortran_edit_descriptor():
    assert e12_5(0.0) == " 0.00000E+00"
    assert e12_5(8.9e16) == " 0.89000E+17"
    assert e12_5(-1234567.0) == "-0.12346E+07"
    assert e12_5(0.099999999) == " 0.10000E+00"
    assert e12_5(3.0e-5) == " 0.30000E-04"
