"""The host-compiled regcm_amd/csrc/subex.hpp for the subex tests: builds tests/subex/subex_point.cpp
into a shared library in a temporary directory (once per process) and wraps its calls on NumPy
arrays.  A plain module (nothing collected)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "subex", "subex_point.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="subex_point_")
        so = os.path.join(_dir.name, "libsubex_point.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, SRC],
                       check=True)
        _lib = ctypes.CDLL(so)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def par_array(par):
    return np.array([par.rhmax, par.rhmin, par.tc0, float(par.larcticcorr), float(par.iconvlwp)])


def chis():
    out = np.zeros(256)
    lib().sx_chis(_p(out))
    return out


def pow10(x):
    x = _c(x)
    out = np.zeros(x.shape)
    lib().sx_pow10(ctypes.c_long(x.size), _p(x), _p(out))
    return out


def point(par, chis, t, p, qv, qc, rh, rho, rh0, cgul, cufra, culwc):
    """cldfrac + dqc at every point of equally shaped arrays: a dict fcc, cldfra, cldlwc, rh0adj, dqc, qcth."""
    ins = [_c(a) for a in (t, p, qv, qc, rh, rho, rh0, cgul, cufra, culwc)]
    assert all(a.shape == ins[0].shape for a in ins)
    names = ("fcc", "cldfra", "cldlwc", "rh0adj", "dqc", "qcth")
    out = {n: np.zeros(ins[0].shape) for n in names}
    lib().sx_point(ctypes.c_long(ins[0].size), _p(par_array(par)), _p(_c(chis)), *[_p(a) for a in ins],
                   *[_p(out[n]) for n in names])
    return out


def columns(par, dt, dtsec, rem, fcc, dqc, t, p, pf, qv, qc, rh, rho, psb, qck1, cevap, caccr, rainnc, lsmrnc, trrate):
    """The rain columns: 3-D arrays (kz, ...) (pf: kz + 1), 2-D arrays (...).  Returns a dict of the
    increments, the new accumulators, remrat / rembc and the final pptsum."""
    kz = t.shape[0]
    shp3, shp2 = t.shape, t.shape[1:]
    ncol = int(np.prod(shp2))
    in3 = [_c(a).reshape(-1) for a in (fcc, dqc, t, p, pf, qv, qc, rh, rho)]
    in2 = [_c(a).reshape(-1) for a in (psb, qck1, cevap, caccr)]
    out = {n: np.zeros(shp3) for n in ("lsc_t", "lsc_qv", "lsc_qc")}
    acc = {"rainnc": _c(rainnc).copy(), "lsmrnc": _c(lsmrnc).copy(), "trrate": _c(trrate).copy()}
    r3 = {n: np.zeros(shp3) for n in ("remrat", "rembc")}
    pptsum = np.zeros(shp2)
    lib().sx_columns(ctypes.c_long(ncol), ctypes.c_int(kz), _p(par_array(par)), ctypes.c_double(dt), ctypes.c_double(dtsec),
                     ctypes.c_int(1 if rem else 0), *[_p(a) for a in in3], *[_p(a) for a in in2],
                     _p(out["lsc_t"]), _p(out["lsc_qv"]), _p(out["lsc_qc"]), _p(acc["rainnc"]), _p(acc["lsmrnc"]),
                     _p(acc["trrate"]), _p(r3["remrat"]), _p(r3["rembc"]), _p(pptsum))
    out.update(acc)
    out.update(r3)
    out["pptsum"] = pptsum
    return out
