"""CPU checks of the output stream: the NumPy transcription the GPU tests measure against
(tests/output_ref.py) is held to a plain triple loop of the same Fortran text
(Main/mod_output.F90:226-452, 576, 933-941, 1057-1150), point by point in Python floats, on
17 x 19 x 6 and 37 x 29 x 18, both cores, with a band and a doubly periodic case; both branches of
the 100 m search are populated; the engine library exports the three entry points.

Python's float + - * / are the IEEE double operations, as NumPy's; the log of both sides is
np.log, so the two agree bit for bit.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from regcm_amd import constants as C
from regcm_amd.config import OUTPUT_FIELDS, SIGMA_TABLES
from tests import output_ref
from tests.condtq_ref import _A, _C, EP2, TZERO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the lowest layer of the 18-level table ends at sigma = 0.99 (some 80 m: below 100 m), the one
# of this six-level set at 0.98 (some 160 m: above)
SIGMA6 = np.array([0.0, 0.2, 0.45, 0.7, 0.9, 0.98, 1.0])
SHAPES = {
    "17x19x6": dict(jx=17, iy=19, kz=6, sigma=SIGMA6),
    "37x29x18": dict(jx=37, iy=29, kz=18, sigma=np.array(SIGMA_TABLES[18], dtype=np.float64)),
}
CORES = {"hydro": dict(idynamic=1), "nh": dict(idynamic=2), "band": dict(idynamic=1, i_band=1),
         "crm": dict(idynamic=2, i_band=1, i_crm=1)}


def make_case(shape, core, seed=3):
    """(rc, sigma, state, leftovers): a seeded state of plausible magnitudes, coupled with p*."""
    s = dict(SHAPES[shape])
    sigma = s.pop("sigma")
    rc = SimpleNamespace(ptop=5.0, rhmin=0.01, rhmax=1.01, i_band=0, i_crm=0, **s)
    for k, v in CORES[core].items():
        setattr(rc, k, v)
    rng = np.random.Generator(np.random.PCG64(seed))
    kz, shp = rc.kz, (rc.iy, rc.jx)
    r3 = lambda n, lo, hi: rng.uniform(lo, hi, (n,) + shp)
    psa = rng.uniform(80.0, 97.0, (1,) + shp)
    hs = 0.5 * (sigma[1:] + sigma[:-1])
    tprof = (215.0 + 75.0 * hs)[:, None, None]
    st = {"PSA": psa, "ATM1_T": (tprof + r3(kz, -3, 3)) * psa, "ATM1_QV": r3(kz, 1e-5, 1.5e-2) * psa,
          "ATM1_QC": r3(kz, 0, 1e-4) * psa, "ATM1_U": r3(kz, -25, 25) * psa, "ATM1_V": r3(kz, -25, 25) * psa,
          "ATM1_QI": r3(kz, 0, 1e-5) * psa, "ATM1_QR": r3(kz, 0, 1e-5) * psa, "ATM1_QS": r3(kz, 0, 1e-5) * psa,
          "ATM1_TKE": r3(kz + 1, 1e-3, 2.0)}
    pre = {"PSA": psa + rng.uniform(-0.05, 0.05, psa.shape)}
    if rc.idynamic == 2:
        zf = np.cumsum(r3(kz + 1, 30.0, 900.0)[::-1], axis=0)[::-1]                    # decreasing with k
        st.update({"ATM1_PP": r3(kz, -300, 300) * psa, "ATM1_W": r3(kz + 1, -1, 1) * psa,
                   "ATM0_PS": psa * 1000.0, "ATM0_PF": (sigma[:, None, None] * psa + rc.ptop) * 1000.0,
                   "ATM0_Z": 0.5 * (zf[1:] + zf[:-1])})
        pre.update({"ATM1_PP": st["ATM1_PP"] + r3(kz, -5, 5), "ATM0_PR": (hs[:, None, None] * psa + rc.ptop) * 1000.0})
    left = {"PR": output_ref.atm1_pr(rc, sigma, pre), "ATMS_ZQ": np.cumsum(r3(kz + 1, 50, 2000)[::-1], axis=0)[::-1],
            "ATMS_PF3D": r3(kz + 1, 5e3, 1e5), "OMEGA": r3(kz, -1e-3, 1e-3)}
    return rc, sigma, st, left


def names_of(rc):
    nh = rc.idynamic == 2
    return [n for n in OUTPUT_FIELDS if not (n in ("W", "PP") and not nh) and not (n in ("ZH", "ZF", "OMEGA") and nh)]


def pfwsat_point(t, p):
    """Share/pfesat.inc and Share/pfwsat.inc at one point."""
    td = min(max(t - TZERO, -75.0), 100.0)
    c = _A if td >= 0.0 else _C
    es = (c[0] + td * (c[1] + td * (c[2] + td * (c[3] + td * (c[4] + td * (c[5] + td * (c[6] + td * (c[7] + td * c[8])))))))) * 100.0
    return EP2 * (es / (p - es))


def loops(rc, sigma, st, names, left):
    """The Fortran text as a plain triple loop over k, i, j (1-based, as written there)."""
    kz, jx, iy, ptop, nh = rc.kz, rc.jx, rc.iy, rc.ptop, rc.idynamic == 2
    jci1, jci2 = (1, jx) if rc.i_band else (2, jx - 2)
    ici1, ici2 = (1, iy) if rc.i_crm else (2, iy - 2)
    rovg = C.rgas / C.egrav
    f = lambda n: (lambda j, i, k=1: float(st[n][k - 1, (i - 1) % iy, (j - 1) % jx]))   # the ghost line of a period wraps
    lf = lambda n: (lambda j, i, k: float(left[n][k - 1, i - 1, j - 1]))
    sig = lambda k: float(sigma[k - 1])
    psa, t, qv, u, v = f("PSA"), f("ATM1_T"), f("ATM1_QV"), f("ATM1_U"), f("ATM1_V")
    log = lambda x: float(np.log(np.float64(x)))
    out = {n: np.zeros((1 if n in output_ref.TWO_D else kz, iy, jx)) for n in names}
    branch = np.zeros((iy, jx), dtype=int)

    def xw(w, j, i, k):
        return 0.25 * (w(j, i, k) + w(j + 1, i, k) + w(j, i + 1, k) + w(j + 1, i + 1, k)) / psa(j, i)

    for i in range(ici1, ici2 + 1):
        for j in range(jci1, jci2 + 1):
            ps = psa(j, i)
            put = lambda n, k, x: out[n].__setitem__((k - 1, i - 1, j - 1), x)
            for k in range(1, kz + 1):
                for n in names:
                    if n == "T":
                        put(n, k, t(j, i, k) / ps)
                    elif n == "U":
                        put(n, k, xw(u, j, i, k))
                    elif n == "V":
                        put(n, k, xw(v, j, i, k))
                    elif n == "W":
                        put(n, k, 0.5 * (f("ATM1_W")(j, i, k + 1) + f("ATM1_W")(j, i, k)) / ps)
                    elif n == "PP":
                        put(n, k, f("ATM1_PP")(j, i, k) / ps)
                    elif n == "QV":
                        q = qv(j, i, k) / ps
                        put(n, k, q / (1.0 + q))
                    elif n in ("QC", "QI", "QR", "QS"):
                        put(n, k, f("ATM1_" + n)(j, i, k) / ps)
                    elif n == "TKE":
                        put(n, k, f("ATM1_TKE")(j, i, k))
                    elif n == "PH" and not nh:
                        put(n, k, (sig(k) * ps + ptop) * 1000.0)
                    elif n == "PH":
                        pp = f("ATM1_PP")
                        put(n, k, ptop * 1000.0 if k == 1 else
                            f("ATM0_PF")(j, i, k) + 0.5 * (pp(j, i, k - 1) + pp(j, i, k)) / ps)
                    elif n == "ZH":
                        cell = ptop / ps
                        lay = rovg * t(j, i, k) / ps * log((sig(k + 1) + cell) / (sig(k) + cell))
                        put(n, k, lay if k == kz else lf("ATMS_ZQ")(j, i, k + 1) + lay)
                    elif n == "RH":
                        put(n, k, 100.0 * min(rc.rhmax, max(rc.rhmin, (qv(j, i, k) / ps) /
                                                            pfwsat_point(t(j, i, k) / ps, lf("PR")(j, i, k)))))
                    elif n == "PF":
                        put(n, k, lf("ATMS_PF3D")(j, i, k))
                    elif n == "ZF":
                        put(n, k, lf("ATMS_ZQ")(j, i, k))
                    elif n == "OMEGA":
                        put(n, k, lf("OMEGA")(j, i, k) * 10.0)
            if "PS" in names:
                put("PS", 1, ps)
            if "PS_PA" in names:
                put("PS_PA", 1, f("ATM0_PS")(j, i) + ptop * 1000.0 + f("ATM1_PP")(j, i, kz) / ps if nh else 1000.0 * (ps + ptop))
            if "UA100" in names:
                cell = ptop / ps

                def layer(k):
                    tv = t(j, i, k) / ps * (1.0 + C.ep1 * qv(j, i, k) / ps)
                    return rovg * tv * log((sig(k + 1) + cell) / (sig(k) + cell))
                zz = f("ATM0_Z")(j, i, kz) if nh else layer(kz)
                if zz > 100.0:
                    put("UA100", 1, xw(u, j, i, kz))
                    put("VA100", 1, xw(v, j, i, kz))
                    branch[i - 1, j - 1] = 1
                else:
                    for k in range(kz - 1, 0, -1):
                        zz1 = f("ATM0_Z")(j, i, k) if nh else zz + layer(k)
                        if zz1 > 100.0:
                            ww = (100.0 - zz) / (zz1 - zz)
                            put("UA100", 1, ww * xw(u, j, i, k) + (1.0 - ww) * xw(u, j, i, k + 1))
                            put("VA100", 1, ww * xw(v, j, i, k) + (1.0 - ww) * xw(v, j, i, k + 1))
                            branch[i - 1, j - 1] = 2
                            break
                        zz = zz1
    return out, branch


_RESULTS = {}


def both(shape, core):
    key = (shape, core)
    if key not in _RESULTS:
        rc, sigma, st, left = make_case(shape, core)
        names = names_of(rc)
        _RESULTS[key] = (rc, names, output_ref.output_ref(rc, sigma, st, names, left), loops(rc, sigma, st, names, left))
    return _RESULTS[key]


@pytest.mark.parametrize("core", list(CORES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_transcription_equals_triple_loop(shape, core):
    rc, names, ref, (lp, _) = both(shape, core)
    for n in names:
        assert ref[n].shape == lp[n].shape, n
        assert np.array_equal(ref[n], lp[n]), (n, float(np.max(np.abs(ref[n] - lp[n]))))
        assert np.unique(lp[n][lp[n] != 0.0]).size > 1, n


def test_both_branches_of_the_100m_search():
    """The lowest half level above 100 m (first branch) and below it (the walk up the column): each
    is taken by whole cases of the hydrostatic core, by the choice of the lowest sigma, and both
    inside the NH cases; the transcription's own branch mask agrees with the loop's."""
    seen = set()
    for shape in SHAPES:
        for core in CORES:
            rc, _, ref, (_, branch) = both(shape, core)
            is_, js = output_ref.interior(rc)
            b = branch[is_, js]
            assert np.all(b > 0), (shape, core)               # every column found its level
            assert np.array_equal(ref["_Z100"][1], b == 1), (shape, core)
            seen |= {(core in ("hydro", "band"), int(x)) for x in np.unique(b)}
    assert seen == {(True, 1), (True, 2), (False, 1), (False, 2)}, seen


def test_library_exports_the_output_entry_points():
    """librcmdyn.so exports rcmdyn_set_output, rcmdyn_output_atm, rcmdyn_get_output, and the Python
    host binds them."""
    from regcm_amd import dycore
    lib = dycore.lib()
    for sym in ("rcmdyn_set_output", "rcmdyn_output_atm", "rcmdyn_get_output"):
        assert sym in dycore.EXPORTED, sym
        assert getattr(lib, sym) is not None, sym           # ctypes resolves the symbol or raises
    for m in ("set_output", "output_atm", "get_output"):
        assert callable(getattr(dycore.DynCore, m)), m
