"""rcmdyn_put / rcmdyn_get per field id: which calls an engine admits and with which message it
refuses the others, how many levels a field has, and that a put lands where a get reads it.

The expectation is a model of include/rcmdyn.h's field comments, written from config.py's
named lists; nothing is read out of the engine.  Every field meets a fresh engine of each
configuration (get, put of zeros, get again); then one engine takes all of them in enum order
and another in reverse order, and the model keeps the state the header describes: the physics,
bdyin and TKEPHY buffers exist from the first accepted put of one of their fields on, the slice
fields from rcmdyn_tend_pre_physics on, the tendency diagnostics with rcmdyn_set_diagnostics.
A refused put changes nothing.

Where the engine and the header's comments part, the expectation follows the engine:
 - a get of a field whose buffer this engine does not hold reports 'unknown field': the NH
   fields on a hydrostatic engine, the XxB_B1 record and ATM0_PSDOT before the first put of
   one of them, and on a hydrostatic engine XPPB_B1, XWWB_B1, ATM0_PSDOT, PPPHY and WPHY even
   after the other fields of their group were put;
 - XPSB_B1 cannot be put on the NH core ('reads no ps record'), but once another record field
   was put a get of it succeeds (zeros);
 - a put of ATMS_QXB3D_* is 'read-only' on every engine, a get of it without nqx = 5 names
   nqx.
No step is run apart from one rcmdyn_tend_pre_physics; exact comparisons throughout.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from regcm_amd import icbc
from regcm_amd.config import (ATMS_FIELDS, BDY_FIELDS, CONFIGS, FIELD, FIELD_NAMES, NH_BDY_FIELDS,
                              NH_PHY_FIELDS, NH_STATE_FIELDS, NH_STATIC_FIELDS, PHY_FIELDS, QX_ATMS_FIELDS,
                              QX_PHY_FIELDS, QX_STATE_FIELDS, STATE_FIELDS, STATIC_FIELDS, TKE_STATE_FIELDS,
                              field_levels)

pytestmark = pytest.mark.gpu

# the groups of include/rcmdyn.h's enum comments that config.py does not name
READ_ONLY_DIAG = ["PSC", "PTEN", "PSDOTA", "QDOT", "PHI"]
TEND_DIAG = ["TTEN", "UTEN", "VTEN", "QVTEN", "QCTEN", "OMEGA", "XKC"]      # rcmdyn_set_diagnostics
BDYIN_FIELDS = ["XUB_B1", "XVB_B1", "XTB_B1", "XQB_B1", "XPSB_B1", "XPPB_B1", "XWWB_B1", "ATM0_PSDOT"]
NH_BDYIN_FIELDS = ["XPPB_B1", "XWWB_B1", "ATM0_PSDOT"]
TKE_FIELDS = TKE_STATE_FIELDS + ["TKEPHY", "KPBL"]
HYDRO_ONLY_ATMS = ["ATMS_ZQ", "ATMS_ZA", "ATMS_DZQ"]

NH_ONLY = set(NH_STATE_FIELDS + NH_BDY_FIELDS + NH_STATIC_FIELDS + NH_PHY_FIELDS + NH_BDYIN_FIELDS)
NQX5_PUT = set(QX_STATE_FIELDS + QX_PHY_FIELDS)
NQX5 = NQX5_PUT | set(QX_ATMS_FIELDS)
NO_PUT = set(READ_ONLY_DIAG + TEND_DIAG + ATMS_FIELDS + QX_ATMS_FIELDS)
ALL_PHY = set(PHY_FIELDS + NH_PHY_FIELDS + QX_PHY_FIELDS)

P_READONLY = "rcmdyn_put: field is read-only or unknown"
P_NQX = "rcmdyn_put: qi/qr/qs fields need nqx = 5 (ipptls = 2)"
P_TKE = "rcmdyn_put: TKE/kpbl fields need ibltyp=2 (UW PBL)"
P_KPBL_KZ = "rcmdyn_put: kpbl is greater than kz"
P_KPBL_INT = "rcmdyn_put: kpbl must hold integers"
P_NH = "rcmdyn_put: non-hydrostatic field on a hydrostatic engine"
P_NOPS = "rcmdyn_put: the non-hydrostatic core reads no ps record (p* is atm0%ps)"
G_DIAG = "rcmdyn_get: tendency diagnostics are off (rcmdyn_set_diagnostics)"
G_SLICE = "rcmdyn_get: no slice fields yet (rcmdyn_tend_pre_physics)"
G_ZQ = "rcmdyn_get: zq/za/dzq are not computed by mkslice for idynamic=2"
G_PHY = "rcmdyn_get: no physics tendencies were put"
G_NQX = "rcmdyn_get: qi/qr/qs fields need nqx = 5 (ipptls = 2)"
G_TKE = "rcmdyn_get: TKE/kpbl fields need ibltyp=2 (UW PBL)"
G_TKEPHY = "rcmdyn_get: no TKE tendency was put"
G_UNKNOWN = "rcmdyn_get: unknown field"


def test_the_lists_cover_the_enum():
    groups = [STATE_FIELDS, STATIC_FIELDS, BDY_FIELDS, READ_ONLY_DIAG, TEND_DIAG, NH_STATE_FIELDS, NH_BDY_FIELDS,
              NH_STATIC_FIELDS, PHY_FIELDS, NH_PHY_FIELDS, ATMS_FIELDS, BDYIN_FIELDS, TKE_FIELDS, QX_STATE_FIELDS,
              QX_PHY_FIELDS, QX_ATMS_FIELDS]
    assert sorted(n for g in groups for n in g) == sorted(FIELD_NAMES)
    assert len(ATMS_FIELDS) == 22


_SMALL = dict(jx=24, iy=20, nspgx=None, nspgd=None)
ENGINES = {
    "hydro": dataclasses.replace(CONFIGS["C1"], **_SMALL),
    "hydro_full": dataclasses.replace(CONFIGS["C1"], ipptls=2, ibltyp=2, iuwvadv=1, **_SMALL),
    "nh": dataclasses.replace(CONFIGS["N1"], **_SMALL),
    "nh_full": dataclasses.replace(CONFIGS["N1"], ipptls=2, ibltyp=2, **_SMALL),
}


@pytest.fixture(scope="module")
def cases():
    """{engine name: (RunConfig, generated split constants and start state)}, made once."""
    out = {}
    for key, rc in ENGINES.items():
        out[key] = (rc, (icbc.generate_nh if rc.idynamic == 2 else icbc.generate)(rc))
    return out


def engine(case, nproc=(1, 1)):
    from regcm_amd.dycore import DynCore
    rc, data = case
    return DynCore(rc, data["split"], nproc_j=nproc[0], nproc_i=nproc[1])


class Model:
    """What the header says an engine of this configuration answers, and the state it keeps."""

    def __init__(self, rc):
        self.nh = rc.idynamic == 2
        self.nqx5 = rc.nqx == 5
        self.uw = rc.ibltyp == 2
        self.physics = self.bdyin = self.tkephy = self.slice = self.diag = False

    def put(self, name):
        """The refusal of a put of valid values, or None; an accepted put allocates its group."""
        if name in NO_PUT:
            return P_READONLY
        if name in NQX5_PUT and not self.nqx5:
            return P_NQX
        if name in TKE_FIELDS and not self.uw:
            return P_TKE
        if name in NH_ONLY and not self.nh:
            return P_NH
        if name == "XPSB_B1" and self.nh:
            return P_NOPS
        if name in ALL_PHY:
            self.physics = True
        if name in BDYIN_FIELDS:
            self.bdyin = True
        if name == "TKEPHY":
            self.tkephy = True
        return None

    def get(self, name):
        if name in TEND_DIAG and not self.diag:
            return G_DIAG
        if name in ATMS_FIELDS:
            if not self.slice:
                return G_SLICE
            if self.nh and name in HYDRO_ONLY_ATMS:
                return G_ZQ
        if name in PHY_FIELDS + NH_PHY_FIELDS and not self.physics:
            return G_PHY
        if name in NQX5:
            if not self.nqx5:
                return G_NQX
            if name in QX_PHY_FIELDS and not self.physics:
                return G_PHY
            if name in QX_ATMS_FIELDS and not self.slice:
                return G_SLICE
        if name in TKE_FIELDS:
            if not self.uw:
                return G_TKE
            if name == "TKEPHY" and not self.tkephy:
                return G_TKEPHY
        # no buffer on this engine
        if name in NH_ONLY and not self.nh:
            return G_UNKNOWN
        if name in BDYIN_FIELDS and not self.bdyin:
            return G_UNKNOWN
        return None


def raw_put(e, fid, arr, j1=1, i1=1, k1=1):
    from regcm_amd.dycore import lib
    a = np.ascontiguousarray(arr, dtype=np.float64)
    nk, ni, nj = a.shape
    rc = lib().rcmdyn_put(e.h, fid, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                          j1, j1 + nj - 1, i1, i1 + ni - 1, k1, k1 + nk - 1)
    return lib().rcmdyn_last_error(e.h).decode() if rc else None


def raw_get(e, fid, nk):
    """(refusal or None, the (nk, iy, jx) box 1..jx x 1..iy x 1..nk, NaN where nothing was written)"""
    from regcm_amd.dycore import lib
    out = np.full((nk, e.rc.iy, e.rc.jx), np.nan)
    rc = lib().rcmdyn_get(e.h, fid, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                          1, e.rc.jx, 1, e.rc.iy, 1, nk)
    return (lib().rcmdyn_last_error(e.h).decode() if rc else None), out


def levels_written(e, name):
    """Levels a get of k = 1..kz+2 fills: whole planes, from k = 1 on, nothing above."""
    err, out = raw_get(e, FIELD[name], e.rc.kz + 2)
    assert err is None, (name, err)
    full = [not np.isnan(out[k]).any() for k in range(out.shape[0])]
    none = [np.isnan(out[k]).all() for k in range(out.shape[0])]
    n = sum(full)
    assert full[:n] == [True] * n and none[n:] == [True] * (len(full) - n), name
    return n


@pytest.mark.parametrize("order", ["fresh", "enum", "reverse"])
@pytest.mark.parametrize("key", list(ENGINES))
def test_admissibility_matrix(cases, key, order):
    """fresh: a new engine for every field; enum, reverse: one engine takes them all in turn."""
    rc = cases[key][0]
    e, m = engine(cases[key]), Model(rc)
    got, want = {}, {}
    for name in (FIELD_NAMES[::-1] if order == "reverse" else FIELD_NAMES):
        if order == "fresh":
            e.close()
            e, m = engine(cases[key]), Model(rc)
        nk = field_levels(name, rc.kz, rc.nsplit)
        zeros = np.zeros((nk, rc.iy, rc.jx))
        want[name] = (m.get(name), m.put(name), m.get(name))
        got[name] = (raw_get(e, FIELD[name], nk)[0], raw_put(e, FIELD[name], zeros), raw_get(e, FIELD[name], nk)[0])
    bad = {n: (got[n], want[n]) for n in got if got[n] != want[n]}
    assert not bad, bad
    # every field this engine now reads has the host's level count
    for name in FIELD_NAMES:
        if m.get(name) is None:
            assert levels_written(e, name) == field_levels(name, rc.kz, rc.nsplit), name
    e.close()


def test_every_message_is_met(cases):
    """The matrix above meets every refusal the two calls have (the KPBL value checks are in
    test_ids_out_of_range_and_kpbl_values), in both states of every lazily allocated group."""
    seen = set()
    for key, (rc, _) in cases.items():
        for order in (FIELD_NAMES, FIELD_NAMES[::-1]):
            m = Model(rc)
            for name in order:
                seen.update((m.get(name), m.put(name), m.get(name)))
            m.slice = m.diag = True
            seen.update(m.get(name) for name in FIELD_NAMES)
    assert seen == {None, P_READONLY, P_NQX, P_TKE, P_NH, P_NOPS, G_DIAG, G_SLICE, G_ZQ, G_PHY, G_NQX, G_TKE,
                    G_TKEPHY, G_UNKNOWN}


def test_which_message_wins(cases):
    """Fields two refusals apply to, on the plain hydrostatic engine (nqx = 2, ibltyp = 1)."""
    rc = cases["hydro"][0]
    e = engine(cases["hydro"])
    z = np.zeros((rc.kz + 1, rc.iy, rc.jx))
    # nqx before 'no physics tendencies were put'; read-only before nqx
    assert raw_get(e, FIELD["QIPHY"], rc.kz)[0] == G_NQX
    assert raw_put(e, FIELD["QIPHY"], z[:rc.kz]) == P_NQX
    assert raw_put(e, FIELD["ATMS_QXB3D_QI"], z[:rc.kz]) == P_READONLY
    assert raw_get(e, FIELD["ATMS_QXB3D_QI"], rc.kz)[0] == G_NQX
    # ibltyp before 'no TKE tendency was put'
    assert raw_get(e, FIELD["TKEPHY"], rc.kz + 1)[0] == G_TKE
    # 'no physics tendencies were put' before the missing NH buffer, which shows once TPHY is put
    assert raw_get(e, FIELD["WPHY"], rc.kz + 1)[0] == G_PHY
    assert raw_put(e, FIELD["WPHY"], z) == P_NH
    assert raw_put(e, FIELD["TPHY"], z[:rc.kz]) is None
    assert raw_get(e, FIELD["WPHY"], rc.kz + 1)[0] == G_UNKNOWN
    # no slice fields before the NH refusal of zq
    n = engine(cases["nh"])
    assert raw_get(n, FIELD["ATMS_ZQ"], rc.kz + 1)[0] == G_SLICE
    # ibltyp before the KPBL value check
    assert raw_put(e, FIELD["KPBL"], np.full((1, rc.iy, rc.jx), rc.kz + 1.0)) == P_TKE
    e.close()
    n.close()


def test_ids_out_of_range_and_kpbl_values(cases):
    rc = cases["hydro_full"][0]
    e = engine(cases["hydro_full"])
    z = np.zeros((1, rc.iy, rc.jx))
    for fid in (-1, len(FIELD_NAMES)):
        assert raw_put(e, fid, z) == P_READONLY
        assert raw_get(e, fid, 1)[0] == G_UNKNOWN
    k = np.full((1, rc.iy, rc.jx), float(rc.kz))
    assert raw_put(e, FIELD["KPBL"], k) is None
    k[0, 7, 5] = rc.kz + 1.0
    assert raw_put(e, FIELD["KPBL"], k) == P_KPBL_KZ
    k[0, 7, 5] = 2.5
    assert raw_put(e, FIELD["KPBL"], k) == P_KPBL_INT
    # the refused puts wrote nothing
    assert np.array_equal(e.get("KPBL"), np.full((1, rc.iy, rc.jx), float(rc.kz)))
    e.close()


@pytest.mark.parametrize("key", ["hydro_full", "nh"])
def test_after_pre_physics_and_diagnostics(cases, key):
    """With the start state put, one rcmdyn_tend_pre_physics and the diagnostics on, the slice
    fields and the tendencies are read, with the host's level counts."""
    rc, data = cases[key]
    e, m = engine(cases[key]), Model(rc)
    st = dict(data["state"])
    if rc.nqx == 5:
        st.update(icbc.hydrometeor_state(rc, st, nqx=5))
    if rc.ibltyp == 2:
        st.update(icbc.tke_state(rc))
    e.put_state(st)
    e.bdyval()
    e.set_diagnostics(True)
    e.tend_pre_physics()
    m.slice = m.diag = True
    got, want = {}, {}
    for name in FIELD_NAMES:
        nk = field_levels(name, rc.kz, rc.nsplit)
        want[name] = m.get(name)
        got[name] = raw_get(e, FIELD[name], nk)[0]
    bad = {n: (got[n], want[n]) for n in got if got[n] != want[n]}
    assert not bad, bad
    for name in TEND_DIAG + ATMS_FIELDS + (QX_ATMS_FIELDS if rc.nqx == 5 else []):
        if want[name] is None:
            assert levels_written(e, name) == field_levels(name, rc.kz, rc.nsplit), name
        else:
            assert want[name] == G_ZQ and name in HYDRO_ONLY_ATMS
    e.close()


def ramp(name, rc, sign=1.0):
    """value = 10000 k + 100 i + j (Fortran indices), exact in fp64; KPBL holds integers <= kz."""
    nk = field_levels(name, rc.kz, rc.nsplit)
    k, i, j = np.meshgrid(np.arange(1, nk + 1), np.arange(1, rc.iy + 1), np.arange(1, rc.jx + 1), indexing="ij")
    if name == "KPBL":
        return ((7 * i + j + (3 if sign < 0 else 0)) % (rc.kz + 1)).astype(np.float64)
    return sign * (10000.0 * k + 100.0 * i + j)


@pytest.mark.parametrize("key,nproc", [("hydro", (1, 1)), ("hydro_full", (1, 1)), ("nh", (1, 1)), ("nh_full", (1, 1)),
                                       ("hydro_full", (2, 2)), ("nh_full", (2, 2))])
def test_round_trip(cases, key, nproc):
    rc = cases[key][0]
    e, m = engine(cases[key], nproc), Model(rc)
    writable = [n for n in FIELD_NAMES if m.put(n) is None]
    assert set(STATE_FIELDS + STATIC_FIELDS + BDY_FIELDS + PHY_FIELDS + ["XUB_B1"]) <= set(writable)
    for name in writable:
        full = ramp(name, rc)
        e.put(name, full)
        assert np.array_equal(e.get(name), full), name
    # a box with j1, i1, k1 > 1 (k1 = 1 where the field has one level), across the tile seams of
    # the 2 x 2 tiling (j = 12 | 13, i = 10 | 11), leaves the rest as it was; every field still
    # holds its own ramp after all the other puts
    j1, i1 = 3, 4
    for name in writable:
        full = ramp(name, rc)
        assert np.array_equal(e.get(name), full), name
        nk = full.shape[0]
        k1 = 2 if nk > 1 else 1
        box = ramp(name, rc, -1.0)[k1 - 1:max(nk - 1, 1), i1 - 1:rc.iy - 2, j1 - 1:rc.jx - 5]
        e.put(name, box, j1=j1, i1=i1, k1=k1)
        full[k1 - 1:max(nk - 1, 1), i1 - 1:rc.iy - 2, j1 - 1:rc.jx - 5] = box
        assert np.array_equal(e.get(name), full), name
    e.close()
