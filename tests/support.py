"""What the GPU test files share: the error norms with the cross-grid crop, the generated cases,
"create, put the state, run bdyval" for the engine and the oracle, the state names of a
configuration, and the synthetic physics tendencies.  A plain module (no fixtures, nothing
collected); whatever belongs to one feature stays in that feature's test file.
"""
import dataclasses

import numpy as np

from regcm_amd import icbc
from regcm_amd.config import (CONFIGS, NH_PHY_FIELDS, NH_STATE_FIELDS, PHY_FIELDS, QX_STATE_FIELDS,
                              STATE_FIELDS, TKE_STATE_FIELDS, field_levels)

# the prognostic fields of the non-hydrostatic core: no dstor / hstor, pp and w instead
NH_FIELDS = STATE_FIELDS[:12] + NH_STATE_FIELDS

# the fields that live on the cross grid, among those the tests compare (the ATMS_* slice
# fields are compared whole)
CROSS = frozenset(
    ["ATM1_T", "ATM1_QV", "ATM1_QC", "ATM2_T", "ATM2_QV", "ATM2_QC", "PSA", "PSB", "DSTOR", "HSTOR",
     "PSC", "PTEN", "TTEN", "QVTEN", "QCTEN", "OMEGA", "QDOT", "XKC", "PHI",
     "ATM1_PP", "ATM2_PP", "ATM1_W", "ATM2_W", "ATM1_TKE", "ATM2_TKE"] + QX_STATE_FIELDS)


# ------------------------------------------------------------------------------- error norms
def crop(a, rc, name):
    """A cross-grid field on the points it has: rows 1..iy-1 and columns 1..jx-1; a tropical
    band (i_band) is periodic in j and keeps every column, the cloud-resolving configuration
    (i_crm) is periodic in i as well and keeps every row.  Any other field whole."""
    if name not in CROSS:
        return a
    return a[..., : rc.iy if rc.i_crm else rc.iy - 1, : rc.jx if rc.i_band else rc.jx - 1]


_crop = crop          # relerr and rel_l2 take a `crop` switch of their own


def relerr(a, b, rc, name, crop=True):
    """Relative max-norm of a - b; crop=False compares a cross-grid field whole."""
    if crop:
        a, b = _crop(a, rc, name), _crop(b, rc, name)
    den = max(np.max(np.abs(b)), 1e-300)
    return float(np.max(np.abs(a - b)) / den)


def rel_l2(a, b, rc, name, crop=True):
    """Relative L2 norm of a - b, cropped like relerr."""
    if crop:
        a, b = _crop(a, rc, name), _crop(b, rc, name)
    den = float(np.sqrt(np.sum(b * b)))
    return float(np.sqrt(np.sum((a - b) ** 2))) / max(den, 1e-300)


# ------------------------------------------------------------------------------- the cases
_CASES = {}


def case(name, **overrides):
    """(rc, data, state) of CONFIGS[name] with the overrides, generated once and shared: a test
    that changes the state copies it first.  'C' / 'N' are C1 / N1 cut to the 37 x 29 grid (or to the
    jx, iy, nspgx, nspgd among the overrides).
    The state is the generated one plus the UW TKE (ibltyp = 2) and the patchy hydrometeors
    (nqx = 5) where the configuration has them."""
    key = (name,) + tuple(sorted(overrides.items()))
    if key not in _CASES:
        if name in ("C", "N"):
            cut = dict(jx=37, iy=29, nspgx=None, nspgd=None)
            cut.update(overrides)               # another cut: jx=34, iy=23, nspgx=7, nspgd=7
            rc = dataclasses.replace(CONFIGS["C1" if name == "C" else "N1"], **cut)
        else:
            rc = dataclasses.replace(CONFIGS[name], **overrides)
        gen = icbc.generate_crm if rc.i_crm else icbc.generate_nh if rc.idynamic == 2 else icbc.generate
        data = gen(rc)
        st = dict(data["state"])
        if rc.nqx > 2:
            st.update(icbc.hydrometeor_state(rc, st, nqx=rc.nqx))
        if rc.ibltyp == 2:
            st.update({k: v for k, v in icbc.tke_state(rc).items() if k not in st})
        _CASES[key] = (rc, data, st)
    return _CASES[key]


def with_species(rc, state):
    """ipptls = 2: the state with patchy qi, qr, qs layers (icbc.hydrometeor_state)."""
    if rc.nqx <= 2:
        return state
    st = dict(state)
    st.update(icbc.hydrometeor_state(rc, st, nqx=rc.nqx))
    return st


def state_names(rc, tke=False):
    """The prognostic fields of a configuration; tke: with the UW TKE where ibltyp = 2."""
    names = NH_FIELDS if rc.idynamic == 2 else list(STATE_FIELDS)
    return names + (QX_STATE_FIELDS if rc.nqx > 2 else []) + (TKE_STATE_FIELDS if tke and rc.ibltyp == 2 else [])


# ------------------------------------------------------------------------------- the two cores
def _start(c, data, state, extra, bdyval):
    c.put_state(data["state"] if state is None else state)
    for name, a in (extra or {}).items():
        c.put(name, a)
    if bdyval:
        c.bdyval()
    return c


def engine(rc, data, state=None, nproc=(1, 1), bdyval=True, extra=None):
    """A DynCore on nproc = (tiles in j, tiles in i) holding the state (default: the generated
    one) and the extra fields, after the initial bdyval."""
    from regcm_amd.dycore import DynCore
    return _start(DynCore(rc, data["split"], nproc_j=nproc[0], nproc_i=nproc[1]), data, state, extra, bdyval)


def oracle(rc, data, state=None, bdyval=True, tiles=None, extra=None):
    """The oracle started the same way; tiles: run as set_nproc tiles on that many host threads
    (an int) or as the given (tiles in j, tiles in i)."""
    from oracle.oracle import OracleCore, OracleParallel
    if tiles is None:
        o = OracleCore(rc, data["split"])
    elif isinstance(tiles, tuple):
        o = OracleParallel(rc, data["split"], dims=tiles)
    else:
        o = OracleParallel(rc, data["split"], nthreads=tiles)
    return _start(o, data, state, extra, bdyval)


def pair(rc, data, state=None, nproc=(1, 1), bdyval=True, tiles=None, extra=None):
    """(oracle, engine) started alike."""
    return (oracle(rc, data, state, bdyval, tiles, extra), engine(rc, data, state, nproc, bdyval, extra))


# ------------------------------------------------------------------------------- driving a run
def physics_tendencies(rc, seed=7):
    """Synthetic pc_physic tendencies, coupled with p* (~90 cb) like aten: heating of a few
    K/day, moistening/condensation of ~1e-3 kg/kg/day, momentum drag of a few m/s/day."""
    rng = np.random.Generator(np.random.PCG64(seed))
    scale = {"TPHY": 5e-3, "QVPHY": 1e-6, "QCPHY": 1e-7, "UPHY": 5e-3, "VPHY": 5e-3,
             "PPPHY": 5e-2, "WPHY": 1e-4}
    out = {}
    for name in PHY_FIELDS + (NH_PHY_FIELDS if rc.idynamic == 2 else []):
        nk = field_levels(name, rc.kz, rc.nsplit)
        x = rng.standard_normal((nk, rc.iy, rc.jx))
        # moisture sources are non-negative: a negative forecast would trigger the
        # negative-moisture fix, whose in-tile sweep (:382-393) makes the reference itself
        # decomposition-dependent where such points meet a tile edge
        out[name] = scale[name] * (np.abs(x) if name in ("QVPHY", "QCPHY") else x)
    return out


def advance(e, path, nsteps, phy=None):
    """nsteps by rcmdyn_step ("step"), by tend + bdyval ("pair"), or by the physics seam with
    the phy tendencies put between its halves ("physics")."""
    if path == "step":
        e.step(nsteps)
        return
    for _ in range(nsteps):
        if path == "pair":
            e.tend()
        else:
            e.tend_pre_physics()
            for name, arr in (phy or {}).items():
                e.put(name, arr)
            e.tend_post_physics()
        e.bdyval()


def variant_id(v):
    """The parametrize id of an option variant: "iboudy=4,ipptls=2", "default" for none."""
    return ",".join(f"{k}={x}" for k, x in v.items()) or "default"
