"""Host API of the MI355X dynamical-core engine (ctypes over include/rcmdyn.h).

``DynCore`` mirrors the calls the reference driver makes on this path
(Main/mod_regcm_interface.F90:172-228): ``tend()`` for ``call tend``, ``bdyval()`` for
``call bdyval``, ``step(n)`` for n iterations of that loop, and ``put``/``get`` for the module
state that ``mod_atm_interface`` holds.  Errors come back as exceptions carrying the engine's
message (the reference calls ``fatal``; e.g. 'CFL VIOLATION', Main/mod_tendency.F90:702).

The engine library is built in-tree (``regcm_amd/librcmdyn.so``); there is no CPU fallback:
if the library or a GPU is missing, construction fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

from .config import CHE_FIELD, CUMTRAN_FIELD, FIELD, OUTPUT_2D, OUTPUT_FIELD, OUTPUT_FIELDS, TRACER_DIAG_TERM, TRACER_FIELD, RcmdynConfig, build_config, field_levels

_HERE = os.path.dirname(os.path.abspath(__file__))
# RCMDYN_LIB selects an instrumented build (tools/phases.py); default: the in-tree engine
LIB_PATH = os.environ.get("RCMDYN_LIB") or os.path.join(_HERE, "librcmdyn.so")
_lib = None

EXPORTED = [
    "rcmdyn_create", "rcmdyn_destroy", "rcmdyn_last_error", "rcmdyn_set_nproc",
    "rcmdyn_tile_extent", "rcmdyn_tile_extent_cfg", "rcmdyn_put", "rcmdyn_get", "rcmdyn_set_time", "rcmdyn_get_time",
    "rcmdyn_tend", "rcmdyn_bdyval", "rcmdyn_step", "rcmdyn_synchronize", "rcmdyn_diagnostics",
    "rcmdyn_comm_unique_id", "rcmdyn_last_step_ms", "rcmdyn_set_diagnostics", "rcmdyn_kernel_times",
    "rcmdyn_tend_pre_physics", "rcmdyn_tend_post_physics", "rcmdyn_bdyin", "rcmdyn_reductions", "rcmdyn_runtime_info",
    "rcmdyn_exchange_plan", "rcmdyn_overlap_shares",
    "rcmdyn_set_budget", "rcmdyn_get_budget", "rcmdyn_reset_budget",
    "rcmdyn_set_massck", "rcmdyn_get_massck",
    "rcmdyn_set_condtq", "rcmdyn_put_rh0adj", "rcmdyn_get_condtq",
    "rcmdyn_set_subex", "rcmdyn_put_subex", "rcmdyn_get_subex", "rcmdyn_physics_subex",
    "rcmdyn_set_tracers", "rcmdyn_put_tracer", "rcmdyn_get_tracer", "rcmdyn_put_tracer_nudge",
    "rcmdyn_set_cumtran", "rcmdyn_put_cumtran", "rcmdyn_get_cumtran",
    "rcmdyn_set_tracer_budget", "rcmdyn_get_tracer_budget", "rcmdyn_reset_tracer_budget",
    "rcmdyn_set_output", "rcmdyn_output_atm", "rcmdyn_get_output",
    "rcmdyn_set_output_che", "rcmdyn_output_che", "rcmdyn_get_output_che",
]

# enum rcmdyn_budget_term, in order: the tendency budget of t and qv (idiag = 1)
BUDGET_TERMS = ["T_ADH", "T_ADV", "T_ADI", "T_BDY", "T_DIF", "Q_ADH", "Q_ADV", "Q_ADI", "Q_BDY", "Q_DIF"]
IQV = 1    # the reference's index of water vapour (Main/mpplib/mod_runparams.F90:38)
# one record of the mass check (rcmdyn_get_massck), in order
MASSCK_COLUMNS = ("lcount", "dt", "drymass", "dryadv", "qmass", "qadv")
# enum rcmdyn_condtq_term, in order: the held rh0adj, the last tend's condensation increments
CONDTQ_TERMS = ["RH0ADJ", "T", "QV", "QC"]
# enum rcmdyn_subex_field, in order: the host's 2-D tables, cucloud's output, the accumulators, and
# what the device forms (REMRAT / REMBC with rem on); SUBEX_2D: the fields of one plane
SUBEX_FIELDS = ["RH0", "QCK1", "CGUL", "CEVAP", "CACCR", "CU_CLDFRA", "CU_CLDLWC", "RAINNC", "LSMRNC",
                "FCC", "CLDFRA", "CLDLWC", "RH0ADJ", "LSC_T", "LSC_QV", "LSC_QC", "TRRATE", "REMRAT", "REMBC"]
SUBEX_2D = ("RH0", "QCK1", "CGUL", "CEVAP", "CACCR", "RAINNC", "LSMRNC", "TRRATE")
# the host box every put and get ends with: j1, j2, i1, i2, k1, k2
BOX = [ctypes.c_int32] * 6


class EngineError(RuntimeError):
    pass


def _number(table, key) -> int:
    """A term or field by name (table: the names in order, or a name -> number dict) or by number."""
    if not isinstance(key, str):
        return int(key)
    return table[key] if isinstance(table, dict) else table.index(key)


def lib():
    """Load the in-tree engine library (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(f"engine library missing: {LIB_PATH} (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    i32 = ctypes.c_int32
    dp = ctypes.POINTER(ctypes.c_double)
    L.rcmdyn_create.argtypes = [ctypes.POINTER(RcmdynConfig), ctypes.POINTER(P)]
    L.rcmdyn_destroy.argtypes = [P]
    L.rcmdyn_last_error.argtypes = [P]
    L.rcmdyn_last_error.restype = ctypes.c_char_p
    L.rcmdyn_set_nproc.argtypes = [i32, i32, i32, ctypes.POINTER(i32)]
    L.rcmdyn_tile_extent.argtypes = [i32, i32, i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.rcmdyn_tile_extent_cfg.argtypes = [ctypes.POINTER(RcmdynConfig), i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.rcmdyn_put.argtypes = [P, i32, dp, *BOX]
    L.rcmdyn_get.argtypes = [P, i32, dp, *BOX]
    L.rcmdyn_set_time.argtypes = [P, ctypes.c_int64, ctypes.c_double, ctypes.c_double]
    L.rcmdyn_get_time.argtypes = [P, ctypes.POINTER(ctypes.c_int64), dp, dp]
    L.rcmdyn_tend.argtypes = [P]
    L.rcmdyn_tend_pre_physics.argtypes = [P]
    L.rcmdyn_tend_post_physics.argtypes = [P]
    L.rcmdyn_bdyin.argtypes = [P]
    L.rcmdyn_bdyval.argtypes = [P]
    L.rcmdyn_step.argtypes = [P, i32]
    L.rcmdyn_synchronize.argtypes = [P]
    L.rcmdyn_diagnostics.argtypes = [P, dp]
    L.rcmdyn_comm_unique_id.argtypes = [ctypes.POINTER(ctypes.c_uint8)]
    L.rcmdyn_last_step_ms.argtypes = [P, dp]
    L.rcmdyn_set_diagnostics.argtypes = [P, i32]
    L.rcmdyn_reductions.argtypes = [P, dp]
    L.rcmdyn_runtime_info.argtypes = [ctypes.c_char_p, i32]
    L.rcmdyn_exchange_plan.argtypes = [ctypes.POINTER(RcmdynConfig), i32, ctypes.POINTER(ctypes.c_int64),
                                       ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    L.rcmdyn_overlap_shares.argtypes = [ctypes.POINTER(RcmdynConfig), ctypes.POINTER(i32), i32]
    L.rcmdyn_kernel_times.argtypes = [P, i32, i32, ctypes.c_char_p, ctypes.POINTER(i32), dp, ctypes.POINTER(i32)]
    L.rcmdyn_set_budget.argtypes = [P, i32, i32, ctypes.c_double]
    L.rcmdyn_get_budget.argtypes = [P, i32, dp, *BOX]
    L.rcmdyn_reset_budget.argtypes = [P]
    L.rcmdyn_set_massck.argtypes = [P, i32, i32]
    L.rcmdyn_get_massck.argtypes = [P, dp, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_int64)]
    L.rcmdyn_set_condtq.argtypes = [P, i32, ctypes.c_double]
    L.rcmdyn_put_rh0adj.argtypes = [P, dp, *BOX]
    L.rcmdyn_get_condtq.argtypes = [P, i32, dp, *BOX]
    L.rcmdyn_set_subex.argtypes = [P, i32, ctypes.c_double, ctypes.c_double, ctypes.c_double, i32, i32, i32, i32, i32, i32]
    L.rcmdyn_put_subex.argtypes = [P, i32, dp, *BOX]
    L.rcmdyn_get_subex.argtypes = [P, i32, dp, *BOX]
    L.rcmdyn_physics_subex.argtypes = [P]
    L.rcmdyn_set_tracers.argtypes = [P, i32, i32]
    L.rcmdyn_put_tracer.argtypes = [P, i32, i32, dp, *BOX]
    L.rcmdyn_get_tracer.argtypes = [P, i32, i32, dp, *BOX]
    L.rcmdyn_put_tracer_nudge.argtypes = [P, dp, dp]
    L.rcmdyn_set_cumtran.argtypes = [P, i32, i32]
    L.rcmdyn_put_cumtran.argtypes = [P, i32, dp, *BOX]
    L.rcmdyn_get_cumtran.argtypes = [P, i32, dp, *BOX]
    L.rcmdyn_set_tracer_budget.argtypes = [P, i32, ctypes.c_double, ctypes.c_double]
    L.rcmdyn_get_tracer_budget.argtypes = [P, i32, i32, dp, *BOX]
    L.rcmdyn_reset_tracer_budget.argtypes = [P]
    L.rcmdyn_set_output.argtypes = [P, i32, i32]
    L.rcmdyn_output_atm.argtypes = [P, ctypes.c_uint32]
    L.rcmdyn_get_output.argtypes = [P, i32, ctypes.c_void_p, *BOX]
    L.rcmdyn_set_output_che.argtypes = [P, i32, i32, i32]
    L.rcmdyn_output_che.argtypes = [P, ctypes.c_uint32, i32, i32]
    L.rcmdyn_get_output_che.argtypes = [P, i32, i32, ctypes.c_void_p, *BOX]
    _lib = L
    return L


def set_nproc(nproc: int, jx: int, iy: int):
    cp = (ctypes.c_int32 * 2)()
    if lib().rcmdyn_set_nproc(nproc, jx, iy, cp):
        raise EngineError("rcmdyn_set_nproc failed")
    return int(cp[0]), int(cp[1])


def tile_extent(jx: int, iy: int, nproc_j: int, nproc_i: int, tile: int, i_band: int = 0, i_crm: int = 0):
    """Index ranges of one tile, ([jde1, jde2, ide1, ide2, jce1, jce2, ice1, ice2],
    [left, right, bottom, top]).  With i_band / i_crm the j / i direction is periodic
    (rcmdyn_tile_extent_cfg): no boundary side there, and the cross range takes every point."""
    ext = (ctypes.c_int32 * 8)()
    bdy = (ctypes.c_int32 * 4)()
    if i_band or i_crm:
        cfg = RcmdynConfig()
        cfg.jx, cfg.iy, cfg.nproc_j, cfg.nproc_i = jx, iy, nproc_j, nproc_i
        cfg.i_band, cfg.i_crm = i_band, i_crm
        if lib().rcmdyn_tile_extent_cfg(ctypes.byref(cfg), tile, ext, bdy):
            raise EngineError("rcmdyn_tile_extent_cfg failed")
    elif lib().rcmdyn_tile_extent(jx, iy, nproc_j, nproc_i, tile, ext, bdy):
        raise EngineError("rcmdyn_tile_extent failed")
    return list(ext), list(bdy)


PLAN_COLUMNS = ("call", "kind", "chan", "dir", "peer", "count", "sig")


def exchange_plan(rc, split, nproc_j: int, nproc_i: int, rank: int, nsteps: int) -> np.ndarray:
    """Host-only communication plan of one rank (rcmdyn_exchange_plan): an (n, 7) int64 array
    with the columns PLAN_COLUMNS, in issue order.  No GPU is touched."""
    cfg = build_config(rc, split, nproc_j, nproc_i, tile_first=rank, tile_count=1, comm_rank=rank,
                       comm_size=nproc_j * nproc_i)
    n = ctypes.c_int64()
    if lib().rcmdyn_exchange_plan(ctypes.byref(cfg), nsteps, None, 0, ctypes.byref(n)):
        raise EngineError(lib().rcmdyn_last_error(None).decode())
    out = np.zeros((n.value, 7), dtype=np.int64)
    if lib().rcmdyn_exchange_plan(ctypes.byref(cfg), nsteps, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  n.value, ctypes.byref(n)):
        raise EngineError(lib().rcmdyn_last_error(None).decode())
    return out


def runtime_info() -> str:
    """Paths (and RCCL version) of the HIP runtime and librccl the engine is bound to."""
    buf = ctypes.create_string_buffer(1024)
    if lib().rcmdyn_runtime_info(buf, 1024):
        raise EngineError(lib().rcmdyn_last_error(None).decode())
    return buf.value.decode()


def comm_unique_id() -> bytes:
    buf = (ctypes.c_uint8 * 128)()
    if lib().rcmdyn_comm_unique_id(buf):
        raise EngineError(lib().rcmdyn_last_error(None).decode())
    return bytes(buf)


def overlap_shares(rc, split, nproc_j: int, nproc_i: int):
    """Host-only (rcmdyn_overlap_shares): per rank of an nproc_j x nproc_i job, the points of
    k_columns / k_momentum / k_scalars that run beside the prologue exchange (part 1) and their
    totals, as [(col_p1, col, mom_p1, mom, sca_p1, sca), ...]."""
    n = nproc_j * nproc_i
    out = []
    for r in range(n):
        cfg = build_config(rc, split, nproc_j, nproc_i, tile_first=r, tile_count=1, comm_rank=r, comm_size=n)
        v = (ctypes.c_int32 * 6)()
        if lib().rcmdyn_overlap_shares(ctypes.byref(cfg), v, 1):
            raise EngineError(lib().rcmdyn_last_error(None).decode())
        out.append(tuple(v))
    return out


class DynCore:
    """The dynamical core of one process: one or more tiles on one GPU."""

    def __init__(self, rc, split, nproc_j: int = 1, nproc_i: int = 1, tile_first: int = 0,
                 tile_count: Optional[int] = None, comm_rank: int = 0, comm_size: int = 1,
                 device: int = -1, unique_id: Optional[bytes] = None):
        self.rc = rc
        self.cfg = build_config(rc, split, nproc_j, nproc_i, tile_first, tile_count,
                                comm_rank, comm_size, device, unique_id)
        self.h = ctypes.c_void_p()
        if lib().rcmdyn_create(ctypes.byref(self.cfg), ctypes.byref(self.h)):
            raise EngineError(lib().rcmdyn_last_error(None).decode())

    def _check(self, rc):
        if rc:
            raise EngineError(lib().rcmdyn_last_error(self.h).decode())

    def close(self):
        """rcmdyn_destroy: a lazy tend still pending is launched first; its failure raises."""
        if self.h:
            rc = lib().rcmdyn_destroy(self.h)
            self.h = ctypes.c_void_p()
            if rc:
                raise EngineError(lib().rcmdyn_last_error(None).decode())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _put_box(self, fn, arr, j1, i1, k1, *lead):
        """fn(h, *lead, src, box) with a (nk, ni, nj) array as the box that starts at the global
        indices (j1, i1, k1)."""
        a = np.ascontiguousarray(arr, dtype=np.float64)
        nk, ni, nj = a.shape
        self._check(fn(self.h, *lead, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                       j1, j1 + nj - 1, i1, i1 + ni - 1, k1, k1 + nk - 1))

    def _get_box(self, fn, nk, *lead, dtype=np.float64) -> np.ndarray:
        """fn(h, *lead, dst, box) over the whole domain and nk levels: a zero-filled (nk, iy, jx) array
        with what the call wrote."""
        out = np.zeros((nk, self.rc.iy, self.rc.jx), dtype=dtype)
        self._check(fn(self.h, *lead, out.ctypes.data_as(fn.argtypes[1 + len(lead)]),
                       1, self.rc.jx, 1, self.rc.iy, 1, nk))
        return out

    def put(self, name: str, arr: np.ndarray, j1: int = 1, i1: int = 1, k1: int = 1):
        self._put_box(lib().rcmdyn_put, arr, j1, i1, k1, FIELD[name])

    def get(self, name: str) -> np.ndarray:
        return self._get_box(lib().rcmdyn_get, field_levels(name, self.rc.kz, self.rc.nsplit), FIELD[name])

    def put_state(self, st: dict):
        for name, arr in st.items():
            self.put(name, arr)

    def set_time(self, lcount: int, dt: float, xbctime: float):
        self._check(lib().rcmdyn_set_time(self.h, lcount, dt, xbctime))

    def get_time(self):
        a, b, c = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        self._check(lib().rcmdyn_get_time(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def tend(self):
        self._check(lib().rcmdyn_tend(self.h))

    def tend_pre_physics(self):
        """surface_pressures .. mkslice .. new_pressure: the ATMS_* fields become readable."""
        self._check(lib().rcmdyn_tend_pre_physics(self.h))

    def tend_post_physics(self):
        """The rest of tend, with the *PHY tendencies put since (physics coupling seam)."""
        self._check(lib().rcmdyn_tend_post_physics(self.h))

    def bdyval(self):
        self._check(lib().rcmdyn_bdyval(self.h))

    def bdyin(self):
        """bdyin from read_icbc on: the record put into the XxB_B1 fields becomes b1."""
        self._check(lib().rcmdyn_bdyin(self.h))

    def step(self, n: int = 1):
        self._check(lib().rcmdyn_step(self.h, n))

    def synchronize(self):
        self._check(lib().rcmdyn_synchronize(self.h))

    def diagnostics(self):
        out = (ctypes.c_double * 4)()
        self._check(lib().rcmdyn_diagnostics(self.h, out))
        return list(out)

    def reductions(self):
        """(ptntot, pt2tot, cflmax) of the last step over the whole job (the 3-hourly report,
        Main/mod_tendency.F90:705-725, Main/mod_sound.F90:634-646); collective over ranks."""
        out = (ctypes.c_double * 3)()
        self._check(lib().rcmdyn_reductions(self.h, out))
        return tuple(out)

    def last_step_ms(self) -> float:
        v = ctypes.c_double()
        self._check(lib().rcmdyn_last_step_ms(self.h, ctypes.byref(v)))
        return v.value

    def set_diagnostics(self, on: bool = True):
        self._check(lib().rcmdyn_set_diagnostics(self.h, 1 if on else 0))

    def set_budget(self, on: bool = True, idgq: int = IQV, rw: float = 1.0):
        """The tendency budget of t and qv (idiag = 1): every later tend adds each term times rw
        (the host's alarm_out_atm%rw) to its accumulator; only idgq = iqv is computed."""
        self._check(lib().rcmdyn_set_budget(self.h, 1 if on else 0, idgq, rw))

    def get_budget(self, term) -> np.ndarray:
        """One accumulator, by name (BUDGET_TERMS) or number, as a (kz, iy, jx) array: zero
        outside the interior cross points."""
        return self._get_box(lib().rcmdyn_get_budget, self.rc.kz, _number(BUDGET_TERMS, term))

    def reset_budget(self):
        """Zeroes the ten accumulators (the host does it after writing them to the ATM file)."""
        self._check(lib().rcmdyn_reset_budget(self.h))

    def set_massck(self, on: bool = True, cap: int = 1024):
        """The mass check of tend (Main/mod_massck.F90): every later tend appends one record
        (MASSCK_COLUMNS) to a device ring of cap records; the same on and cap keep the log."""
        self._check(lib().rcmdyn_set_massck(self.h, 1 if on else 0, cap))
        if on:
            self._massck_cap = cap

    def get_massck(self):
        """(records [count, 6], lost): the records of the tends since the last call, oldest
        first, and how many older ones the ring overwrote.  Empties the log; collective over
        the ranks of a job (it adds the four sums over them)."""
        cap = getattr(self, "_massck_cap", 1)
        out = np.zeros((cap, len(MASSCK_COLUMNS)))
        n, lost = ctypes.c_int32(), ctypes.c_int64()
        self._check(lib().rcmdyn_get_massck(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cap,
                                            ctypes.byref(n), ctypes.byref(lost)))
        return out[:n.value].copy(), int(lost.value)

    def set_condtq(self, on: bool = True, conf: float = 1.0):
        """The SUBEX condensation (condtq, ipptls = 1) inside tend; conf is subexparam's
        condensation efficiency, in (0, 1].  Every later tend needs an rh0adj (put_rh0adj)."""
        self._check(lib().rcmdyn_set_condtq(self.h, 1 if on else 0, conf))

    def put_rh0adj(self, arr: np.ndarray, j1: int = 1, i1: int = 1, k1: int = 1):
        """cldfrac's adjusted humidity threshold, a (kz, ni, nj) array of values in [0, 0.99999]
        starting at the global indices (j1, i1, k1).  tend waits for one put since the switch-on
        that covers the interior cross points of the tiles and their rings on every level."""
        self._put_box(lib().rcmdyn_put_rh0adj, arr, j1, i1, k1)

    def get_condtq(self, term) -> np.ndarray:
        """One term by name (CONDTQ_TERMS) or number as a (kz, iy, jx) array: the held rh0adj, or
        the last tend's coupled condensation increment of t, qv or qc (zero outside the interior
        cross points)."""
        return self._get_box(lib().rcmdyn_get_condtq, self.rc.kz, _number(CONDTQ_TERMS, term))

    def set_subex(self, on: bool = True, rhmax: float = 1.01, rhmin: float = 0.01, tc0: float = 238.0,
                  larcticcorr: bool = False, iconvlwp: int = 1, rem: bool = False, icldfrac: int = 0,
                  icldmstrat: int = 0, lsecind: bool = False):
        """SUBEX on the device (ipptls = 1): cldfrac with subex_cldfrac and the rain columns of subex
        run where the reference calls physical_parametrizations, in a whole tend / step or from
        physics_subex on the split path.  rhmax, rhmin, tc0, larcticcorr, iconvlwp: the run's
        settings; rem: also REMRAT / REMBC.  icldfrac, icldmstrat, lsecind name options that are
        not built: anything but 0 is refused.  The five 2-D tables must be put before a run."""
        self._check(lib().rcmdyn_set_subex(self.h, 1 if on else 0, rhmax, rhmin, tc0, int(larcticcorr), int(iconvlwp),
                                           int(rem), int(icldfrac), int(icldmstrat), int(lsecind)))

    def put_subex(self, name, arr: np.ndarray, j1: int = 1, i1: int = 1, k1: int = 1):
        """One field (SUBEX_FIELDS name or number) the host owns: the tables RH0, QCK1, CGUL, CEVAP,
        CACCR and the accumulators RAINNC, LSMRNC as (ni, nj) or (1, ni, nj) arrays, cucloud's
        CU_CLDFRA (in [0, 1]) and CU_CLDLWC as (kz, ni, nj) arrays, starting at (j1, i1, k1)."""
        a = np.asarray(arr)
        self._put_box(lib().rcmdyn_put_subex, a[None] if a.ndim == 2 else a, j1, i1, k1, _number(SUBEX_FIELDS, name))

    def get_subex(self, name) -> np.ndarray:
        """One field (SUBEX_FIELDS name or number) as a (1, iy, jx) array (SUBEX_2D) or a (kz, iy,
        jx) array: zero outside the interior cross points."""
        f = _number(SUBEX_FIELDS, name)
        nk = 1 if 0 <= f < len(SUBEX_FIELDS) and SUBEX_FIELDS[f] in SUBEX_2D else self.rc.kz
        return self._get_box(lib().rcmdyn_get_subex, nk, f)

    def physics_subex(self):
        """The subex kernels of the split path, between tend_pre_physics and tend_post_physics
        (which runs them first if this was not called); once per tend."""
        self._check(lib().rcmdyn_physics_subex(self.h))

    def set_tracers(self, ntr: int, ichebdy: int = 1):
        """Declares ntr chemical tracers (the reference's ichem = 1 chain of tend and bdyval);
        ntr = 0 switches the family off and frees its buffers.  Only ichebdy = 1 is built."""
        self._check(lib().rcmdyn_set_tracers(self.h, ntr, ichebdy))

    def put_tracer(self, name, itr: int, arr: np.ndarray, j1: int = 1, i1: int = 1, k1: int = 1):
        """One field (TRACER_FIELDS name or number) of tracer itr = 1..ntr, a (kz, ni, nj) array
        coupled with p*, starting at the global indices (j1, i1, k1)."""
        self._put_box(lib().rcmdyn_put_tracer, arr, j1, i1, k1, _number(TRACER_FIELD, name), itr)

    def get_tracer(self, name, itr: int) -> np.ndarray:
        """One field of tracer itr as a (kz, iy, jx) array."""
        return self._get_box(lib().rcmdyn_get_tracer, self.rc.kz, _number(TRACER_FIELD, name), itr)

    def put_tracer_nudge(self, cefc: np.ndarray, cegc: np.ndarray):
        """nudge_chiten's tables as (kz, nspgx) arrays, [k - 1, ib - 1] = cefc(ib, k); zero until put."""
        a = np.ascontiguousarray(cefc, dtype=np.float64)
        b = np.ascontiguousarray(cegc, dtype=np.float64)
        if a.shape != (self.rc.kz, self.rc.nspgx) or b.shape != a.shape:
            raise EngineError(f"put_tracer_nudge: the tables must have shape (kz, nspgx) = {(self.rc.kz, self.rc.nspgx)}")
        self._check(lib().rcmdyn_put_tracer_nudge(self.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  b.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    def set_cumtran(self, on: bool = True, ncum: int = 1):
        """The tracers' cumulus mixing (cumtran, ichcumtra = 1) inside tend: it acts in a tend whose
        clock has lcount > 0 and lcount % ncum == 0 (ncum = dtcum / dtsec).  The three inputs start
        at zero (kcumtop = 0 mixes nothing) until put_cumtran."""
        self._check(lib().rcmdyn_set_cumtran(self.h, 1 if on else 0, ncum))

    def put_cumtran(self, name, arr: np.ndarray, j1: int = 1, i1: int = 1, k1: int = 1):
        """One input (CUMTRAN_FIELDS name or number): DOTRAN (0 / 1) and KTOP (integers in 0 .. kz)
        as (ni, nj) or (1, ni, nj) arrays, CLDFRA (in [0, 1]) as a (kz, ni, nj) array, starting at
        the global indices (j1, i1, k1)."""
        a = np.asarray(arr)
        self._put_box(lib().rcmdyn_put_cumtran, a[None] if a.ndim == 2 else a, j1, i1, k1, _number(CUMTRAN_FIELD, name))

    def get_cumtran(self, name) -> np.ndarray:
        """One held input as a (1, iy, jx) array (DOTRAN, KTOP) or a (kz, iy, jx) array (CLDFRA)."""
        f = _number(CUMTRAN_FIELD, name)
        return self._get_box(lib().rcmdyn_get_cumtran, self.rc.kz if f == CUMTRAN_FIELD["CLDFRA"] else 1, f)

    def set_tracer_budget(self, on: bool = True, rw: float = 1.0, cfdout: float = 1.0):
        """The tracer budget (ichdiag > 0): every later tend adds each stage term times rw (the
        host's alarm_out_atm%rw) to its accumulator, and an acting cumtran its pseudo-tendency
        times cfdout (alarm_out_che%rw)."""
        self._check(lib().rcmdyn_set_tracer_budget(self.h, 1 if on else 0, rw, cfdout))

    def get_tracer_budget(self, term, itr: int) -> np.ndarray:
        """One accumulator (TRACER_DIAG_TERMS name or number) of tracer itr as a (kz, iy, jx) array:
        zero outside the interior cross points."""
        return self._get_box(lib().rcmdyn_get_tracer_budget, self.rc.kz, _number(TRACER_DIAG_TERM, term), itr)

    def reset_tracer_budget(self):
        """Zeroes every accumulator (the host does it after writing them at alarm_out_che)."""
        self._check(lib().rcmdyn_reset_tracer_budget(self.h))

    def set_output(self, on: bool = True, prec: int = 8):
        """The output stream (mod_output's dyn-owned ATM / SRF / SHF fields, formed on the device):
        prec = 8 hands doubles to the host, prec = 4 the stream files' 4-byte reals."""
        self._check(lib().rcmdyn_set_output(self.h, 1 if on else 0, prec))
        if on:
            self._out_prec = prec

    def output_atm(self, fields):
        """Snapshot of the named fields (OUTPUT_FIELDS names or numbers; or a ready bit mask as an
        int) from the state as it stands: forms them on the device and starts their copy to the
        host; returns without waiting.  Steps issued afterwards do not change what get_output
        returns.  Collective over the ranks of a job."""
        if isinstance(fields, int):
            mask = fields
        else:
            mask = 0
            for f in fields:
                mask |= 1 << _number(OUTPUT_FIELD, f)
        self._check(lib().rcmdyn_output_atm(self.h, mask))

    def get_output(self, name) -> np.ndarray:
        """One field of the last output_atm as a (kz, iy, jx) array, (1, iy, jx) for the 2-D fields,
        float32 or float64 by set_output's prec: zero outside the interior cross points.  Waits for
        that snapshot's copy only."""
        f = _number(OUTPUT_FIELD, name)
        nk = 1 if 0 <= f < len(OUTPUT_FIELDS) and OUTPUT_FIELDS[f] in OUTPUT_2D else self.rc.kz
        return self._get_box(lib().rcmdyn_get_output, nk, f,
                             dtype=np.float32 if getattr(self, "_out_prec", 8) == 4 else np.float64)

    def set_output_che(self, on: bool = True, prec: int = 8, nbatch: int = 1):
        """The tracers' output stream (the CHE file's dyn-owned fields, formed on the device): prec as
        in set_output; nbatch (1 .. ntr) is the largest number of tracers one output_che takes and
        sizes the two buffer sets."""
        self._check(lib().rcmdyn_set_output_che(self.h, 1 if on else 0, prec, nbatch))
        if on:
            self._che_prec = prec

    def output_che(self, fields, itr1: int, itr2: int):
        """Snapshot of the named fields (CHE_FIELDS names or numbers; or a ready bit mask as an int)
        of the tracers itr1 .. itr2 from the state as it stands: forms them on the device and starts
        their copy to the host; returns without waiting.  With the tracer budget on it zeroes all
        five sums of these tracers, whatever the fields.  The engine holds the snapshots of the last
        two calls."""
        if isinstance(fields, int):
            mask = fields
        else:
            mask = 0
            for f in fields:
                mask |= 1 << _number(CHE_FIELD, f)
        self._check(lib().rcmdyn_output_che(self.h, mask, itr1, itr2))

    def get_output_che(self, name, itr: int) -> np.ndarray:
        """One field of tracer itr from the newer held snapshot that has it, as a (kz, iy, jx) array,
        (1, iy, jx) for BURDEN, float32 or float64 by set_output_che's prec: zero outside the
        interior cross points.  Waits for that snapshot's copy only."""
        f = _number(CHE_FIELD, name)
        return self._get_box(lib().rcmdyn_get_output_che, 1 if f == CHE_FIELD["BURDEN"] else self.rc.kz, f, itr,
                             dtype=np.float32 if getattr(self, "_che_prec", 8) == 4 else np.float64)

    def kernel_times(self, nsteps: int, cap: int = 64) -> dict:
        """{kernel name: (launches, average ms per launch)} over nsteps eager steps."""
        names = ctypes.create_string_buffer(cap * 48)
        launches = (ctypes.c_int32 * cap)()
        avg = (ctypes.c_double * cap)()
        n = ctypes.c_int32()
        self._check(lib().rcmdyn_kernel_times(self.h, nsteps, cap, names, launches, avg, ctypes.byref(n)))
        raw = names.raw
        out = {}
        for q in range(n.value):
            nm = raw[q * 48:(q + 1) * 48].split(b"\0", 1)[0].decode()
            out[nm] = (int(launches[q]), float(avg[q]))
        return out
