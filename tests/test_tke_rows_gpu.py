"""The engine against tests/tke_ref.py, the NumPy statement of one step of the UW-PBL TKE in the
hydrostatic core (ibltyp = 2) written from the Fortran text.  No oracle is involved.  Through the
C-ABI with rcmdyn_set_diagnostics on: two steps of tend + bdyval from the state after the initial
bdyval, on tests/test_tke_rows_cpu.py's inputs (a TKE that varies in i, j and k with a patch, a TKEPHY of
both signs that puts the forecast on the tkemin floor, a zonal wind that reverses along the west and
east lines).

Grids: C1 cut to 37 x 29 and to 34 x 23, variants default, upstream_mode 0, idiffu 2, idiffu 3, iboudy 4,
iboudy 3, and the 37 x 29 grid as 2 x 2 tiles (default and idiffu 3, whose column the tile bounds place;
they are read from the host-side decomposition).

Tolerance: none.  QDOT, then ATM1_TKE and ATM2_TKE after tend and after bdyval, bit for bit at every
cross point of the kz + 1 levels, boundary lines included, with the non-vacuity asserts of
tests/test_tke_rows_cpu.py (check_tke).
"""
import functools

import pytest

from regcm_amd.dycore import tile_extent
from tests import support
from tests.support import variant_id
from tests.test_dyn_rows_cpu import GRIDS
from tests.test_tke_rows_cpu import VARIANTS, check_tke, start, two_steps

pytestmark = pytest.mark.gpu

ONE = (1, 1)
CASES = [(g, v, ONE) for g in GRIDS for v in VARIANTS] + [("37x29", v, (2, 2)) for v in ({}, {"idiffu": 3})]


def _cid(p):
    return p if isinstance(p, str) else "x".join(map(str, p)) if isinstance(p, tuple) else variant_id(p)


@functools.lru_cache(maxsize=None)
def _engine_run(grid, vkey, nproc):
    rc, data, st, extra = start(grid, dict(vkey))
    e = support.engine(rc, data, st, nproc, bdyval=False, extra=extra)
    e.set_diagnostics(True)
    e.bdyval()
    return rc, two_steps(e)


@pytest.mark.parametrize("grid,variant,nproc", CASES, ids=_cid)
def test_tke_step_bit_for_bit(grid, variant, nproc):
    rc, steps = _engine_run(grid, tuple(sorted(variant.items())), nproc)
    tiles = [tile_extent(rc.jx, rc.iy, nproc[0], nproc[1], t) for t in range(nproc[0] * nproc[1])]
    for n, step in enumerate(steps):
        check_tke(f"{grid} {_cid(nproc)} {variant_id(variant)} step {n + 1}", rc, step, n == 0, tiles=tiles)
