"""SAV checkpoint / restart.

The reference's SAV file holds atm1/atm2 u, v, t, qx, sfs%psa/psb and dstor/hstor on the owned
index ranges (Main/mod_savefile.F90:85-172, written at :764 every savfrq, read back by
Main/mod_init.F90:414-465 with dt = dt2 at :864-870).  rcmdyn_get of those fields plus
rcmdyn_get_time is the SAV write; a fresh engine fed by rcmdyn_put / rcmdyn_set_time is the
restart.  The continued run is bit-identical to the uninterrupted one, also when the restart
runs on another decomposition (the hydrostatic step is decomposition-invariant, SURVEY.md
8(e)).
"""
import numpy as np
import pytest

from regcm_amd.config import STATE_FIELDS
from tests.support import engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nproc", [(1, 1), (2, 2)])
def test_restart_bit_identical(c1_data, nproc):
    rc, data = c1_data
    ref = engine(rc, data)
    ref.step(7)
    run = engine(rc, data)
    run.step(4)
    sav = {name: run.get(name) for name in STATE_FIELDS}
    clock = run.get_time()
    run.close()
    rst = engine(rc, data, nproc=nproc, bdyval=False)    # statics and boundary data, as init reads them again
    for name, a in sav.items():
        rst.put(name, a)
    rst.set_time(*clock)
    rst.step(3)
    for name in STATE_FIELDS:
        assert np.array_equal(rst.get(name), ref.get(name)), name
    assert rst.get_time() == ref.get_time()
