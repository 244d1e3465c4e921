"""SAV restart against the oracle, both cores.

The reference writes atm1/atm2 u, v, t, qx (NH: pp, w; ibltyp = 2: tke), sfs%psa/psb and
dstor/hstor on the owned ranges (Main/mod_savefile.F90:85-172) and a restart reads them back
with dt = dt2 (Main/mod_init.F90:414-465, 864-870), every alarm created anew at the restart
time (Main/mpplib/mod_timer.F90:280-303: `now` = the restart time, so alarm_day acts on the
first step and the NH upper radiative mask is rebuilt there, Main/mod_sound.F90:500).

RCM_initialize then calls bdyval (Main/mod_regcm_interface.F90:150) before the first step:
it refills the boundary lines and the boundary-wind slices that decouple reads
(Main/mod_tendency.F90:895-994).  That call is not idempotent (atm2 takes the boundary values
atm1 already holds), so a reference restart is not bit-identical to the uninterrupted run; the
check is therefore the oracle restarted the same way.  Here a SAV is rcmdyn_get of those fields
plus the clock, taken from the oracle after n steps; the restart puts it over a fresh init,
sets the clock one bdyval back (dt = dt2) and calls bdyval, on the oracle and on a 2x2
decomposed engine alike (oracle/rcm_oracle.c rebuilds the radiative mask under the same alarm
rule).  Tolerances are the step tolerances of tests/test_parity_gpu.py and tests/test_nh_gpu.py
(relative max-norm; the transcendental functions differ by ulps between OCML and libm).
"""
import dataclasses

import pytest

from regcm_amd import icbc
from tests.support import case, engine, oracle, relerr, state_names

pytestmark = pytest.mark.gpu


def sav_fields(rc):
    return state_names(rc, tke=True)


def tke(rc):
    return icbc.tke_state(rc) if rc.ibltyp == 2 else None


def write_sav(core, rc):
    return {n: core.get(n) for n in sav_fields(rc)}, core.get_time()


def restart(core, rc, sav, clock, lcount=None):
    """a fresh run (core: after init, which read the statics, the boundary data and the initial
    state): the SAV fields over the initial state, dt = dt2, then RCM_initialize's bdyval (which
    advances the boundary clock by dtsec)"""
    for name, a in sav.items():
        core.put(name, a)
    lc, _, xb = clock
    core.set_time(lc if lcount is None else lcount, 2.0 * rc.dt, xb - rc.dt)
    core.bdyval()
    return core


@pytest.mark.parametrize("ibltyp", [1, 2])
def test_hydrostatic_restart_matches_oracle_restart(c1_data, ibltyp):
    rc0, data = c1_data
    rc = dataclasses.replace(rc0, ibltyp=ibltyp)
    ro, re = pair_from_sav(rc, data, 4)
    for c in (ro, re):
        c.step(6)
    assert re.get_time() == ro.get_time()
    for name in sav_fields(rc):
        whole = name in ("DSTOR", "HSTOR")      # these two on the full arrays, the rest cropped
        err = relerr(re.get(name), ro.get(name), rc, name, crop=not whole)
        assert err < 1e-10, (name, err)


def pair_from_sav(rc, data, n, lcount=None):
    """the oracle's SAV after n steps; the oracle and a 2x2 engine restarted from it"""
    o = oracle(rc, data, extra=tke(rc))
    o.step(n)
    sav, clock = write_sav(o, rc)
    o.close()
    ro = restart(oracle(rc, data, bdyval=False, extra=tke(rc)), rc, sav, clock, lcount)
    re = restart(engine(rc, data, nproc=(2, 2), bdyval=False, extra=tke(rc)), rc, sav, clock, lcount)
    return ro, re


@pytest.mark.parametrize("ibltyp", [1, 2])
def test_nh_restart_matches_oracle_restart(ibltyp):
    rc0, data, _ = case("N1")
    rc = dataclasses.replace(rc0, ibltyp=ibltyp)
    ro, re = pair_from_sav(rc, data, 3)
    for c in (ro, re):
        c.step(2)                      # the first step rebuilds the radiative mask (alarm_day)
    assert re.get_time() == ro.get_time()
    for name in sav_fields(rc):
        err = relerr(re.get(name), ro.get(name), rc, name)
        assert err < 1e-10, (name, err)


def test_nh_restart_across_the_day_alarm():
    """restart a step before a simulated day boundary: the mask is rebuilt at the restart and
    again when the day alarm acts two steps later, on the engine as on the oracle"""
    rc, data, _ = case("N1")
    day = int(round(86400.0 / rc.dt))
    ro, re = pair_from_sav(rc, data, 3, lcount=day - 1)
    for c in (ro, re):
        c.step(3)
    assert re.get_time() == ro.get_time()
    for name in sav_fields(rc):
        err = relerr(re.get(name), ro.get(name), rc, name)
        assert err < 1e-10, (name, err)
