"""GPU tests of SUBEX on the device (rcmdyn_set_subex; subex.hpp, subex.hip): cldfrac with
subex_cldfrac and the rain columns of subex beside condtq.

The oracle stubs the microphysics, so the yardstick is tests/subex_ref.py, a NumPy transcription of
the Fortran text (tests/test_subex_cpu.py holds the host-compiled header to it bit for bit).  It is
run on the engine's own mkslice export and p*b, with the 10**x of qcth and the chis table from the
host-compiled header, so every comparison here asks for equal bits.  Grids: the 37 x 29 cuts of C1
and N1 and the odd 34 x 23 grid, on inputs whose branch populations tests/test_subex_cpu.py counts.

On tiles: the first tend on 2 x 2 or 1 x 3 tiles gives every subex field, condtq's increments and
the tendencies of one tile bit for bit.  Tiles and one tile part after that step with or without
subex: as tests/test_condtq_gpu.py notes, the reference's own negative-moisture sweep is
tile-dependent where an evaporated cloud meets a tile edge.  Later steps are therefore held to the
tiled host route (the same tiles with subex off, the host putting rh0adj and the increments, which
fills the rings from global arrays): state and tendencies stay equal through a second tend, which
reads the forecasts the first one computed on the rings from the exchanged rh0adj and LSC_*."""
import dataclasses

import numpy as np
import pytest

from regcm_amd import icbc
from regcm_amd.config import CONFIGS
from regcm_amd.dycore import SUBEX_FIELDS, EngineError
from tests import condtq_ref as cq
from tests import subex_host as sh
from tests import subex_ref as sx
from tests.support import case, engine, physics_tendencies, state_names

pytestmark = pytest.mark.gpu       # the host-compiled header needs g++: without it the tests fail, they do not skip

TENS = ["TTEN", "QVTEN", "QCTEN"]
LSC = ["LSC_T", "LSC_QV", "LSC_QC"]
FIELDS3 = ["FCC", "CLDFRA", "CLDLWC", "RH0ADJ"] + LSC          # get-only, kz levels
KEY = {"FCC": "fcc", "CLDFRA": "cldfra", "CLDLWC": "cldlwc", "RH0ADJ": "rh0adj", "LSC_T": "lsc_t", "LSC_QV": "lsc_qv",
       "LSC_QC": "lsc_qc", "RAINNC": "rainnc", "LSMRNC": "lsmrnc", "TRRATE": "trrate", "REMRAT": "remrat", "REMBC": "rembc"}


def setup(name, **over):
    """(rc, data, the rainy state) of a 37 x 29 cut, or of the odd 34 x 23 grid."""
    if name == "odd":
        rc = dataclasses.replace(CONFIGS["C1"], jx=34, iy=23, nspgx=None, nspgd=None)
        data = icbc.generate(rc)
        return rc, data, sx.rainy_state(rc, data["state"])
    if name == "N":
        over.setdefault("ifrayd", 0)
    rc, data, st0 = case(name, **over)
    return rc, data, sx.rainy_state(rc, st0)


def par_of(rc, **kw):
    """The run's scalars; the arctic correction is on in every test (rainy_state has its points)."""
    kw.setdefault("larcticcorr", True)
    return sx.params(rhmax=rc.rhmax, rhmin=rc.rhmin, **kw)


def switch_on(e, rc, par, rem=False, tables=True):
    e.set_subex(True, par.rhmax, par.rhmin, par.tc0, par.larcticcorr, par.iconvlwp, rem)
    if tables:
        for n, a in sx.tables(rc).items():
            e.put_subex(n, a)
    return e


def on_engine(rc, data, st, par, nproc=(1, 1), diag=False, condtq=False, rem=False):
    e = engine(rc, data, st, nproc=nproc)
    if diag:
        e.set_diagnostics(True)
    if condtq:
        e.set_condtq(True, 1.0)
    return switch_on(e, rc, par, rem=rem)


def same(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    eq = a.view(np.int64) == b.view(np.int64)
    assert eq.all(), (what, int((~eq).sum()), a[~eq][:3], b[~eq][:3])


def same_state(a, b, names):
    assert a.get_time() == b.get_time()
    for n in names:
        same(a.get(n), b.get(n), n)


def reference(e, rc, par, dt, cu=None, acc=None, rem=False):
    """The transcription on the engine's own export of this tend (after tend_pre_physics)."""
    f = sx.slice_inputs(e.get, e.get("PSB")[0])
    return sx.run(f, sx.tables(rc), par, dt, rc.dt, sh.chis(), pow10=sh.pow10, cu=cu, acc=acc, rem=rem)


def against_reference(e, rc, c, s, names):
    I = cq.interior(rc)
    for n in names:
        ref = c[KEY[n]] if KEY[n] in c else s[KEY[n]]
        got = e.get_subex(n)
        if got.shape[0] == 1:
            same(got[0][I[1:]], ref[I[1:]], n)
        else:
            same(got[I], ref[I], n)
        outside = np.ones(got.shape, bool)
        outside[(slice(None),) + I[1:]] = False
        assert not got[outside].any(), n                       # a get writes the interior cross points only


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("name", ["C", "N"])
def test_off_is_the_engine_without_subex(name):
    rc, data, st = setup(name)
    names = state_names(rc)
    a, b = engine(rc, data, st), engine(rc, data, st)
    switch_on(b, rc, par_of(rc))                  # on, fed and off again: nothing is left of it
    b.put_subex("CU_CLDFRA", sx.cucloud(rc)[0])
    b.set_subex(False)
    for e in (a, b):
        e.set_diagnostics(True)
        e.step(3)
        e.tend()
    for n in TENS:
        same(a.get(n), b.get(n), n)
    for e in (a, b):
        e.bdyval()
    same_state(a, b, names)
    ka, kb = a.kernel_times(2), b.kernel_times(2)
    assert {k: v[0] for k, v in ka.items()} == {k: v[0] for k, v in kb.items()}
    assert not any("subex" in k for k in kb)
    with pytest.raises(EngineError, match="subex is off"):
        b.get_subex("FCC")
    with pytest.raises(EngineError, match="subex is off"):
        b.physics_subex()


# ------------------------------------------------------------------ 2. one split tend, both cores
@pytest.mark.parametrize("name,hostphy,iconvlwp", [("C", True, 1), ("C", False, 0), ("N", True, 0), ("odd", True, 1)])
def test_one_split_tend_against_the_transcription(name, hostphy, iconvlwp):
    rc, data, st = setup(name)
    par = par_of(rc, iconvlwp=iconvlwp)
    a = on_engine(rc, data, st, par, diag=True)
    dt = a.get_time()[1]
    a.tend_pre_physics()
    a.physics_subex()
    c, s = reference(a, rc, par, dt)
    against_reference(a, rc, c, s, FIELDS3 + ["RAINNC", "LSMRNC", "TRRATE"])
    I = cq.interior(rc)
    assert s["surface"][I[1:]].sum() > 0 and s["lost_all"][I[1:]].sum() > 0 and (s["lsc_t"][I] != 0).sum() > 0
    # on the engine's own export: the arctic factor at work at both clamps and between, the pptmax
    # clamp before and after accretion, the dlowval gate of the evaporation
    cloudy = c["fcc"] > 0
    m = s["masks"]
    count = {"arctic 0.15 clamp": (c["arctic_lo"] & cloudy)[I].sum(), "arctic 1.0 clamp": (c["arctic_hi"] & cloudy)[I].sum(),
             "arctic between": (c["arctic"] & ~c["arctic_lo"] & ~c["arctic_hi"] & cloudy)[I].sum(),
             "pptmax before accretion": m["pptmax_auto"][I].sum(), "pptmax after accretion": m["pptmax_acc"][I].sum(),
             "rdevap <= dlowval": m["evap_gate"][I].sum(), "in-cloud water": (c["cloudy"] & (c["cldlwc"] > 0))[I].sum()}
    print(name, {k: int(v) for k, v in count.items()})
    assert all(v > 0 for v in count.values()), count
    lsc = {n: a.get_subex(n) for n in LSC}
    a.physics_subex()                              # once per tend: the second call does nothing
    same(a.get_subex("RAINNC")[0][I[1:]], s["rainnc"][I[1:]], "RAINNC after a second call")
    phy = physics_tendencies(rc) if hostphy else {}
    for n in ("TPHY", "QVPHY", "QCPHY"):
        if hostphy:
            a.put(n, phy[n])
    a.tend_post_physics()
    # the same tend on an engine without subex whose host formed the sums
    b = engine(rc, data, st)
    b.set_diagnostics(True)
    b.tend_pre_physics()
    for n, l in zip(("TPHY", "QVPHY", "QCPHY"), LSC):
        b.put(n, (phy[n] + lsc[l]) if hostphy else lsc[l])
    b.tend_post_physics()
    for n in TENS:
        same(a.get(n), b.get(n), n)
    for e in (a, b):
        e.bdyval()
    same_state(a, b, state_names(rc))


# ------------------------------------------------------------------ 3. whole mode equals split mode
@pytest.mark.parametrize("name,condtq", [("C", False), ("C", True), ("N", True)])
def test_whole_mode_equals_split_mode(name, condtq):
    rc, data, st = setup(name)
    par = par_of(rc)
    w = on_engine(rc, data, st, par, condtq=condtq)
    p = on_engine(rc, data, st, par, condtq=condtq)
    w.step(3)
    for q in range(3):
        p.tend_pre_physics()
        if q != 1:                                 # the second tend leaves it to tend_post_physics
            p.physics_subex()
        p.tend_post_physics()
        p.bdyval()
    same_state(w, p, state_names(rc))
    for n in FIELDS3 + ["RAINNC", "LSMRNC", "TRRATE"]:
        same(w.get_subex(n), p.get_subex(n), n)
    assert w.get_subex("RAINNC").max() > 0
    if condtq:                                     # no put_rh0adj was made: condtq read the device's field
        for e in (w, p):
            same(e.get_condtq("RH0ADJ"), e.get_subex("RH0ADJ"), "RH0ADJ")
        for n in ("T", "QV", "QC"):
            same(w.get_condtq(n), p.get_condtq(n), n)
        assert (w.get_condtq("QC") != 0).sum() > 0
    # the drop-in pair (a lazy tend, then bdyval) runs the same whole tend
    d = on_engine(rc, data, st, par, condtq=condtq)
    for _ in range(3):
        d.tend()
        d.bdyval()
    same_state(w, d, state_names(rc))
    same(w.get_subex("RAINNC"), d.get_subex("RAINNC"), "RAINNC of the drop-in pair")


# ------------------------------------------------------------------ 4. accumulators
def test_accumulators():
    rc, data, st = setup("C")
    par = par_of(rc)
    e = on_engine(rc, data, st, par)
    I2 = cq.interior(rc)[1:]
    rng = np.random.Generator(np.random.PCG64(2))
    start = {n: rng.uniform(0.0, 2.0, (rc.iy, rc.jx)) for n in ("RAINNC", "LSMRNC")}
    for n, a in start.items():
        e.put_subex(n, a)
        same(e.get_subex(n)[0][I2], a[I2], n)
    for n in start:                                # a put of zeros resets them
        e.put_subex(n, np.zeros((rc.iy, rc.jx)))
        assert not e.get_subex(n).any()
    acc = {n: np.zeros((rc.iy, rc.jx)) for n in ("RAINNC", "LSMRNC", "TRRATE")}
    hits = np.zeros((rc.iy, rc.jx), int)
    for _ in range(3):
        dt = e.get_time()[1]
        e.tend_pre_physics()
        c, s = reference(e, rc, par, dt, acc=acc)
        hits += s["surface"]
        same(s["rainnc"][s["surface"]], (acc["RAINNC"] + s["prainx"])[s["surface"]], "rainnc + prainx")
        acc = {"RAINNC": s["rainnc"], "LSMRNC": s["lsmrnc"], "TRRATE": s["trrate"]}
        e.tend_post_physics()
        e.bdyval()
        against_reference(e, rc, c, s, ["RAINNC", "LSMRNC", "TRRATE"])
    assert (hits[I2] == 3).sum() > 0 and (hits[I2] == 0).sum() > 0


# ------------------------------------------------------------------ 5. convective input
@pytest.mark.parametrize("iconvlwp", [1, 0])
def test_convective_cloud_merges_as_in_the_transcription(iconvlwp):
    rc, data, st = setup("C")
    par = par_of(rc, iconvlwp=iconvlwp)
    e = on_engine(rc, data, st, par)
    cu = sx.cucloud(rc)
    e.put_subex("CU_CLDFRA", cu[0])
    e.put_subex("CU_CLDLWC", cu[1])
    dt = e.get_time()[1]
    e.tend_pre_physics()
    e.physics_subex()
    c, s = reference(e, rc, par, dt, cu=cu)
    I = cq.interior(rc)
    assert c["conv"][I].sum() > 0 and (~c["conv"] & (cu[0] > 0))[I].sum() > 0 and (c["conv"] & c["cloudy"])[I].sum() > 0
    against_reference(e, rc, c, s, FIELDS3)
    e.tend_post_physics()


# ------------------------------------------------------------------ 6. decomposition
def one_tend(e):
    e.tend()
    out = {n: e.get_subex(n) for n in FIELDS3 + ["RAINNC", "LSMRNC", "TRRATE"]}
    out.update({"condtq " + n: e.get_condtq(n) for n in ("RH0ADJ", "T", "QV", "QC")})
    out.update({n: e.get(n) for n in TENS})
    return out


def differing(a, b):
    """{key: (points that differ, their i range, their j range)} of two dicts of arrays."""
    out = {}
    for k in a:
        ne = np.argwhere(np.asarray(a[k]).view(np.int64) != np.asarray(b[k]).view(np.int64))
        if len(ne):
            out[k] = (len(ne), (int(ne[:, -2].min()), int(ne[:, -2].max())), (int(ne[:, -1].min()), int(ne[:, -1].max())))
    return out


@pytest.mark.parametrize("nproc,nograph", [((2, 2), False), ((1, 3), False), ((2, 2), True)], ids=["2x2", "1x3", "2x2-no-graph"])
def test_tiles_equal_one_tile(nproc, nograph, monkeypatch):
    """One tend on tiles gives every subex field, condtq's increments and the tendencies of one tile
    bit for bit.  The ring: the tiles' tendency kernels and condtq compute the forecasts of the
    ring from the rh0adj and the increments that travelled there, and the next tend reads those
    forecasts.  An engine on the same tiles with subex off, whose host puts the one-tile rh0adj
    and increments (a put fills the rings from the global arrays), must therefore stay equal to the
    tiled subex engine through a second tend, state and tendencies.  (Tiles against one tile part
    after the first step with or without subex, at the reference's own tile-dependent
    negative-moisture sweep: tests/test_condtq_gpu.py.)"""
    rc, data, st = setup("C")
    par = par_of(rc)
    names = state_names(rc)
    a = on_engine(rc, data, st, par, diag=True, condtq=True)
    one = one_tend(a)
    if nograph:
        monkeypatch.setenv("RCMDYN_NO_GRAPH", "1")
    d = on_engine(rc, data, st, par, nproc=nproc, diag=True, condtq=True)
    dec = one_tend(d)
    diff = differing(one, dec)
    print("tiles against one tile, first tend:", diff)
    assert not diff, diff
    assert (one["condtq QC"] != 0).sum() > 0 and one["RAINNC"].max() > 0 and (one["LSC_T"] != 0).sum() > 0
    h = engine(rc, data, st, nproc=nproc)
    h.set_diagnostics(True)
    h.set_condtq(True, 1.0)

    def host_tend(src):
        h.put_rh0adj(src["RH0ADJ"])
        for n, l in zip(("TPHY", "QVPHY", "QCPHY"), LSC):
            h.put(n, src[l])
        h.tend()

    host_tend(one)
    for e in (d, h):
        e.bdyval()
    same_state(d, h, names)
    dec2 = one_tend(d)
    host_tend(dec2)
    got = {n: h.get(n) for n in TENS}
    got.update({"condtq " + n: h.get_condtq(n) for n in ("T", "QV", "QC")})
    diff = differing(got, dec2)
    print("tiled subex engine against the tiled host route, second tend:", diff)
    assert not diff, diff
    for e in (d, h):
        e.bdyval()
    same_state(d, h, names)


# ------------------------------------------------------------------ 7. the band
def test_band_against_the_transcription():
    rc, data, st = setup("C", i_band=1)
    par = par_of(rc)
    e = on_engine(rc, data, st, par, condtq=True)
    dt = e.get_time()[1]
    e.tend_pre_physics()
    e.physics_subex()
    c, s = reference(e, rc, par, dt)
    assert cq.interior(rc)[2] == slice(0, rc.jx)
    against_reference(e, rc, c, s, FIELDS3 + ["RAINNC", "LSMRNC", "TRRATE"])
    seam = [0, 1, rc.jx - 2, rc.jx - 1]
    assert (c["fcc"][:, 2:-2, seam] > 0).sum() > 0
    e.tend_post_physics()
    e.bdyval()
    # a whole tend on a second engine gives the same state: the wrapped ring of rh0adj
    w = on_engine(rc, data, st, par, condtq=True)
    w.step(1)
    same_state(w, e, state_names(rc))


# ------------------------------------------------------------------ 8. rem on, with tracers declared
def test_rem_fields_against_the_transcription():
    rc, data, st = setup("C")
    par = par_of(rc)
    e = engine(rc, data, st)
    switch_on(e, rc, par, rem=True)                # before the tracers: the order is free
    e.set_tracers(2)
    dt = e.get_time()[1]
    e.tend_pre_physics()
    e.physics_subex()
    c, s = reference(e, rc, par, dt, rem=True)
    I = cq.interior(rc)
    assert (s["remrat"][I] > 0).sum() > 0 and (s["rembc"][I] > 0).sum() > 0
    against_reference(e, rc, c, s, FIELDS3 + ["REMRAT", "REMBC"])
    e.tend_post_physics()
    e.bdyval()
    e.step(2)                                      # the whole tend holds the tracers' slice as well
    assert np.isfinite(e.get_subex("REMBC")).all()


# ------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_engine_usable():
    rc, data, st = setup("C")
    par = par_of(rc)
    e = engine(rc, data, st)
    args = (par.rhmax, par.rhmin, par.tc0, False, 1, False)
    for kw, word in (({"icldfrac": 3}, "icldfrac"), ({"icldmstrat": 1}, "icldmstrat"), ({"lsecind": True}, "lsecind")):
        with pytest.raises(EngineError, match=word):
            e.set_subex(True, *args, **kw)
    for bad, word in (((0.5, 0.9, 238.0, False, 1, False), "rhmin"), ((1.01, 0.01, float("nan"), False, 1, False), "tc0"),
                      ((1.01, 0.01, 238.0, False, 2, False), "iconvlwp")):
        with pytest.raises(EngineError, match=word):
            e.set_subex(True, *bad)
    with pytest.raises(EngineError, match="subex is off"):          # the refused calls left it off
        e.put_subex("RH0", sx.tables(rc)["RH0"])
    rc2, data2, _ = case("C", ipptls=2)
    e2 = engine(rc2, data2)
    with pytest.raises(EngineError, match="ipptls = 2"):
        e2.set_subex(True, *args)
    e2.step(1)
    # a run before the five tables were put names the first one missing
    switch_on(e, rc, par, tables=False)
    tab = sx.tables(rc)
    for n in ("RH0", "QCK1", "CGUL", "CEVAP", "CACCR"):
        for call in (e.tend, lambda: e.step(1), e.physics_subex):
            with pytest.raises(EngineError, match=f"no {n} was put"):
                call()
        e.put_subex(n, tab[n][2:5, 2:5], j1=3, i1=3)               # a small box is no covering put
        with pytest.raises(EngineError, match=f"no {n} was put"):
            e.tend()
        e.put_subex(n, tab[n])
    with pytest.raises(EngineError, match="no rcmdyn_tend_pre_physics"):
        e.physics_subex()
    e.set_condtq(True, 1.0)
    with pytest.raises(EngineError, match="subex is on"):
        e.put_rh0adj(cq.rh0adj_field(rc))
    cu = sx.cucloud(rc)[0]
    for bad in (-1.0e-9, 1.0000001, float("nan")):
        x = cu.copy()
        x[3, 7, 9] = bad
        with pytest.raises(EngineError, match=r"CU_CLDFRA must"):
            e.put_subex("CU_CLDFRA", x)
    with pytest.raises(EngineError, match="must be finite"):
        e.put_subex("CEVAP", np.full((rc.iy, rc.jx), np.inf))
    for n in ("REMRAT", "REMBC"):
        with pytest.raises(EngineError, match="needs rem = 1"):
            e.get_subex(n)
    for f in (-1, len(SUBEX_FIELDS), 99):
        with pytest.raises(EngineError, match="unknown field"):
            e.get_subex(f)
        with pytest.raises(EngineError, match="unknown field"):
            e.put_subex(f, np.zeros((rc.iy, rc.jx)))
    with pytest.raises(EngineError, match="read-only"):
        e.put_subex("FCC", np.zeros((rc.kz, rc.iy, rc.jx)))
    with pytest.raises(EngineError, match="put only"):
        e.get_subex("RH0")
    with pytest.raises(EngineError, match="icldfrac"):               # refused: the switch stays on
        e.set_subex(True, *args, icldfrac=1)
    # a whole step (replayed from its graph) ends a stray pre phase: the export is stale after it
    e.step(2)
    e.tend_pre_physics()
    e.step(1)
    with pytest.raises(EngineError, match="no rcmdyn_tend_pre_physics ran"):
        e.tend_post_physics()
    with pytest.raises(EngineError, match="no rcmdyn_tend_pre_physics since"):
        e.physics_subex()
    e.step(2)                                                        # usable: condtq without a put of rh0adj
    assert e.get_subex("RAINNC").max() > 0
    same(e.get_condtq("RH0ADJ"), e.get_subex("RH0ADJ"), "RH0ADJ")
