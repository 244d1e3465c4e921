"""GPU checks of the device mass check of tend through the C-ABI: rcmdyn_set_massck /
rcmdyn_get_massck (include/rcmdyn.h; regcm_amd/csrc/massck.hip).

The yardstick is a NumPy restatement of the reference text (Main/mod_massck.F90:190-306, the
idynamic /= 3 branch), with the reference's ranges and signs, per tile of the decomposition, from
the fields the engine returns before each tend; it is not an execution of the reference.

Grids: C1 and N1 cut to jx = 37, iy = 29 (kz = 18): a partial last 64-lane column and a partial
last chunk of 16 interior rows, more than one row chunk.  The tile cases use C1 and N1 unchanged as
2 x 2; the periodic cases the i_band = 1 hydrostatic variant and CONFIGS["CRM"].

Tolerance of each sum (derived, not measured): |got - want| <= (n + 16) * 2**-52 * A, with n the
number of leaf summands and A the sum of |leaf| after scaling: either side's summation in any
order errs by at most (n - 1) * 2**-53 * A, and the at most eight roundings inside a leaf add
8 * 2**-53 * |leaf| per side.  Everything else (non-interference, paths, ring, transports of the
same decomposition) is bit for bit.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from regcm_amd.config import FIELD, TWO_D, build_config
from regcm_amd.constants import egrav
from regcm_amd.dycore import BUDGET_TERMS
from tests import support
from tests.support import advance, case, physics_tendencies, state_names

pytestmark = pytest.mark.gpu

OFF = "the mass check is off"
SUMS = ("drymass", "dryadv", "qmass", "qadv")          # columns 2..5 of a record


def engine(rc, data, st, cap=None, nproc=(1, 1), budget=False, diag=False):
    e = support.engine(rc, data, st, nproc, bdyval=False)
    if diag:
        e.set_diagnostics(True)
    if budget:
        e.set_budget(True, rw=0.25)
    if cap is not None:
        e.set_massck(True, cap)
    e.bdyval()
    return e


def qnames(rc):
    return ["ATM1_QV", "ATM1_QC"] + (["ATM1_QI", "ATM1_QR", "ATM1_QS"] if rc.nqx == 5 else [])


def inputs(e, rc):
    """What massck reads, as the engine holds it before a tend, and the clock."""
    f = {n: e.get(n) for n in ["ATM1_U", "ATM1_V", "PSA"] + qnames(rc)}
    return f, e.get_time()


# ------------------------------------------------------------------ the reference text in NumPy
def reference(rc, f, dt, nproc=(1, 1), lines="wesn"):
    """Main/mod_massck.F90:190-306 over every tile of the decomposition.  f: global arrays
    [k - 1, i - 1, j - 1]; a ghost point of a periodic direction is the wrapped one.  Returns
    {sum: (value, A, n)}: the value, the sum of |leaf| and the number of leaves."""
    from regcm_amd.dycore import tile_extent
    jx, iy, kz = rc.jx, rc.iy, rc.kz
    dx = rc.ds * 1000.0
    dxsq = dx * dx
    regrav = 1.0 / egrav
    sigma = rc.sigma
    dsigma = np.array([sigma[k + 1] - sigma[k] for k in range(kz)])
    u, v, psa = f["ATM1_U"], f["ATM1_V"], f["PSA"][0]
    qx = [f[n] for n in qnames(rc)]
    coef = dt * 3.e4 * dsigma * dx * regrav                      # per level, left to right
    val = dict.fromkeys(SUMS, 0.0)
    A = dict.fromkeys(SUMS, 0.0)
    n = dict.fromkeys(SUMS, 0)
    for tile in range(nproc[0] * nproc[1]):
        (jde1, jde2, ide1, ide2, jce1, jce2, ice1, ice2), (left, right, bottom, top) = \
            tile_extent(jx, iy, nproc[0], nproc[1], tile, rc.i_band, rc.i_crm)
        jci1, jci2 = jce1 + (1 if left else 0), jce2 - (1 if right else 0)
        ici1, ici2 = ice1 + (1 if bottom else 0), ice2 - (1 if top else 0)
        J, I = slice(jci1 - 1, jci2), slice(ici1 - 1, ici2)
        # internal dry air mass (:190-198, 235)
        tttmp = psa[I, J].sum()
        tdrym = 0.0
        for k in range(kz):
            tdrym = tdrym + tttmp * dsigma[k]
        val["drymass"] += tdrym * dxsq * 1000.0 * regrav
        A["drymass"] += (np.abs(psa[I, J])[None] * dsigma[:, None, None] * dxsq * 1000.0 * regrav).sum()
        n["drymass"] += kz * psa[I, J].size
        # moisture (:256-265, 306)
        tqmass = 0.0
        for q in qx:
            for k in range(kz):
                tttmp = q[k][I, J].sum()
                tqmass = tqmass + tttmp * dsigma[k]
            A["qmass"] += (np.abs(q[:, I, J]) * dsigma[:, None, None] * dxsq * 1000.0 * regrav).sum()
            n["qmass"] += q[:, I, J].size
        val["qmass"] += tqmass * dxsq * 1000.0 * regrav
        # boundary input (:203-234, 269-304): (has, sign, wind sum [k, point], cross indices)
        ii = np.arange(ice1, ice2 + 1)                 # i = ice1 .. ice2
        jj = np.arange(jci1, jci2 + 1)                 # j = jci1 .. jci2
        sides = []
        if left and "w" in lines:
            sides.append((+1, u[:, ii % iy, jde1 - 1] + u[:, ii - 1, jde1 - 1], ii - 1, np.full_like(ii, jce1 - 1)))
        if right and "e" in lines:
            sides.append((-1, u[:, ii % iy, jde2 - 1] + u[:, ii - 1, jde2 - 1], ii - 1, np.full_like(ii, jce2 - 1)))
        if bottom and "s" in lines:
            sides.append((+1, v[:, ide1 - 1, jj % jx] + v[:, ide1 - 1, jj - 1], np.full_like(jj, ice1 - 1), jj - 1))
        if top and "n" in lines:
            sides.append((-1, v[:, ide2 - 1, jj % jx] + v[:, ide2 - 1, jj - 1], np.full_like(jj, ice2 - 1), jj - 1))
        for sign, wind, ic, jc in sides:
            leaf = coef[:, None] * wind
            val["dryadv"] += sign * leaf.sum()
            A["dryadv"] += np.abs(leaf).sum()
            n["dryadv"] += leaf.size
            for q in qx:
                leaf = coef[:, None] * (wind * (q[:, ic, jc] / psa[ic, jc][None]))
                val["qadv"] += sign * leaf.sum()
                A["qadv"] += np.abs(leaf).sum()
                n["qadv"] += leaf.size
    return {s: (val[s], A[s], n[s]) for s in SUMS}


def bound(n, a):
    return (n + 16) * 2.0 ** -52 * a


def check_record(tag, rec, want, clock):
    assert rec[0] == clock[0] and rec[1] == clock[1], (tag, rec[:2], clock)
    for q, s in enumerate(SUMS):
        w, a, n = want[s]
        err, b = abs(rec[2 + q] - w), bound(n, a)
        print(f"{tag} {s}: got {rec[2 + q]:.17e} want {w:.17e} |diff| {err:.3e} bound {b:.3e} "
              f"(n = {n}, A = {a:.6e})")
        assert err <= b, (tag, s, err, b)


def run_against_reference(rc, data, st, nsteps=3, nproc=(1, 1), lines="wesn"):
    e = engine(rc, data, st, cap=8, nproc=nproc)
    wants, clocks = [], []
    for _ in range(nsteps):
        f, clock = inputs(e, rc)
        wants.append(reference(rc, f, clock[1], nproc, lines))
        clocks.append(clock)
        e.tend()
        e.bdyval()
    recs, lost = e.get_massck()
    assert recs.shape == (nsteps, 6) and lost == 0
    for q in range(nsteps):
        check_record(f"step {q}", recs[q], wants[q], clocks[q])
    return recs, wants, clocks


# ------------------------------------------------------------------ 1. against the reference text
@pytest.mark.parametrize("core,kw", [("C", {}), ("N", {}), ("C", {"ipptls": 2}), ("N", {"ipptls": 2})],
                         ids=["C", "N", "C,ipptls=2", "N,ipptls=2"])
def test_massck_matches_the_reference_text(core, kw):
    rc, data, st = case(core, **kw)
    recs, wants, clocks = run_against_reference(rc, data, st)
    assert [c[0] for c in clocks] == [0, 1, 2]
    assert clocks[0][1] == rc.dt and clocks[2][1] == 2.0 * rc.dt       # dtsec, then the leapfrog 2 dtsec
    for w in wants:
        for s in SUMS:
            assert w[s][1] > 0.0, s                   # flow and moisture on every boundary line
    assert (recs[:, 3] != 0.0).all() and (recs[:, 5] != 0.0).all()
    assert (recs[:, 2] > 0.0).all() and (recs[:, 4] > 0.0).all()


# ------------------------------------------------------------------ 2. periodic sides
def test_massck_band_has_no_west_and_east_lines():
    rc, data, st = case("C", i_band=1)
    recs, wants, _ = run_against_reference(rc, data, st, lines="sn")      # the south + north sums only
    assert (recs[:, 3] != 0.0).all() and (recs[:, 5] != 0.0).all()
    # two lines over every j of the periodic direction, and every j in the interior
    assert wants[0]["dryadv"][2] == 2 * rc.kz * rc.jx
    assert wants[0]["drymass"][2] == rc.kz * rc.jx * (rc.iy - 3)


def test_massck_crm_has_no_lines_and_takes_every_point():
    rc, data, st = case("CRM")
    recs, wants, _ = run_against_reference(rc, data, st)
    assert (recs[:, 3] == 0.0).all() and (recs[:, 5] == 0.0).all()       # exactly 0.0
    assert wants[0]["drymass"][2] == rc.kz * rc.jx * rc.iy and wants[0]["dryadv"][2] == 0
    assert (recs[:, 2] > 0.0).all() and (recs[:, 4] > 0.0).all()


# ------------------------------------------------------------------ 3. no effect on the step
@pytest.mark.parametrize("budget", [False, True], ids=["", "budget"])
@pytest.mark.parametrize("path", ["step", "pair", "physics"])
@pytest.mark.parametrize("core", ["C", "N"])
def test_massck_does_not_change_the_step(core, path, budget):
    rc, data, st = case(core)
    phy = physics_tendencies(rc) if path == "physics" else None
    off = engine(rc, data, st, budget=budget, diag=True)
    on = engine(rc, data, st, cap=16, budget=budget, diag=True)
    for e in (off, on):
        advance(e, path, 6, phy)
    for name in state_names(rc) + ["TTEN", "QVTEN"]:
        assert np.array_equal(off.get(name), on.get(name)), name
    assert off.get_time() == on.get_time()
    if budget:
        for n in BUDGET_TERMS:
            assert np.array_equal(off.get_budget(n), on.get_budget(n)), n
        assert on.get_budget("T_ADH").any()
    recs, lost = on.get_massck()
    assert recs.shape == (6, 6) and lost == 0 and list(recs[:, 0]) == [0, 1, 2, 3, 4, 5]


# ------------------------------------------------------------------ 4. one log on every path
@pytest.mark.parametrize("core", ["C", "N"])
def test_massck_log_is_the_same_on_every_path(core):
    rc, data, st = case(core)
    logs = {}
    for path in ("step", "pair", "physics", "step again"):
        e = engine(rc, data, st, cap=8)
        advance(e, path.split()[0], 5)
        logs[path], lost = e.get_massck()
        assert logs[path].shape == (5, 6) and lost == 0
        assert e.get_massck()[0].shape == (0, 6)            # the read emptied the log
    for path in ("pair", "physics", "step again"):           # 'step again': a second engine built alike
        assert np.array_equal(logs["step"], logs[path]), path
    e = engine(rc, data, st, cap=8)
    e.step(2)
    a, la = e.get_massck()
    e.step(3)
    b, lb = e.get_massck()
    assert la == 0 and lb == 0 and a.shape == (2, 6) and b.shape == (3, 6)
    assert np.array_equal(np.concatenate([a, b]), logs["step"])


# ------------------------------------------------------------------ 5. ring
def test_massck_ring_keeps_the_newest_records():
    rc, data, st = case("C")
    big = engine(rc, data, st, cap=8)
    big.step(6)
    want, _ = big.get_massck()
    e = engine(rc, data, st, cap=2)
    e.step(5)
    got, lost = e.get_massck()
    assert got.shape == (2, 6) and lost == 3
    assert np.array_equal(got, want[3:5])
    e.step(1)
    got, lost = e.get_massck()
    assert got.shape == (1, 6) and lost == 0
    assert np.array_equal(got[0], want[5])


# ------------------------------------------------------------------ 6. refusals
def test_massck_off_by_default_and_refusals():
    from regcm_amd.dycore import EngineError
    rc, data, st = case("C")
    e = engine(rc, data, st)
    e.step(1)
    with pytest.raises(EngineError, match=OFF):
        e.get_massck()
    for cap in (0, -1, 65537):
        with pytest.raises(EngineError, match="rcmdyn_set_massck"):
            e.set_massck(True, cap)
        with pytest.raises(EngineError, match=OFF):          # the refused call left it off
            e.get_massck()
    ref = engine(rc, data, st)
    ref.step(1)
    ref.set_massck(True, 4)
    e.set_massck(True, 4)
    for cap in (0, -1, 65537):                               # refused on a running check: it keeps running
        with pytest.raises(EngineError, match="rcmdyn_set_massck"):
            e.set_massck(True, cap)
    e.set_massck(True, 4)                                    # the same on and cap: the log is kept
    e.step(1)
    ref.step(1)
    got, lost = e.get_massck()
    want, _ = ref.get_massck()
    assert got.shape == (1, 6) and lost == 0 and np.array_equal(got, want)
    assert got[0, 0] == 1 and got[0, 2] > 0.0
    e.set_massck(False)
    with pytest.raises(EngineError, match=OFF):
        e.get_massck()


# ------------------------------------------------------------------ 7. tiles and transports
@pytest.mark.parametrize("transport", ["copy", "rccl"])
@pytest.mark.parametrize("name", ["C1", "N1"])
def test_massck_tiles_match_one_tile(name, transport, monkeypatch):
    rc, data, st = case(name)
    one = engine(rc, data, st, cap=4)
    if transport == "rccl":
        monkeypatch.setenv("RCMDYN_FORCE_RCCL", "1")
    dec = engine(rc, data, st, cap=4, nproc=(2, 2))
    wants, clocks = [], []
    for _ in range(3):
        f, clock = inputs(one, rc)
        assert clock == dec.get_time()
        wants.append(reference(rc, f, clock[1], (2, 2)))
        single = reference(rc, f, clock[1])
        for s in SUMS:                                       # the restatement itself: per tile against one tile
            assert wants[-1][s][2] == single[s][2]
            assert abs(wants[-1][s][0] - single[s][0]) <= bound(single[s][2], single[s][1]), s
        clocks.append(clock)
        one.step(1)
        dec.step(1)
    a, _ = one.get_massck()
    b, _ = dec.get_massck()
    assert a.shape == (3, 6) and b.shape == (3, 6)
    assert np.array_equal(a[:, :2], b[:, :2])
    for q in range(3):
        check_record(f"{name} {transport} 2x2 step {q}", b[q], wants[q], clocks[q])
        check_record(f"{name} one tile step {q}", a[q], wants[q], clocks[q])
        for c, s in enumerate(SUMS):
            w, amp, n = wants[q][s]
            assert abs(a[q, 2 + c] - b[q, 2 + c]) <= bound(n, amp), (q, s)


# ------------------------------------------------------------------ 8. off path
@pytest.mark.parametrize("name,nproc", [("C", (1, 1)), ("N", (1, 1)), ("C1", (2, 2))], ids=["C", "N", "C1 2x2"])
def test_massck_off_issues_no_launch(name, nproc):
    rc, data, st = case(name)
    off = engine(rc, data, st, nproc=nproc).kernel_times(2)
    on = engine(rc, data, st, cap=4, nproc=nproc).kernel_times(2)
    assert not [k for k in off if "massck" in k]
    ntile = nproc[0] * nproc[1]
    assert on["k_massck"][0] == 2 * ntile and on["k_massck_final"][0] == 2
    rest = {k: v[0] for k, v in on.items() if "massck" not in k}
    assert rest == {k: v[0] for k, v in off.items()}
    assert list(rest) == list(off)                           # in the same order of first launch


# ------------------------------------------------------------------ 9. Fortran host
def test_massck_through_the_fortran_host():
    """One hydrostatic script through regcm_amd/fortran/test_shim (ops 26, 27) and through the
    Python host: switch on, three steps, read the log; the same bits."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fdir = os.path.join(root, "regcm_amd", "fortran")
    subprocess.run(["make", "-s", "-C", fdir], check=True)
    rc, data, st = case("C")
    CREATE, DESTROY, PUT, BDYVAL, STEP, SET_MASSCK, GET_MASSCK, END = 1, 2, 3, 6, 7, 26, 27, 0
    cfg = build_config(rc, data["split"])
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as fh:
            raw = bytes(cfg)
            fh.write(struct.pack("<i", len(raw)) + raw + struct.pack("<i", CREATE))
            for name, a in st.items():
                a = np.ascontiguousarray(a, dtype=np.float64)
                nk, ni, nj = a.shape
                dims = 2 if name in TWO_D and nk == 1 else 3
                fh.write(struct.pack("<9i", PUT, dims, FIELD[name], 1, nj, 1, ni, 1, nk) + a.tobytes())
            fh.write(struct.pack("<3i", SET_MASSCK, 1, 8) + struct.pack("<i", BDYVAL) + struct.pack("<2i", STEP, 3))
            fh.write(struct.pack("<2i", GET_MASSCK, 8) + struct.pack("<i", DESTROY) + struct.pack("<i", END))
        subprocess.run([os.path.join(fdir, "test_shim"), fin, fout], check=True, timeout=120)
        buf = open(fout, "rb").read()
    count, lost = struct.unpack_from("<iq", buf, 0)
    fo = np.frombuffer(buf, dtype=np.float64, count=6 * count, offset=12).reshape(count, 6)
    assert len(buf) == 12 + 48 * count
    e = engine(rc, data, st, cap=8)
    e.step(3)
    py, plost = e.get_massck()
    assert count == 3 and lost == 0 and plost == 0
    assert np.array_equal(py, fo)
