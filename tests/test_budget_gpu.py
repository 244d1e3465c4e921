"""GPU checks of the tendency budget of t and qv (the reference's idiag = 1) through the C-ABI:
rcmdyn_set_budget / rcmdyn_get_budget / rcmdyn_reset_budget (include/rcmdyn.h).

What tend does around its phases (Main/mod_tendency.F90:1276-1279, 1332-1376, 1465-1487,
1521-1530, 1557-1560, 1603-1606, 1673-1676; ten2diag :2123-2175): it snapshots the running
dynamic tendency (ten0 / qen0) and adds (ten - ten0) * rw to tdiag / qdiag %adh, adv, adi, bdy,
dif on the interior cross points.  The engine stores the same differences of the running sum
its tendency kernels hold.

Grids: C1 and N1 cut to jx = 37, iy = 29 (nspgx = nspgd = 7, kz = 18): two 32-wide block
columns with the second partial, four 8-row block rows with the last partial.  The tile cases
use C1 and N1 unchanged as 2 x 2.

Tolerances.
 - closure: at every interior point |sum of the five terms - TTEN| <= 2**-50 * A, A = sum |term|
   (five rounded differences of a telescoping sum plus four additions: fewer than 8 units of
   2**-53 * A).  Derived, not measured.
 - dif and bdy against the oracle with the process switched off: 2e-12 * max|oracle TTEN| (twice
   the one-tend bound of the totals, tests/test_parity_gpu.py: a difference of two totals).
 - adh, adv, adi against the NumPy restatements of the reference text: rtol 1e-10, atol 1e-11 *
   max|want| (tests/test_oracle_cpu.py's tolerance for these restatements).
 - everything else (non-interference, accumulation, tiles, transports) is bit for bit.
"""
import dataclasses

import numpy as np
import pytest

from regcm_amd.dycore import BUDGET_TERMS
from tests import support
from tests.dyn_ref import HYDRO_INPUTS, band_mask, hydro_stages
from tests.support import advance, case, physics_tendencies, state_names

pytestmark = pytest.mark.gpu

T_TERMS, Q_TERMS = BUDGET_TERMS[:5], BUDGET_TERMS[5:]
OFF = "the tendency budget is off"


def engine(rc, data, st, rw=None, nproc=(1, 1), diag=True):
    e = support.engine(rc, data, st, nproc, bdyval=False)
    if diag:
        e.set_diagnostics(True)
    if rw is not None:
        e.set_budget(True, rw=rw)
    e.bdyval()
    return e


def terms(e):
    return {n: e.get_budget(n) for n in BUDGET_TERMS}


def interior(rc):
    """Mask [i, j] of the interior cross points jci1:jci2 x ici1:ici2 of the whole domain (every
    point of a periodic direction)."""
    m = np.zeros((rc.iy, rc.jx), dtype=bool)
    js = slice(0, rc.jx) if rc.i_band else slice(1, rc.jx - 2)
    is_ = slice(0, rc.iy) if rc.i_crm else slice(1, rc.iy - 2)
    m[is_, js] = True
    return m


# ------------------------------------------------------------------ 1. off by default
@pytest.mark.parametrize("core", ["C", "N"])
def test_budget_off_by_default_and_refusals(core):
    from regcm_amd.dycore import EngineError
    rc, data, st = case(core)
    e = engine(rc, data, st)
    e.step(1)
    with pytest.raises(EngineError, match=OFF):
        e.get_budget("T_ADH")
    with pytest.raises(EngineError, match=OFF):
        e.reset_budget()
    for bad in (dict(rw=0.0), dict(rw=-1.0), dict(rw=float("nan")), dict(rw=float("inf")), dict(idgq=2),
                dict(idgq=0)):
        with pytest.raises(EngineError, match="rcmdyn_set_budget"):
            e.set_budget(True, **bad)
        with pytest.raises(EngineError, match=OFF):         # the refused call left it off
            e.get_budget("T_ADH")
    e.set_budget(True, rw=1.0)
    for bad in (-1, len(BUDGET_TERMS)):
        with pytest.raises(EngineError, match="unknown budget term"):
            e.get_budget(bad)
    assert all(not v.any() for v in terms(e).values())       # allocated zeroed, no tend yet
    # refused calls on a running budget change neither the switch nor rw
    ref = engine(rc, data, st, rw=1.0)
    ref.step(1)
    ref.reset_budget()                                       # e's budget was off during step 1
    for bad in (dict(rw=0.0), dict(rw=float("nan")), dict(idgq=2)):
        with pytest.raises(EngineError, match="rcmdyn_set_budget"):
            e.set_budget(True, **bad)
    e.tend()
    e.bdyval()
    ref.step(1)
    got, want = terms(e), terms(ref)
    for n in BUDGET_TERMS:
        assert np.array_equal(got[n], want[n]), n
    assert got["T_ADH"].any() and got["Q_ADH"].any()
    e.set_budget(False)
    with pytest.raises(EngineError, match=OFF):
        e.get_budget("T_ADH")


# ------------------------------------------------------------------ 2. non-interference
@pytest.mark.parametrize("path", ["step", "pair", "physics"])
@pytest.mark.parametrize("core", ["C", "N"])
def test_budget_does_not_change_the_step(core, path):
    """6 steps with the budget on and off: every state field and TTEN / QVTEN bit-identical; the
    *PHY tendencies enter no term."""
    rc, data, st = case(core)
    phy = physics_tendencies(rc) if path == "physics" else None
    off = engine(rc, data, st)
    on = engine(rc, data, st, rw=0.25)
    for e in (off, on):
        advance(e, path, 6, phy)
    for name in state_names(rc) + ["TTEN", "QVTEN"]:
        assert np.array_equal(off.get(name), on.get(name)), name
    assert off.get_time() == on.get_time()
    got = terms(on)
    assert got["T_ADH"].any() and got["Q_DIF"].any()
    if path == "physics":
        # the same trajectory needs the same *PHY in the forecast: compare one tend from the start
        a, b = engine(rc, data, st, rw=0.25), engine(rc, data, st, rw=0.25)
        advance(a, "physics", 1, phy)
        advance(b, "physics", 1, None)
        assert not np.array_equal(a.get("TTEN"), b.get("TTEN"))
        ta, tb = terms(a), terms(b)
        for n in BUDGET_TERMS:
            assert np.array_equal(ta[n], tb[n]), n


# ------------------------------------------------------------------ 3. / 7. closure
def check_closure(rc, data, st, nproc=(1, 1)):
    e = engine(rc, data, st, rw=1.0, nproc=nproc)
    e.tend()
    got = terms(e)
    m = interior(rc)
    nh = rc.idynamic == 2
    k0 = rc.rayndamp if (nh and rc.ifrayd == 1 and not rc.i_crm) else 0   # Rayleigh-damped levels enter no term
    for names, total in ((T_TERMS, "TTEN"), (Q_TERMS, "QVTEN")):
        tot = e.get(total)
        s = np.zeros_like(tot)
        a = np.zeros_like(tot)
        for n in names:                                   # adh, adv, adi, bdy, dif in this order
            s = s + got[n]
            a = a + np.abs(got[n])
            assert not got[n][:, ~m].any(), (n, "outside the interior")
            assert np.isfinite(got[n]).all(), n
        err = np.abs(s - tot)[k0:, m]
        bound = (2.0 ** -50 * a)[k0:, m]
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"{rc.jx}x{rc.iy} idynamic={rc.idynamic} {total}: worst |sum - total| / (2^-50 A) = {worst:.3f}, max A = {a.max():.3e}")
        assert a[k0:, m].max() > 0.0
        assert (err <= bound).all(), (total, worst)
    # the terms the reference never writes, or writes as an exact zero
    zeros = ["T_ADV", "T_ADI"] if nh else ["Q_ADI"]
    if rc.iboudy in (0, 2, 3):
        zeros += ["T_BDY", "Q_BDY"]
    for n in zeros:
        assert not got[n].any(), n
    for n in set(BUDGET_TERMS) - set(zeros):
        assert got[n].any(), n
    return got


CLOSURE = [("C", {}), ("C", {"iboudy": 4}), ("C", {"iboudy": 2}),
           ("N", {"ifrayd": 0}), ("N", {"ifrayd": 0, "iboudy": 4}), ("N", {"ifrayd": 0, "iboudy": 2}), ("N", {})]
VARIANTS = [(c, v) for v in ({"idiffu": 2}, {"idiffu": 3}, {"isladvec": 1}, {"ipptls": 2}, {"upstream_mode": 0})
            for c in ("C", "N")] + [("C", {"i_band": 1}), ("CRM", {})]


def _cid(p):
    return p[0] + "," + (",".join(f"{k}={x}" for k, x in p[1].items()) or "default")


@pytest.mark.parametrize("p", CLOSURE + VARIANTS, ids=_cid)
def test_budget_closes_on_the_total_tendency(p):
    """One tend from the start state, rw = 1, no *PHY: the five terms sum to TTEN (QVTEN)."""
    rc, data, st = case(p[0], **p[1])
    check_closure(rc, data, st)


# ------------------------------------------------------------------ 4. dif and bdy against the oracle
@pytest.mark.parametrize("core", ["C", "N"])
def test_dif_and_bdy_match_the_oracle_with_the_process_off(core):
    from oracle.oracle import OracleCore
    rc, data, st = case(core)
    tot = {}
    for tag, opts in (("full", {}), ("nodif", {"ckh": 0.0, "adyndif": 0.0}),
                      ("nobdy", {"ckh": 0.0, "adyndif": 0.0, "iboudy": 2})):
        rcv = dataclasses.replace(rc, **opts)
        o = OracleCore(rcv, data["split"])
        o.put_state(st)
        o.bdyval()
        o.tend()
        tot[tag] = {n: o.get(n) for n in ("TTEN", "QVTEN")}
        o.close()
    e = engine(rc, data, st, rw=1.0)
    e.tend()
    got = terms(e)
    m = interior(rc)
    band = band_mask(rc)
    assert band.sum() == 500
    for total, dif, bdy in (("TTEN", "T_DIF", "T_BDY"), ("QVTEN", "Q_DIF", "Q_BDY")):
        full = tot["full"][total]
        scale = np.abs(full[:, m]).max()
        want_dif = full - tot["nodif"][total]
        want_bdy = tot["nodif"][total] - tot["nobdy"][total]
        assert not want_bdy[:, m & ~band].any()
        assert (np.abs(want_bdy[:, m & band]).max(axis=0) > 0).all()     # non-zero on every band column
        for name, want in ((dif, want_dif), (bdy, want_bdy)):
            share = np.abs(want[:, m]).max() / scale
            err = np.abs(got[name] - want)[:, m].max()
            print(f"{rc.jx}x{rc.iy} idynamic={rc.idynamic} {name}: oracle max / total max = {share:.3e}, |engine - oracle| / max|{total}| = "
                  f"{err / scale:.3e}")
            assert share >= 1e-4, (name, share)
            assert err <= 2e-12 * scale, (name, err / scale)


# ------------------------------------------------------------------ 5. adh, adv, adi against the reference text
def _close(got, want, name):
    assert np.abs(want).max() > 0.0, name
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg=name)


NH_INPUTS = ("ATM1_U", "ATM1_V", "ATM1_T", "ATM1_PP", "ATM1_W", "ATM1_QV", "PSA", "MSFX", "MSFD", "ATM0_PR",
             "ATM0_PS", "ATM0_RHOF", "DPSDXM", "DPSDYM")


def off_band(rc):
    nsp = rc.nspgx
    J = np.arange(nsp + 1, rc.jx - nsp)
    I = np.arange(nsp + 1, rc.iy - nsp)
    return (slice(None), (I - 1)[:, None], (J - 1)[None, :])


def test_hydrostatic_terms_match_the_numpy_restatement():
    """Each term is the difference of two of the restatement's running sums: off the band for adh,
    adv, adi; at every interior point for the relaxation of t."""
    rc, data, st = case("C")
    e = engine(rc, data, st, rw=1.0)
    g = {n: e.get(n) for n in HYDRO_INPUTS}
    _, dt0, xbc = e.get_time()
    e.tend()
    got = terms(e)
    r = hydro_stages(rc, g, dt0, xbc)
    s1, s2, s3, s4, q1s, q2s = r["s1"], r["s2"], r["s3"], r["s4"], r["q1"], r["q2"]
    sl = off_band(rc)
    Jc = np.arange(2, rc.jx - 1)
    Ic = np.arange(2, rc.iy - 1)
    sc = (slice(None), (Ic - 1)[:, None], (Jc - 1)[None, :])     # every interior point
    _close(got["T_ADH"][sl], (s1 - 0.0)[sl], "T_ADH")
    _close(got["T_ADV"][sl], (s2 - s1)[sl], "T_ADV")
    _close(got["T_ADI"][sl], (s3 - s2)[sl], "T_ADI")
    _close(got["T_BDY"][sc], (s4 - s3)[sc], "T_BDY")
    _close(got["Q_ADH"][sl], (q1s - 0.0)[sl], "Q_ADH")
    _close(got["Q_ADV"][sl], (q2s - q1s)[sl], "Q_ADV")


def nh_stages(rc, g):
    """Off the band, from the state g after bdyval: the NH t tendency of the theta path atm1%t *
    thten / tha (ithadv = 1), and the running sum of the qv tendency after hadvqv (q1), vadvqv
    (q2) and atmx%qx * cr (q3) (the staged restatements of tests/test_oracle_cpu.py::
    _nh_tend_restatement and its two tests)."""
    from regcm_amd import constants as C
    kz, nsp = rc.kz, rc.nspgx
    sig = rc.sigma
    hsig = (sig[1:] + sig[:-1]) * 0.5
    dsig = sig[1:] - sig[:-1]
    twt1 = np.zeros(kz + 1); twt2 = np.zeros(kz + 1)
    for k in range(2, kz + 1):
        twt1[k] = (sig[k - 1] - hsig[k - 2]) / (hsig[k - 1] - hsig[k - 2])
        twt2[k] = 1.0 - twt1[k]
    dx = rc.ds * 1000.0
    J = np.arange(nsp + 1, rc.jx - nsp)
    I = np.arange(nsp + 1, rc.iy - nsp)

    def at(a, dj=0, di=0):
        return a[:, (I + di - 1)[:, None], (J + dj - 1)[None, :]]

    ps = at(g["PSA"])[0]
    msfx, msfd = at(g["MSFX"])[0], g["MSFD"]
    umc = g["ATM1_U"] * msfd[0][None]
    vmc = g["ATM1_V"] * msfd[0][None]
    pa = g["PSA"][0]
    psd = np.zeros_like(pa)
    psd[1:, 1:] = (pa[1:, 1:] + pa[:-1, 1:] + pa[1:, :-1] + pa[:-1, :-1]) * 0.25
    rpsd = np.divide(1.0, psd, out=np.zeros_like(psd), where=psd > 0)
    umd = g["ATM1_U"] * rpsd[None] * msfd[0][None]
    vmd = g["ATM1_V"] * rpsd[None] * msfd[0][None]
    ucc = at(umd) + at(umd, 0, 1) + at(umd, 1, 0) + at(umd, 1, 1)
    vcc = at(vmd) + at(vmd, 0, 1) + at(vmd, 1, 0) + at(vmd, 1, 1)
    pinv = np.divide(1.0, pa, out=np.zeros_like(pa), where=pa > 0)
    xw = g["ATM1_W"] * pinv[None]
    egrav = 9.80665
    qdot = np.zeros((kz + 1,) + ps.shape)
    for k in range(2, kz + 1):
        qdot[k - 1] = (-at(g["ATM0_RHOF"])[k - 1] * egrav * at(xw)[k - 1] / at(g["ATM0_PS"])[0] -
                       sig[k - 1] * (at(g["DPSDXM"])[0] * (twt1[k] * ucc[k - 1] + twt2[k] * ucc[k - 2]) +
                                     at(g["DPSDYM"])[0] * (twt1[k] * vcc[k - 1] + twt2[k] * vcc[k - 2])))
    a = at(umc, 1, 1) + at(umc, 1, 0) - at(umc, 0, 1) - at(umc)
    b = at(vmc, 1, 1) + at(vmc, 0, 1) - at(vmc, 1, 0) - at(vmc)
    dummy = 1.0 / (2.0 * dx * msfx * msfx)
    cr = (a + b) * dummy[None] + (qdot[1:] - qdot[:-1]) * ps[None] / dsig[:, None, None]
    u1 = at(umc, 0, 1) + at(umc)
    u2 = at(umc, 1, 1) + at(umc, 1, 0)
    v1 = at(vmc, 1, 0) + at(vmc)
    v2 = at(vmc, 1, 1) + at(vmc, 0, 1)
    ul = rc.uoffc * 0.5 * rc.dt / dx
    f1 = 0.5 * ul * (u2 + u1) / ps[None]
    f2 = 0.5 * ul * (v2 + v1) / ps[None]
    xmsf = 1.0 / (msfx * msfx * (4.0 * dx))

    def hadv(c, w, e_, s_, n):
        fx1 = (1.0 + f1) * w + (1.0 - f1) * c
        fx2 = (1.0 + f1) * c + (1.0 - f1) * e_
        fy1 = (1.0 + f2) * s_ + (1.0 - f2) * c
        fy2 = (1.0 + f2) * c + (1.0 - f2) * n
        return -xmsf[None] * (u2 * fx2 - u1 * fx1 + v2 * fy2 - v1 * fy1)

    # ---- t: the theta path
    rgas = C.rgas
    cpd = 3.5 * rgas
    rovcp = rgas * (1.0 / cpd)
    with np.errstate(divide="ignore", invalid="ignore"):
        thf = (g["ATM1_T"] * pinv[None]) * (1.0e5 / (g["ATM0_PR"] + g["ATM1_PP"] * pinv[None])) ** rovcp
    th, thw, the, ths, thn = at(thf), at(thf, -1), at(thf, 1), at(thf, 0, -1), at(thf, 0, 1)
    fg = hadv(th, thw, the, ths, thn)
    for (p, m) in ((thn, ths), (the, thw)):
        big = np.abs(p + m - 2.0 * th) / ps[None] > rc.t_extrema
        fg = np.where(big & (th > p) & (th > m), np.minimum(fg, 0.0), fg)
        fg = np.where(big & (th < p) & (th < m), np.maximum(fg, 0.0), fg)
    tha = th * ps[None]
    thten = 0.0 + fg
    for k in range(2, kz + 1):
        fx = qdot[k - 1] * (twt1[k] * tha[k - 1] + twt2[k] * tha[k - 2])
        thten[k - 2] = thten[k - 2] - fx * (1.0 / dsig[k - 2])
        thten[k - 1] = thten[k - 1] + fx * (1.0 / dsig[k - 1])
    thten = thten + th * cr
    tdyn = at(g["ATM1_T"]) * thten / tha
    # ---- qv
    minqq, dlowval = 1.0e-8, 1.0e-20
    xds = 1.0 / dsig
    q1 = g["ATM1_QV"]
    xq = np.maximum(q1 * pinv[None], minqq)
    c, w, e_, s_, n = at(xq), at(xq, -1), at(xq, 1), at(xq, 0, -1), at(xq, 0, 1)
    fg = hadv(c, w, e_, s_, n)
    den = np.maximum(c, dlowval)
    for (p, m) in ((n, s_), (e_, w)):
        big = np.abs(p + m - 2.0 * c) / den > rc.q_rel_extrema
        fg = np.where(big & (c > p) & (c > m), np.minimum(fg, 0.0), fg)
        fg = np.where(big & (c < p) & (c < m), np.maximum(fg, 0.0), fg)
    q1s = 0.0 + fg                                               # after hadvqv
    q2s = q1s.copy()                                             # after vadvqv
    f = at(q1)
    for k in range(2, kz + 1):
        qcon = (sig[k - 1] - hsig[k - 1]) / (hsig[k - 2] - hsig[k - 1])
        fk, fkm = f[k - 1], f[k - 2]
        ok = (fk > minqq * ps) & (fkm > minqq * ps)
        with np.errstate(divide="ignore", invalid="ignore"):
            flux = qdot[k - 1] * np.where(ok, fk * (fkm / fk) ** qcon, 0.0)
        q2s[k - 2] = q2s[k - 2] - flux * xds[k - 2]
        q2s[k - 1] = q2s[k - 1] + flux * xds[k - 1]
    q3s = q2s + c * cr                                           # after atmx%qx * cr
    return dict(tdyn=tdyn, q1=q1s, q2=q2s, q3=q3s)


def test_nonhydrostatic_terms_match_the_numpy_restatement():
    """T_ADH is the whole theta path; the qv terms are the differences of the restatement's running
    sums; off the band."""
    rc, data, st = case("N")
    e = engine(rc, data, st, rw=1.0)
    g = {n: e.get(n) for n in NH_INPUTS}
    e.tend()
    got = terms(e)
    r = nh_stages(rc, g)
    sl = off_band(rc)
    _close(got["T_ADH"][sl], r["tdyn"] - 0.0, "T_ADH")
    _close(got["Q_ADH"][sl], r["q1"] - 0.0, "Q_ADH")
    _close(got["Q_ADV"][sl], r["q2"] - r["q1"], "Q_ADV")
    _close(got["Q_ADI"][sl], r["q3"] - r["q2"], "Q_ADI")


# ------------------------------------------------------------------ 6. accumulation and reset
@pytest.mark.parametrize("core", ["C", "N"])
def test_budget_accumulates_and_resets(core):
    rc, data, st = case(core)
    b = engine(rc, data, st, rw=1.0, diag=False)          # read and reset after every step
    per_step = []
    for _ in range(5):
        b.step(1)
        per_step.append(terms(b))
        b.reset_budget()
        assert all(not v.any() for v in terms(b).values())
    a = engine(rc, data, st, rw=0.2, diag=False)          # never reset, one rcmdyn_step(5)
    a.step(5)
    a2 = engine(rc, data, st, rw=0.2, diag=False)         # five tend + bdyval pairs
    advance(a2, "pair", 5)
    ga, ga2 = terms(a), terms(a2)
    for n in BUDGET_TERMS:
        acc = np.zeros_like(ga[n])
        for s in range(5):
            acc = acc + per_step[s][n] * 0.2
        assert np.array_equal(ga[n], acc), n
        assert np.array_equal(ga2[n], ga[n]), n
    a.reset_budget()
    for n, v in terms(a).items():
        assert not v.any() and not np.signbit(v).any(), n
    # a new rw holds from the next tend on (the captured graphs are dropped)
    c = engine(rc, data, st, rw=1.0, diag=False)
    c.step(2)
    before = terms(c)
    c.set_budget(True, rw=0.5)
    c.step(1)
    after = terms(c)
    for n in BUDGET_TERMS:
        assert np.array_equal(before[n], (np.zeros_like(before[n]) + per_step[0][n] * 1.0) + per_step[1][n] * 1.0), n
        assert np.array_equal(after[n], before[n] + per_step[2][n] * 0.5), n


# ------------------------------------------------------------------ 7. tiles and transports
@pytest.mark.parametrize("transport", ["copy", "rccl"])
@pytest.mark.parametrize("name", ["C1", "N1"])
def test_budget_tiles_match_one_tile(name, transport, monkeypatch):
    rc, data, st = case(name)
    one = engine(rc, data, st, rw=1.0, diag=False)
    if transport == "rccl":
        monkeypatch.setenv("RCMDYN_FORCE_RCCL", "1")
    dec = engine(rc, data, st, rw=1.0, nproc=(2, 2), diag=False)
    one.step(3)
    dec.step(3)
    a, b = terms(one), terms(dec)
    m = interior(rc)
    for n in BUDGET_TERMS:
        assert np.array_equal(a[n], b[n]), n
        assert not b[n][:, ~m].any(), n
    assert b["T_ADH"].any() and b["Q_DIF"].any()


@pytest.mark.parametrize("nproc", [(1, 1), (2, 2)], ids=str)
def test_budget_two_launches_match_the_fused_update(nproc, monkeypatch):
    """k_momentum and k_scalars as two launches (RCMDYN_NO_FUSE_UPDATE: the budget instance of
    k_scalars itself, with the overlap parts on tiles) give the fused launch's terms bit for bit."""
    rc, data, st = case("C1")
    fused = engine(rc, data, st, rw=1.0, nproc=nproc, diag=False)
    monkeypatch.setenv("RCMDYN_NO_FUSE_UPDATE", "1")
    two = engine(rc, data, st, rw=1.0, nproc=nproc, diag=False)
    fused.step(3)
    two.step(3)
    a, b = terms(fused), terms(two)
    for n in BUDGET_TERMS:
        assert np.array_equal(a[n], b[n]), n
    assert b["T_DIF"].any() and b["Q_ADV"].any()
