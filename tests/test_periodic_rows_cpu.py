"""The oracle against tests/dyn_ref.py and tests/tke_ref.py on the periodic grids and in the
non-hydrostatic core: the band (i_band = 1) of both cores, the cloud-resolving grid (i_crm = 1), and
the UW TKE of the non-hydrostatic core on a limited area.  The restatements are NumPy written from the
Fortran text and read neither the oracle nor the engine; tests/test_periodic_rows_gpu.py holds the
engine to them with the helpers of this file.

Grids (GRIDS), the smallest odd and even shapes on which every line, ring and wrap column is distinct
from the interior:
  HB   C1 cut to 37 x 29 and to 34 x 23 (nspgx = nspgd = 7, kz 18), i_band = 1, ibltyp = 2
  NL   N1 cut to 37 x 29, ibltyp = 2 (a limited area: the non-hydrostatic qdot and calc_coeff)
  NB   the CRM configuration cut to 37 x 29 with i_crm = 0, iboudy = 5, ibltyp = 2 (kz 23)
  CRM  the CRM configuration cut to 37 x 29 and to 34 x 23 (kz 23)
Variants: default, idiffu = 2, upstream_mode = 0, and iboudy = 4 on HB and NB.  idiffu = 3 is left to
the limited-area cases of tests/test_dyn_rows_* and tests/test_tke_rows_*: its stencil is clamped to
the global 1 and jx - 1 / iy - 1 with no periodic branch (Main/mod_diffusion.F90:605-617), so what it
reads past the end of a period is not a question of the wrap.

Inputs (non_uniform).  The generated statics of the CRM configuration are uniform (MSFX = MSFD = 1, p*
uniform, DPSDXM = DPSDYM = 0), so a static field read from the wrong side of the period gives the same
bits.  The formulas read them as data, so the tests put non-uniform ones: MSFX and MSFD are multiplied
by 1 + 0.01 * pattern, DPSDXM and DPSDYM of the non-hydrostatic core are set to 1e-5 * pattern, HT takes 50 m * (1 + pattern) more where diffu_hgtf = 1
reads it (the hydrostatic core), and on
every grid periodic in j PSA = PSB is multiplied by 1 + a * pattern, the state coupled with p* and the
boundary values keeping their decoupled values.  Each field takes a pattern of its own phase: a
product of sines of 2 pi j / jx and 2 pi i / iy plus a term whose wave numbers divide the period in a
periodic direction and are incommensurate with the grid in the other, so that it is periodic exactly
where the grid is.  For p*, two oracle steps stay finite at every a of PSA_AMPLITUDES_TRIED, 0.01 to 0.9,
on the five periodic cuts (the form itself ends at a = 1, where p* reaches zero); half of the largest,
a = 0.45, is used.  The TKE inputs are those of tests/test_tke_rows_cpu.py made periodic (wave numbers that
divide the period, a patch that straddles j = jx | 1), and the wind normal to the lines that exist
reverses along them.  NB's boundary values of t and qv are moved off the initial state, which they
equal as generated, so that its relaxation terms are not zero.

Rows and tolerances (the project's own, from tests/test_dyn_rows_* and tests/test_tke_rows_*).
 - XKC on every grid, PTEN on HB (iboudy 5, 1, 4), QDOT on every grid: bit for bit at every cross point,
   the columns jx, 1 and under CRM the rows iy, 1 included.
 - ATM1_TKE, ATM2_TKE after tend and after bdyval, over two steps, bit for bit at every cross point of
   the kz + 1 levels (check_tke of tests/test_tke_rows_cpu.py).
 - On HB (iboudy 5, 1, 4; idiffu 1, 2): the diffusion and the relaxation (sponge) of t, qv, qc, u, v as
   on / off differences of two oracle runs from identical state within (n + 1) * 2**-52 * (B + |term|),
   n = 5 (t, qv, qc) and 9 (u, v) as tests/test_dyn_rows_cpu.py counts them, and the totals TTEN, QVTEN,
   QCTEN, UTEN, VTEN at rtol 1e-10, atol 1e-11 * max|want| at every point of the band's interior ranges.

Not vacuous, from the restatement alone (check_statics, check_supports, check_mutants, check_term,
check_tke):
 - the statics differ at every one of the columns jx - 1, jx, 1, 2 (and the matching rows under CRM);
 - the fourth-order diffusion reaches j = 1 and j = jx, the second-order lines are non-zero on each
   side that exists and absent on the periodic sides; every term is non-zero on all of its support
   and zero off it, with median |term| / bound >= 2**20, and each TKE term moves the forecast by
   >= 2**20 ulp at the median point;
 - mutants of the restatement, judged on the two lines next to the wrap (the columns jx and 1, under
   CRM the rows iy and 1 as well) at the levels 2..kz that every term reaches (XKC: every level): (a)
   the wrap replaced by the limited-area zero pad in every neighbour read (the TKE forecast before its
   floor; QDOT, XKC and PTEN on the column jx and the row iy, the only lines whose j + 1 / i + 1 they
   read past the period; on HB the diffusion terms and the totals); (b) each of MSFX, MSFD, PSA (with
   PSB), DPSDXM rolled by one column in j, and by one row in i under CRM (QDOT, XKC and the TKE forecast,
   whichever reads the field; on HB also the totals); (c) nh_qdot with twt(k,1) and twt(k,2) exchanged,
   at the levels where the two weights differ by more than 0.05 (the 23-level table is evenly spaced
   but for four levels, and equal weights make the exchange a no-op); (d) the hydrostatic qdot used for
   the non-hydrostatic TKE.  On the bit-for-bit rows a mutant must miss by more than 2**20 ulp at every
   such value.  One cannot (WEAK_MUTANT): MSFX rolled against the TKE forecast on the CRM cuts, where
   the one term that reads MSFX changes sign along the line and one value of about 2 500 falls to
   between 2**17.7 and 2**19.6 ulp; it alone is allowed one value at or below 2**20 and none below 2**16.
   On the tolerance rows a mutant must miss by more than 1000 x the bound of a term at every value
   where the term is not zero, and by more than 1000 x the tolerance of a total on every column and at
   99 % or more of the values larger than 1e-3 of the field's maximum (check_band_totals says why);
 - on HB and NB the south and north TKE lines each hold inflow and outflow points, on CRM bdyval
   changes no TKE value, and the tkemin floor is active at between 1 % and 99 % of the interior
   points (check_tke; 12 to 13 % on every case).
"""
import dataclasses
import functools

import numpy as np
import pytest

from regcm_amd import icbc
from regcm_amd.config import CONFIGS
from tests import dyn_ref as dr
from tests import tke_ref as tr
from tests.support import case, oracle, variant_id
from tests.test_dyn_rows_cpu import N_ADD, NO_DIF, TOTALS, check_term, prepared, same_state, sponge_support
from tests.test_tke_rows_cpu import check_tke, reversing_flow, tke_inputs, two_steps

CUT = dict(jx=37, iy=29, nspgx=None, nspgd=None)
EVEN = dict(jx=34, iy=23, nspgx=7, nspgd=7)
GRIDS = {"HB-37x29": ("HB", {}), "HB-34x23": ("HB", EVEN), "NL-37x29": ("NL", {}), "NB-37x29": ("NB", CUT),
         "CRM-37x29": ("CRM", CUT), "CRM-34x23": ("CRM", dict(CUT, jx=34, iy=23))}
VARIANTS = [{}, {"idiffu": 2}, {"upstream_mode": 0}]
CASES = [(g, v) for g in GRIDS for v in VARIANTS] + [(g, {"iboudy": 4}) for g in GRIDS if g[:2] in ("HB", "NB")]
MAP_AMPLITUDE = 0.01
PSA_AMPLITUDE = 0.45
PSA_AMPLITUDES_TRIED = (0.01, 0.02, 0.04, 0.08, 0.16, 0.32, 0.64, 0.9)
DPS_AMPLITUDE = 1.0e-5
HT_AMPLITUDE = 50.0 * dr.EGRAV              # 50 m of terrain, as geopotential
ULP20 = 2.0 ** 20

grid_variant = pytest.mark.parametrize("grid,variant", CASES, ids=lambda p: p if isinstance(p, str) else variant_id(p))


# ------------------------------------------------------------------------------ the inputs
def pattern(rc, n):
    """[i, j] in [-1, 1]: sin(2 pi j / jx + a) sin(2 pi i / iy + b) + 0.5 sin(p j + q i + c), scaled by
    1 / 1.5, with phases of the n-th field.  p = 2 pi 3 / jx where j is periodic and 0.83 where it is not,
    q = 2 pi 2 / iy where i is periodic and 0.61 where it is not."""
    G = dr.geom(rc)
    j, i = np.meshgrid(np.arange(1, rc.jx + 1, dtype=np.float64), np.arange(1, rc.iy + 1, dtype=np.float64))
    p = 2.0 * np.pi * 3.0 / rc.jx if G.perj else 0.83
    q = 2.0 * np.pi * 2.0 / rc.iy if G.peri else 0.61
    a, b, c = 0.3 + 1.1 * n, 0.7 + 0.9 * n, 0.2 + 1.7 * n
    return (np.sin(2.0 * np.pi * j / rc.jx + a) * np.sin(2.0 * np.pi * i / rc.iy + b) + 0.5 * np.sin(p * j + q * i + c)) / 1.5


def non_uniform(rc, st, psa_amplitude=PSA_AMPLITUDE):
    """The state with non-uniform statics (the module docstring).  p* is changed on the grids that are
    periodic in j; the fields coupled with it, the boundary values among them, keep their decoupled
    values."""
    st = dict(st)
    for n, name in enumerate(("MSFX", "MSFD")):
        st[name] = st[name] * (1.0 + MAP_AMPLITUDE * pattern(rc, n))[None]
    if rc.idynamic == 2:
        for n, name in enumerate(("DPSDXM", "DPSDYM")):
            st[name] = st[name] + DPS_AMPLITUDE * pattern(rc, 2 + n)[None]
    if rc.diffu_hgtf == 1:                   # the generated terrain is flat over a part of the wrap columns
        st["HT"] = st["HT"] + HT_AMPLITUDE * (1.0 + pattern(rc, 9))[None]
    G = dr.geom(rc)
    if G.perj:
        old = st["PSA"][0]
        f = 1.0 + psa_amplitude * pattern(rc, 4)
        new = old * f
        with np.errstate(divide="ignore", invalid="ignore"):
            fd = np.nan_to_num(dr.psc2psd(new, G) / dr.psc2psd(old, G))
        cross = [f"{lvl}_{n}" for lvl in ("ATM1", "ATM2") for n in ("T", "QV", "QC", "PP", "W")]
        cross += [f"{b}_{t}" for b in ("XTB", "XQB", "XPPB", "XWWB", "XPSB") for t in ("B0", "BT")] + ["PSA", "PSB"]
        dot = ["ATM1_U", "ATM1_V", "ATM2_U", "ATM2_V"] + [f"{b}_{t}" for b in ("XUB", "XVB") for t in ("B0", "BT")]
        for names, fac in ((cross, f), (dot, fd)):
            for name in names:
                if name in st:
                    st[name] = st[name] * fac[None]
    return st


def periodic_tke_inputs(rc):
    """tests/test_tke_rows_cpu.py's tke_inputs with wave numbers that divide the period in a periodic
    direction, and a 4 x 4 patch on the columns jx - 1, jx, 1, 2 (under CRM a second one on the rows
    iy - 1, iy, 1, 2).  A limited area keeps tke_inputs as it is."""
    G = dr.geom(rc)
    if not G.perj:
        return tke_inputs(rc)
    kz, iy, jx = rc.kz, rc.iy, rc.jx
    sig = np.asarray(rc.sigma, dtype=np.float64)[:, None, None]
    k = np.arange(kz + 1, dtype=np.float64)[:, None, None]
    i = np.arange(1, iy + 1, dtype=np.float64)[None, :, None]
    j = np.arange(1, jx + 1, dtype=np.float64)[None, None, :]
    wj = 2.0 * np.pi / jx
    wi = 2.0 * np.pi / iy if G.peri else None
    prof = 1.5 * np.exp(-(1.0 - sig) / 0.08) + 0.05
    out = {}
    for n, name in enumerate(("ATM1_TKE", "ATM2_TKE")):
        ci = np.cos(3.0 * wi * (i - n)) if G.peri else np.cos(2.0 * np.pi * (i - n) / 7.0)
        si = 2.0 * wi * i if G.peri else 0.37 * i
        t = prof * (1.0 + 0.5 * np.sin(4.0 * wj * (j + 2.0 * n)) * ci + 0.2 * np.sin(0.9 * k + si + 5.0 * wj * j + n))
        t[:, 9:13, [jx - 2, jx - 1, 0, 1]] += 2.0
        if G.peri:
            t[:, [iy - 2, iy - 1, 0, 1], 15:19] += 2.0
        out[name] = np.maximum(t, rc.tkemin)
    ph = 2.0 * wj * j + (3.0 * wi * i if G.peri else 2.0 * np.pi * i / 11.0)
    out["TKEPHY"] = out["ATM2_TKE"] / rc.dt * 1.5 * np.sin(ph) * np.cos(np.pi * k / 5.0)
    for a in out.values():
        if not G.peri:
            a[:, iy - 1, :] = 0.0
    return out


def reversing_normal_flow(rc, st):
    """A band has the south and north lines alone, whose inflow / outflow test reads v: p*v of both time
    levels and of the boundary value is multiplied by cos(2 pi 3 j / jx + 0.35 k), so that the meridional
    wind reverses along both lines, at other columns on other levels.  A limited area takes
    tests/test_tke_rows_cpu.py's reversing zonal wind; the CRM grid has no line."""
    G = dr.geom(rc)
    if not G.perj:
        return reversing_flow(rc, st)
    if G.peri:
        return st
    j = np.arange(1, rc.jx + 1, dtype=np.float64)[None, None, :]
    k = np.arange(rc.kz, dtype=np.float64)[:, None, None]
    w = np.cos(2.0 * np.pi * 3.0 * j / rc.jx + 0.35 * k)
    out = dict(st)
    for name in ("ATM1_V", "ATM2_V", "XVB_B0", "XVB_BT"):
        out[name] = st[name] * w
    return out


@functools.lru_cache(maxsize=None)
def _start(grid, vkey, psa_amplitude):
    kind, cut = GRIDS[grid]
    variant = dict(vkey)
    if kind == "HB":
        rc, data, st = case("C", i_band=1, ibltyp=2, **cut, **variant)
        st = prepared(rc, st)
    elif kind == "NL":
        rc, data, st = case("N", ibltyp=2, **cut, **variant)
    else:
        opts = dict(i_crm=0, iboudy=5) if kind == "NB" else {}
        rc = dataclasses.replace(CONFIGS["CRM"], **cut, **dict(opts, **variant))
        data = icbc.generate_crm(rc)
        st = dict(data["state"])
        if kind == "NB":
            # the generated boundary values equal the initial state, which leaves the relaxation of t and
            # qv zero: they are moved off it by 0.1 % and 1 % of a pattern, with a small tendency
            for n, (b, amp) in enumerate((("XTB", 1.0e-3), ("XQB", 1.0e-2))):
                st[b + "_B0"] = st[b + "_B0"] * (1.0 + amp * pattern(rc, 5 + n))[None]
                st[b + "_BT"] = st[b + "_B0"] * (1.0e-6 * pattern(rc, 7 + n))[None]
    st = reversing_normal_flow(rc, non_uniform(rc, st, psa_amplitude))
    tke = periodic_tke_inputs(rc)
    st.update({n: tke[n] for n in ("ATM1_TKE", "ATM2_TKE")})
    return rc, data, st, {"TKEPHY": tke["TKEPHY"]}


def start(grid, variant, psa_amplitude=PSA_AMPLITUDE):
    """(rc, data, state, extra) of a grid and a variant; shared, not to be changed."""
    return _start(grid, tuple(sorted(variant.items())), psa_amplitude)


def more_fields(rc):
    return ("XKC", "PTEN") if rc.idynamic == 1 else ("XKC",)


def run(c, rc):
    """two_steps of the started core c with the inputs of rc's core and XKC (PTEN) after each tend."""
    return two_steps(c, names=tr.input_names(rc), more=more_fields(rc))


@functools.lru_cache(maxsize=None)
def _oracle_run(grid, vkey):
    rc, data, st, extra = start(grid, dict(vkey))
    return rc, run(oracle(rc, data, st, extra=extra), rc)


# ------------------------------------------------------------------------------ the checks both files make
def wrap_lines(rc):
    """[i, j] of the two lines next to the wrap: the columns jx and 1, and under CRM the rows iy and 1,
    within jci x ici."""
    G = dr.geom(rc)
    m = np.zeros((rc.iy, rc.jx), dtype=bool)
    if G.perj:
        m[:, [0, rc.jx - 1]] = True
    if G.peri:
        m[[0, rc.iy - 1], :] = True
    return m & G.box("i", False)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


def check_statics(rc, g):
    """The statics differ at every one of the columns jx - 1, jx, 1, 2 (rows alike under CRM)."""
    G = dr.geom(rc)
    names = ("MSFX", "MSFD", "PSA") + (("DPSDXM", "DPSDYM") if rc.idynamic == 2 else ()) + (("HT",) if rc.diffu_hgtf == 1 else ())
    rows = G.box("i", False).any(axis=1)
    for name in names if G.perj else ():
        a = g[name][0]
        cols = a[rows][:, [rc.jx - 2, rc.jx - 1, 0, 1]]
        assert (np.diff(cols, axis=1) != 0.0).all() and (cols[:, 0] != cols[:, 3]).all(), name
        if G.peri:
            r4 = a[[rc.iy - 2, rc.iy - 1, 0, 1], :]
            assert (np.diff(r4, axis=0) != 0.0).all() and (r4[0] != r4[3]).all(), name


def check_supports(tag, rc, r):
    """The supports of the diffusion increments of the TKE, from the restatement alone: idiffu = 1 has
    the fourth-order form on jcii x icii, which on a band reaches j = 1 and j = jx, and one second-order
    line per side that exists; idiffu = 2 one form on jci x ici.  Each is non-zero on all of its support
    (at some level) and zero off it."""
    G = dr.geom(rc)
    dom = G.box("i", False)
    if rc.idiffu == 2:
        sup = [dom]
    else:
        sup = [G.box("ii", False)] + [ln & dom for ln in G.lines(False)]
        assert len(sup) == 1 + sum((G.left, G.right, G.bottom, G.top))
        if G.perj:
            assert sup[0][:, 0].any() and sup[0][:, rc.jx - 1].any()
    assert len(r["dif"]) == len(sup)
    for n, (inc, m) in enumerate(zip(r["dif"], sup)):
        assert (np.abs(inc[:, m]).max(axis=0) > 0.0).all(), (tag, n, "zero on its support")
        assert not inc[:, ~m].any(), (tag, n, "non-zero off its support")


def rolled(g, name, axis):
    out = dict(g)
    for n in (name, "PSB") if name == "PSA" else (name,):
        out[n] = np.roll(g[n], 1, axis=axis)
    return out


def far_lines(rc):
    """[i, j] of the line whose j + 1 (i + 1) is past the end of the period: the column jx, and under
    CRM the row iy.  XKC, QDOT and PTEN read (j, i), (j + 1, i), (j, i + 1), (j + 1, i + 1) alone, so the
    wrap reaches them there and not on the column 1."""
    G = dr.geom(rc)
    m = np.zeros((rc.iy, rc.jx), dtype=bool)
    if G.perj:
        m[:, rc.jx - 1] = True
    if G.peri:
        m[rc.iy - 1, :] = True
    return m


# The one mutant that cannot miss at every value: MSFX enters the non-hydrostatic TKE through the
# horizontal advection alone (xmapf), which changes sign along the wrap lines, and where it passes
# through zero a 1 % map factor moves the forecast by less.  On the CRM cuts one value of about 2 500
# falls below 2**20 ulp (2**17.7 to 2**19.6).  For this (field, row, grid) alone: at most one such
# value, and none below 2**16.
WEAK_MUTANT = ("MSFX", "TKE forecast", "CRM")
WEAK_FLOOR = 2.0 ** 16


def check_mutants(tag, rc, g, dt0, r):
    """The mutants of the module docstring against the restatement r of the same inputs: each misses
    QDOT, XKC or the TKE forecast (before its floor) by more than 2**20 ulp at every point of the lines
    next to the wrap and every level 2..kz (XKC: 1..kz), but for WEAK_MUTANT."""
    G = dr.geom(rc)
    kind = "CRM" if G.peri else "band" if G.perj else "limited area"
    kz = rc.kz
    nh = rc.idynamic == 2
    lines = wrap_lines(rc)

    def tend(gg, **kw):
        return tr.tke_tend(rc, gg, g["ATM1_TKE"], g["ATM2_TKE"], g["TKEPHY"], dt0, **kw)

    def coeff(gg):
        return (dr.hydro_coeff(rc, gg) if rc.idynamic == 1 else dr.nh_coeff(rc, gg))["xkc"]

    def miss(name, row, got, want, where, levels=slice(1, kz), field=None):
        u = ulps(got[levels][:, where], want[levels][:, where])
        low = int((u <= ULP20).sum())
        print(f"{tag} mutant {name}, {row}: least miss 2**{np.log2(max(u.min(), 2.0 ** -60)):.1f} ulp over {u.size} values, "
              f"{low} at or below 2**20")
        if (field, row, kind) == WEAK_MUTANT:
            assert low <= 1 and u.min() > WEAK_FLOOR, (tag, name, row, low, float(u.min()))
        else:
            assert u.min() > ULP20, (tag, name, row, float(u.min()))

    if G.perj:
        far = far_lines(rc) & G.box("i", False)
        with dr.zero_pad_for_the_wrap():
            mu, xk = tend(g), coeff(g)
        miss("(a) zero pad for the wrap", "TKE forecast", mu["raw"], r["raw"], lines)
        miss("(a) zero pad for the wrap", "QDOT", mu["qdot"], r["qdot"], far)
        miss("(a) zero pad for the wrap", "XKC", xk, coeff(g), far, slice(0, kz))
        reads_qdot = ("MSFD", "PSA", "DPSDXM") if nh else ("MSFX", "MSFD", "PSA")
        for name in ("MSFX", "MSFD", "PSA") + (("DPSDXM",) if nh else ()):
            for axis, what in ((-1, "j"),) + (((-2, "i"),) if G.peri else ()):
                mu = tend(rolled(g, name, axis))
                miss(f"(b) {name} rolled in {what}", "TKE forecast", mu["raw"], r["raw"], lines, field=name)
                if name in reads_qdot:
                    miss(f"(b) {name} rolled in {what}", "QDOT", mu["qdot"], r["qdot"], lines, field=name)
                if name == "PSA":                                # xkc = raw * rdxsq * p*b, raw from u / p*dot
                    miss(f"(b) {name} rolled in {what}", "XKC", coeff(rolled(g, name, axis)), coeff(g), lines, slice(0, kz))
    if nh:
        every = G.box("i", False)
        where = lines if G.perj else every
        # (c) changes nothing at a level whose two weights are equal (evenly spaced sigma): it is held to
        # the levels k = 2..kz where they differ by more than 0.05 (four of the 23-level table)
        twt1, twt2 = dr.twt(rc)
        uneven = np.flatnonzero(np.abs(twt1[2:kz + 1] - twt2[2:kz + 1]) > 0.05) + 1
        assert uneven.size >= 4, uneven
        mu = tend(g, swap_twt=True)
        miss("(c) twt(k,1) and twt(k,2) exchanged", "QDOT", mu["qdot"], r["qdot"], where, uneven)
        mu = tend(g, hydro_qdot=True)
        miss("(d) the hydrostatic qdot", "QDOT", mu["qdot"], r["qdot"], where)
        miss("(d) the hydrostatic qdot", "TKE forecast", mu["raw"], r["raw"], where)


def check_rows(tag, rc, step, xkc=True):
    """XKC of one step's record against the restatement, bit for bit at every cross point (xkc = False:
    the record holds none); the statics, the supports and the mutants."""
    g, dt0, _, mid, _ = step
    G = dr.geom(rc)
    check_statics(rc, g)
    r = tr.tke_tend(rc, g, g["ATM1_TKE"], g["ATM2_TKE"], g["TKEPHY"], dt0)
    check_supports(tag, rc, r)
    check_mutants(tag, rc, g, dt0, r)
    co = dr.hydro_coeff(rc, g) if rc.idynamic == 1 else dr.nh_coeff(rc, g)
    m, e = G.box("i", False), G.box("e", False)
    assert (co["xkc"][:, m] > 0.0).all()
    if not xkc:
        return r
    bad = mid["XKC"][:, m] != co["xkc"][:, m]
    print(f"{tag} XKC: {int(bad.sum())} of {bad.size} points differ")
    assert not bad.any(), "XKC"
    # the lines off jci x ici keep the unscaled coefficient (the scaling loop runs over jci x ici)
    assert np.array_equal(mid["XKC"][:, e & ~m], co["xkc_raw"][:, e & ~m]) and not mid["XKC"][:, ~e].any()
    return r


def check_pten(tag, rc, g, times, got):
    """PTEN of the hydrostatic core with its nudge2d / sponge2d term, bit for bit on jce x ice."""
    dt0, xbc = times
    r = dr.hydro_tend(rc, g, dt0, xbc)
    band = dr.band_mask(rc)
    term = r["PTEN"] - r["pten0"]
    if rc.iboudy == 4:
        wgt = r["tab"]["wgtx"]
        band = np.zeros_like(band)
        for (j, i), ib in dr.band(rc).items():
            band[i - 1, j - 1] = wgt[ib] < 1.0
    G = dr.geom(rc)
    assert band[:, 0].any() and band[:, rc.jx - 1].any() and (band.sum(axis=1) % rc.jx == 0).all()   # whole rows
    assert (term[band] != 0.0).all() and not term[~band].any()
    e = G.box("e", False)
    bad = got[0][e] != r["PTEN"][e]
    print(f"{tag} PTEN: {int(bad.sum())} of {bad.size} points differ")
    assert G.perj and not bad.any(), "PTEN"
    # mutant (a), from the restatement alone: with the zero pad for the wrap PTEN misses by more than
    # 2**20 ulp at every point of the column jx (its j + 1 is past the period), and every diffusion
    # term by more than 1000 x its bound at every value of the columns jx and 1 where it is not zero
    with dr.zero_pad_for_the_wrap():
        mu = dr.hydro_tend(rc, g, dt0, xbc)
    far = far_lines(rc) & e
    u = ulps(mu["PTEN"][far], r["PTEN"][far])
    print(f"{tag} PTEN with the zero pad for the wrap: least miss 2**{np.log2(max(u.min(), 2.0 ** -60)):.1f} ulp")
    assert u.min() > ULP20
    for total, key, dot in TOTALS:
        m = dr.domain_mask(rc, dot) & (np.arange(rc.jx)[None, :] % (rc.jx - 1) == 0)
        want, got = dr.total(r[key.lower() + "_dif"])[:, m], dr.total(mu[key.lower() + "_dif"])[:, m]
        bound = (N_ADD[(key, "dif")] + 1) * 2.0 ** -52 * (np.fmax(r[key].big, np.abs(r[total]))[:, m] + np.abs(want))
        live = want != 0.0
        with np.errstate(divide="ignore", invalid="ignore"):     # a level the term does not touch
            ratio = (np.abs(got - want) / bound)[live]
        print(f"{tag} {total} diffusion with the zero pad for the wrap: least miss {ratio.min():.3e} x bound over {ratio.size} values")
        assert live.any(axis=0).all() and ratio.min() > 1000.0, (total, float(ratio.min()))


# ------------------------------------------------------------------------------ the grid of the text
def test_geometry_of_the_four_grids():
    """The ranges of the text on each kind of grid, and on a limited area today's masks exactly."""
    for grid in ("HB-37x29", "NL-37x29", "NB-37x29", "CRM-37x29", "HB-34x23", "CRM-34x23"):
        rc = start(grid, {})[0]
        G = dr.geom(rc)
        jx, iy = rc.jx, rc.iy
        got = (G.left, G.right, G.bottom, G.top, (G.jde1, G.jde2, G.jdi1, G.jdi2, G.jdii1, G.jdii2),
               (G.jce1, G.jce2, G.jci1, G.jci2, G.jcii1, G.jcii2), (G.ide1, G.ide2, G.idi1, G.idi2, G.idii1, G.idii2),
               (G.ice1, G.ice2, G.ici1, G.ici2, G.icii1, G.icii2))
        lim_j = ((1, jx, 2, jx - 1, 3, jx - 2), (1, jx - 1, 2, jx - 2, 3, jx - 3))
        lim_i = ((1, iy, 2, iy - 1, 3, iy - 2), (1, iy - 1, 2, iy - 2, 3, iy - 3))
        per_j, per_i = ((1, jx) * 3, (1, jx) * 3), ((1, iy) * 3, (1, iy) * 3)
        if rc.i_crm:
            assert got == (False,) * 4 + per_j + per_i
        elif rc.i_band:
            assert got == (False, False, True, True) + per_j + lim_i
        else:
            assert got == (True,) * 4 + lim_j + lim_i


@pytest.mark.parametrize("shape", [(37, 29), (34, 23)], ids=str)
def test_limited_area_masks_are_unchanged(shape):
    """With i_band = i_crm = 0 the geometry reproduces the masks the module stated by hand."""
    jx, iy = shape
    rc = dataclasses.replace(CONFIGS["C1"], jx=jx, iy=iy, nspgx=7, nspgd=7)
    for dot in (False, True):
        j2, i2 = (jx - 1, iy - 1) if dot else (jx - 2, iy - 2)
        jj, ii = np.meshgrid(np.arange(1, jx + 1), np.arange(1, iy + 1))
        dom = (jj >= 2) & (jj <= j2) & (ii >= 2) & (ii <= i2)
        inner = (jj >= 3) & (jj <= j2 - 1) & (ii >= 3) & (ii <= i2 - 1)
        assert np.array_equal(dr.domain_mask(rc, dot), dom)
        ring, corners = dr.ring_masks(rc, dot)
        assert np.array_equal(ring, dom & ~inner)
        assert np.array_equal(corners, ((jj == 2) | (jj == j2)) & ((ii == 2) | (ii == i2)))
        G = dr.geom(rc)
        assert np.array_equal(G.box("ii", dot), inner)
        assert [np.array_equal(a, b) for a, b in zip(G.lines(dot), (jj == 2, jj == j2, ii == 2, ii == i2))] == [True] * 4
        assert dr.tile_columns(rc, dot) == [(j2, 2, i2)]
        sides = dr.band_sides(rc, dot)
        assert {s for s, _ in sides.values()} == {dr.SOUTH, dr.NORTH, dr.WEST, dr.EAST}
        assert all(dom[i - 1, j - 1] for j, i in sides)
    assert np.array_equal(tr.interior(rc), dr.domain_mask(rc))


def test_band_sides_on_the_periodic_grids():
    """South and north only, at every j, with no corner rule; empty under CRM."""
    rc = start("HB-37x29", {})[0]
    for dot, nsp, ihi in ((False, rc.nspgx, rc.iy - 2), (True, rc.nspgd, rc.iy - 1)):
        s = dr.band_sides(rc, dot)
        assert len(s) == 2 * rc.jx * (nsp - 2)
        for j in (1, 2, rc.jx - 1, rc.jx):
            assert [s[(j, i)] for i in range(2, nsp)] == [(dr.SOUTH, i) for i in range(2, nsp)]
            assert [s[(j, ihi - n)] for n in range(nsp - 2)] == [(dr.NORTH, n + 2) for n in range(nsp - 2)]
    for dot in (False, True):
        assert dr.band_sides(start("CRM-37x29", {})[0], dot) == {}


def test_psc2psd_on_the_periodic_grids():
    """The wrapped j - 1 (and i - 1), and no edge line or corner on a periodic side."""
    rng = np.random.Generator(np.random.PCG64(3))
    pc = 80.0 + rng.uniform(0.0, 10.0, (29, 37))
    band, crm = dr.psc2psd(pc, dr.Geom(37, 29, True)), dr.psc2psd(pc, dr.Geom(37, 29, True, True))
    assert band[5, 0] == (pc[5, 0] + pc[4, 0] + pc[5, 36] + pc[4, 36]) * 0.25
    assert band[0, 0] == (pc[0, 0] + pc[0, 36]) * 0.5 and band[28, 36] == (pc[27, 36] + pc[27, 35]) * 0.5
    assert crm[0, 0] == (pc[0, 0] + pc[28, 0] + pc[0, 36] + pc[28, 36]) * 0.25
    assert crm[0, 7] == (pc[0, 7] + pc[28, 7] + pc[0, 6] + pc[28, 6]) * 0.25
    assert (band > 0.0).all() and (crm > 0.0).all()
    assert np.array_equal(band[1:28, 1:36], dr.psc2psd(pc)[1:28, 1:36])


def test_inputs_are_periodic_and_not_uniform():
    for grid in GRIDS:
        rc, _, st, extra = start(grid, {})
        g = dict(st)
        g.update(extra)
        check_statics(rc, g)
        G = dr.geom(rc)
        for name in ("ATM1_TKE", "ATM2_TKE"):
            a = st[name][:, :G.ice2, :G.jce2]
            assert a.min() >= rc.tkemin and all((np.diff(a, axis=ax) != 0.0).mean() > 0.9 for ax in (0, 1, 2))
            if G.perj:
                assert (a[:, 9:13, [rc.jx - 2, rc.jx - 1, 0, 1]] > 2.0).all()


@pytest.mark.parametrize("grid", [g for g in GRIDS if not g.startswith("NL")])
def test_two_steps_stay_finite_at_the_largest_psa_amplitude(grid):
    """What PSA_AMPLITUDE rests on: with p* multiplied by 1 + a * pattern at the largest a tried, two
    oracle steps stay finite on every periodic cut (the smaller a of PSA_AMPLITUDES_TRIED did as well
    when the amplitude was chosen), and PSA_AMPLITUDE is half of it."""
    a = max(PSA_AMPLITUDES_TRIED)
    assert PSA_AMPLITUDE == 0.5 * a and a < 1.0                  # at a = 1 the form brings p* to zero
    rc, data, st, extra = start(grid, {}, a)
    assert st["PSA"][0][dr.geom(rc).box("e", False)].min() > 0.0
    o = oracle(rc, data, st, extra=extra)
    o.step(2)
    names = ("ATM1_T", "ATM1_U", "ATM1_V", "ATM1_QV", "ATM1_TKE") + (("ATM1_W", "ATM1_PP") if rc.idynamic == 2 else ("PSA",))
    for name in names:
        assert np.isfinite(o.get(name)).all(), name
    o.close()


# ------------------------------------------------------------------------------ the rows
@grid_variant
def test_xkc_qdot_and_tke_bit_for_bit(grid, variant):
    rc, steps = _oracle_run(grid, tuple(sorted(variant.items())))
    tag = f"{grid} {variant_id(variant)}"
    check_rows(tag, rc, steps[0])
    for n, step in enumerate(steps):
        check_tke(f"{tag} step {n + 1}", rc, step, n == 0)


@pytest.mark.parametrize("grid,variant", [c for c in CASES if c[0].startswith("HB")] +
                         [(g, {"iboudy": 1}) for g in GRIDS if g.startswith("HB")],
                         ids=lambda p: p if isinstance(p, str) else variant_id(p))
def test_band_pten_bit_for_bit(grid, variant):
    rc, data, st, extra = start(grid, variant)
    o = oracle(rc, data, st, extra=extra)
    g = {n: o.get(n) for n in dr.HYDRO_INPUTS}
    _, dt0, xbc = o.get_time()
    o.tend()
    got = o.get("PTEN")
    o.close()
    check_pten(f"{grid} {variant_id(variant)}", rc, g, (dt0, xbc), got)


# ------------------------------------------------------------------------------ the hydrostatic band, term by term
HB_GRIDS = [g for g in GRIDS if g.startswith("HB")]
HB_VARIANTS = [{}, {"iboudy": 1}, {"iboudy": 4}, {"idiffu": 2}]
hb_cases = pytest.mark.parametrize("grid,variant", [(g, v) for g in HB_GRIDS for v in HB_VARIANTS],
                                   ids=lambda p: p if isinstance(p, str) else variant_id(p))
TEND_OUT = ("TTEN", "QVTEN", "QCTEN", "UTEN", "VTEN", "XKC", "PTEN")


def one_tend(c, rc):
    """One tend of the started hydrostatic core c: the state after bdyval, the times, what tend leaves."""
    g = {n: c.get(n) for n in dr.HYDRO_INPUTS}
    _, dt0, xbc = c.get_time()
    c.tend()
    out = {n: c.get(n) for n in TEND_OUT}
    c.close()
    return g, (dt0, xbc), out


@functools.lru_cache(maxsize=None)
def _hb_oracle_run(grid, vkey, okey):
    rc, data, st, extra = start(grid, dict(vkey))
    rcv = dataclasses.replace(rc, **dict(okey))
    return (rcv,) + one_tend(oracle(rcv, data, st, extra=extra), rcv)


def hb_oracle_run(grid, variant, **opts):
    return _hb_oracle_run(grid, tuple(sorted(variant.items())), tuple(sorted(opts.items())))


def relax_support(rc, r, dot):
    return sponge_support(rc, r["tab"], dot) if rc.iboudy == 4 else dr.band_mask(rc, dot)


def check_band_diffusion(tag, rc, r, full, nodif, fields=TOTALS):
    """The diffusion of the fields as the on / off difference of two runs' totals against the
    restatement r, on jci x ici / jdi x idi of the band: every j, the columns jx and 1 among them."""
    for name, key, dot in fields:
        dom = dr.domain_mask(rc, dot)
        ring, corners = dr.ring_masks(rc, dot)
        assert dom[:, 0].any() and dom[:, rc.jx - 1].any() and not corners.any() and ring.sum() == 2 * rc.jx
        got = full[name] - nodif[name]
        assert (np.abs(got[:, ring]).max(axis=0) > 0.0).all(), name
        check_term(f"{tag} {name} diffusion", got, r[key.lower() + "_dif"], np.fmax(r[key].big, np.abs(r[name])),
                   N_ADD[(key, "dif")], dom, dom)


def check_band_relaxation(tag, rc, r0, on, off, fields=TOTALS):
    """The relaxation (iboudy 5, 1) or the sponge (iboudy 4) of the fields as the on / off difference,
    diffusion off in both runs, against the restatement r0 made without diffusion: the south and north
    rows at every j."""
    for name, key, dot in fields:
        if key == "C":
            assert np.array_equal(on[name], off[name])           # qc is not relaxed
            continue
        dom, band = dr.domain_mask(rc, dot), relax_support(rc, r0, dot)
        assert band[:, 0].any() and band[:, rc.jx - 1].any() and (band.sum(axis=1) % rc.jx == 0).all()
        incs = [r0["sponge"][name]] if rc.iboudy == 4 else r0[key.lower() + "_bdy"]
        check_term(f"{tag} {name} relaxation", on[name] - off[name], incs, np.fmax(r0[key].big, np.abs(r0[name])),
                   N_ADD[(key, "bdy")], band, dom)


def check_band_totals(tag, rc, r, out, g, times):
    """The totals at every point of the band's interior ranges, at the tolerance of the libm rows; and,
    from the restatement alone, two mutants judged on the two lines next to the wrap.  (a) the zero pad
    for the wrap, (b) MSFX, MSFD or PSA (and PSB) rolled by one column: each misses every total that
    reads the field by more than 1000 x that tolerance on every column at the column's strongest level,
    and at SHARE or more of the values with |want| > LARGE * max|want|.  The tolerance's absolute part
    is 1e-11 max|want|, so 1000 x it hides any change below 1e-8 max|want|: at a value of 1e-3 max|want|
    the mutant has to move it by 1e-5 of itself, which a map factor of 1 % amplitude moved by one of jx
    columns (2 pi / jx of it, 1e-3) does unless the term it enters is a small part of the total there;
    below that size, on the levels where qc or the tendency is near zero, nothing can be asked.  QCTEN is
    judged on the levels of its cloud layer, where it has a horizontal term at all."""
    LARGE, SHARE = 1.0e-3, 0.99
    with dr.zero_pad_for_the_wrap():
        mutants = [("the zero pad for the wrap", [t[0] for t in TOTALS], dr.hydro_tend(rc, g, *times))]
    for field, totals in (("MSFX", ("TTEN", "QVTEN", "QCTEN")), ("MSFD", [t[0] for t in TOTALS]), ("PSA", [t[0] for t in TOTALS])):
        mutants.append((field + " rolled", totals, dr.hydro_tend(rc, rolled(g, field, -1), *times)))
    for what, totals, mu in mutants:
        for name, _, dot in TOTALS:
            if name not in totals:
                continue
            m = dr.domain_mask(rc, dot)
            lines = m & (np.arange(rc.jx)[None, :] % (rc.jx - 1) == 0)
            top = np.abs(r[name][:, m]).max()
            tol = 1e-10 * np.abs(r[name]) + 1e-11 * top
            ratio = (np.abs(mu[name] - r[name]) / tol)[:, lines]
            large = np.abs(r[name][:, lines]) > LARGE * top
            if name == "QCTEN":          # off the cloud layer (prepared: levels 4..12) qc moves by its vertical flux
                large[:3] = large[12:] = False               # alone, which reads no neighbour in j
            col = np.where(large, ratio, 0.0).max(axis=0)
            share = float((ratio[large] > 1000.0).mean())
            print(f"{tag} {name} with {what}: least miss of a column {col.min():.3e} x tolerance, "
                  f"{share:.4f} of the {int(large.sum())} large values miss by > 1000 x")
            assert large.any(axis=0).all() and col.min() > 1000.0 and share >= SHARE, (name, what, float(col.min()), share)
    for name, _, dot in TOTALS:
        m = dr.domain_mask(rc, dot)
        assert m[:, 0].any() and m[:, rc.jx - 1].any()
        got, want = out[name][:, m], r[name][:, m]
        assert np.abs(want).max() > 0.0, name
        tol = 1e-10 * np.abs(want) + 1e-11 * np.abs(want).max()
        print(f"{tag} {name}: worst |err| / tolerance = {(np.abs(got - want) / tol).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-11 * np.abs(want).max(), err_msg=name)


@hb_cases
def test_band_diffusion_terms(grid, variant):
    rc, g1, times, full = hb_oracle_run(grid, variant)
    _, g0, _, nodif = hb_oracle_run(grid, variant, **NO_DIF)
    same_state(g1, g0)
    check_band_diffusion(f"{grid} {variant_id(variant)}", rc, dr.hydro_tend(rc, g1, *times), full, nodif)


@hb_cases
def test_band_relaxation_terms(grid, variant):
    rc, g1, times, on = hb_oracle_run(grid, variant, **NO_DIF)
    _, g0, _, off = hb_oracle_run(grid, variant, iboudy=3 if rc.iboudy == 4 else 2, **NO_DIF)
    same_state(g1, g0)
    check_band_relaxation(f"{grid} {variant_id(variant)}", rc, dr.hydro_tend(rc, g1, *times, diffuse=False), on, off)


@hb_cases
def test_band_totals(grid, variant):
    rc, g, times, out = hb_oracle_run(grid, variant)
    check_band_totals(f"{grid} {variant_id(variant)}", rc, dr.hydro_tend(rc, g, *times), out, g, times)
