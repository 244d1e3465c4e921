"""CPU checks of SUBEX on the device (rcmdyn_set_subex, rcmdyn_put_subex, rcmdyn_get_subex,
rcmdyn_physics_subex; regcm_amd/csrc/subex.hpp).

The oracle stubs the microphysics, so the yardstick is tests/subex_ref.py, a NumPy transcription of
cldfrac with subex_cldfrac and of subex.  The host-compiled header (tests/subex/subex_point.cpp) is
held to it bit for bit over a table that populates every branch; its two transcendental pieces
(10**x of qcth and the exp of the chis table) are handed to the transcription and held to NumPy's
own within the ulp bound tests/test_fastmath_cpu.py holds powpos to.  The inputs of the GPU tests
(tests/test_subex_gpu.py) are checked here too, from the transcription alone."""
import ctypes
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from regcm_amd import dycore, icbc
from regcm_amd.config import CONFIGS
from tests import condtq_ref as cq
from tests import subex_host as sh
from tests import subex_ref as sx
from tests.support import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rcmdyn.h")
FDIR = os.path.join(ROOT, "regcm_amd", "fortran")
CALLS = ["rcmdyn_set_subex", "rcmdyn_put_subex", "rcmdyn_get_subex", "rcmdyn_physics_subex"]
POW_ULP = 1.5          # tests/test_fastmath_cpu.py: epow < 1.5


def test_subex_calls_declared_exported_and_bound():
    src = open(HEADER).read()
    L = dycore.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", dycore.LIB_PATH], capture_output=True, text=True).stdout
    for n in CALLS:
        assert re.search(rf"^int {n}\(rcmdyn_t\* h", src, re.M), n
        assert n in dycore.EXPORTED
        assert re.search(rf"\bT {n}$", nm, re.M), n
    i32, dp, P, dbl = ctypes.c_int32, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_double
    assert L.rcmdyn_set_subex.argtypes == [P, i32, dbl, dbl, dbl] + [i32] * 6
    assert L.rcmdyn_put_subex.argtypes == [P, i32, dp] + [i32] * 6
    assert L.rcmdyn_get_subex.argtypes == [P, i32, dp] + [i32] * 6
    assert L.rcmdyn_physics_subex.argtypes == [P]
    for m in ("set_subex", "put_subex", "get_subex", "physics_subex"):
        assert callable(getattr(dycore.DynCore, m)), m
    # no ABI bump, and one order of the fields in the header, the Python host and the Fortran module
    assert re.search(r"#define RCMDYN_ABI_VERSION 6\b", src)
    body = src.split("enum rcmdyn_subex_field", 1)[1].split("}", 1)[0]
    assert re.findall(r"RCMDYN_SUBEX_(\w+)", body) == dycore.SUBEX_FIELDS
    assert re.search(r"RCMDYN_NSUBEX\b", body) and len(dycore.SUBEX_FIELDS) == 19
    f90 = open(os.path.join(FDIR, "mod_gpu_dyn.F90")).read()
    ids = {m.group(1).upper(): int(m.group(2)) for m in re.finditer(r"\bsubex_(\w+)\s*=\s*(\d+)", f90.lower())}
    assert ids == {n: q for q, n in enumerate(dycore.SUBEX_FIELDS)}
    assert re.search(r"rcmdyn_nsubex\s*=\s*19\b", f90)
    for n in CALLS:
        assert re.search(rf"bind\(c, name='{n}'\)", f90), n
        assert re.search(rf"public ::.*\b{n}\b", f90), n
    eng = open(os.path.join(ROOT, "regcm_amd", "csrc", "engine.hip")).read()
    names = re.search(r"SBX_NAME\[RCMDYN_NSUBEX\] = \{(.*?)\};", eng, re.S).group(1)
    assert re.findall(r'"(\w+)"', names) == dycore.SUBEX_FIELDS


def ulps(a, b):
    """|a - b| in units of the spacing of b."""
    return np.abs(a - b) / np.spacing(np.abs(b))


def test_header_power_and_chis_table_against_numpy():
    """The header's 10**x (rcm_pow10) over the exponents of qcth for 150 .. 330 K, and its chis table
    (rcm_exp), against NumPy's: within the bound test_fastmath_cpu.py holds powpos to."""
    t = np.concatenate([np.linspace(150.0, 330.0, 400001), np.random.Generator(np.random.PCG64(1)).uniform(150.0, 330.0, 400000)])
    x = sx.qcth_arg(t)
    e = ulps(sh.pow10(x), sx.pow10(x))
    print("10**x: max ulp", e.max(), "share of equal bits", float((e == 0).mean()))
    assert e.max() < POW_ULP
    c = ulps(sh.chis(), sx.chis_table())
    print("chis: max ulp", c.max())
    assert c.max() < POW_ULP
    assert sh.chis().shape == (sx.NCHI,)


def table(par, kz=14, ncol=9000, seed=3):
    """Columns (k, 1, col) of inputs for cldfrac and subex: realistic values, and blocks of columns
    that force each gate, clamp and branch."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shp = (kz, 1, ncol)
    q = ncol // 18
    blk = lambda n: (slice(None), slice(None), slice(n * q, (n + 1) * q))
    psb = rng.uniform(60.0, 101.0, (1, ncol))
    sig = np.linspace(0.0, 1.0, kz + 1) ** 1.3
    pf = (sig[:, None, None] * psb[None] + 5.0) * 1000.0
    p = 0.5 * (pf[1:] + pf[:-1])
    t = 205.0 + 95.0 * (p / 1.0e5) ** 0.6 + rng.uniform(-12.0, 12.0, shp)      # both sides of tc0, tcel < -50 aloft
    qs = cq.pfwsat(t, p)
    rh = rng.uniform(0.3, 1.02, shp)
    rh[blk(0)] = rng.uniform(0.0, 0.02, rh[blk(0)].shape)                      # under rhmin
    rh[blk(1)] = rng.uniform(1.0, 1.05, rh[blk(1)].shape)                      # rhrng > 0.99999, over rhmax
    qv = rh * qs
    qc = 2.0e-4 * rng.uniform(0.05, 1.0, shp) * (rng.uniform(0.0, 1.0, shp) < 0.6)
    qc[blk(2)] = rng.choice([0.0, 5.0e-11, 1.0e-10, 5.0e-9, 1.0e-7, 2.0e-7], qc[blk(2)].shape)   # the three qc gates
    rh0 = rng.choice([0.8, 0.9], (1, ncol))
    rh0[:, 3 * q:4 * q] = 0.9999                                               # rhrng <= rh0adj for most
    # every ichi bin: a target fcc f through Sundqvist's root on the warm side
    b = blk(4)
    f = rng.uniform(0.0, 1.0, t[b].shape)
    f[0, 0, :256] = (np.arange(256) + 0.5) / 255.0 * (np.arange(256) < 255) + 0.00015 * (np.arange(256) == 255)
    t[b] = rng.uniform(245.0, 300.0, t[b].shape)
    rh[b] = 1.0 - (1.0 - f) * (1.0 - f) * (1.0 - rh0[:, b[2]][None])
    qc[b] = 1.0e-4
    qv[b] = rh[b] * cq.pfwsat(t[b], p[b])
    # the arctic factor at both clamps: low levels, qv under 0.15 * 0.003, and qv = 0.003 exactly
    qv[kz - 3:, :, 5 * q:5 * q + q // 2] = rng.uniform(1.0e-5, 4.0e-4, qv[kz - 3:, :, 5 * q:5 * q + q // 2].shape)
    qv[kz - 3:, :, 5 * q + q // 2:6 * q] = 0.003
    rho = p / (cq.RGAS * t)
    cufra = np.zeros(shp)
    culwc = np.zeros(shp)
    cufra[blk(6)] = rng.uniform(0.0, 0.8, cufra[blk(6)].shape)                 # the merge, cumulus above lowcld
    culwc[blk(6)] = 0.3
    cufra[blk(7)] = rng.uniform(0.0, 1.0e-4, cufra[blk(7)].shape)              # at most lowcld
    culwc[blk(7)] = 0.3
    tab = dict(RH0=rh0, QCK1=np.full((1, ncol), 0.0005), CGUL=rng.choice([0.65, 0.30], (1, ncol)),
               CEVAP=np.full((1, ncol), 1.0e-5), CACCR=rng.choice([6.0, 4.0], (1, ncol)))
    tab["QCK1"][:, 8 * q:9 * q] = 0.05                                         # pptmax before accretion
    tab["CACCR"][:, 9 * q:10 * q] = 5.0e4                                      # pptmax after accretion
    tab["CEVAP"][:, 10 * q:11 * q] = 1.0e-2                                    # rdevap limited by pptkm1 or dqv
    tab["CEVAP"][:, 11 * q:12 * q] = 1.0e-7                                    # by neither
    # rain from a cloud aloft through clear air below: dry (evaporates), saturated (dqv <= 0), and
    # rh at rhmax in unsaturated air (rdevap = 0: the dlowval gate)
    for n, (lo, hi) in ((12, (0.05, 0.5)), (13, (1.0, 1.04)), (14, (par.rhmax, par.rhmax))):
        b = blk(n)
        qc[b] = 0.0
        qc[2:5, :, b[2]] = 3.0e-4
        rh[2:5, :, b[2]] = 0.99
        rh[5:, :, b[2]] = rng.uniform(lo, hi, rh[5:, :, b[2]].shape)
        qv[b] = np.minimum(rh[b], 1.04 if n == 13 else 0.7) * qs[b]
    tab["CEVAP"][:, 12 * q:12 * q + q // 2] = 1.0e-2
    f = dict(t=t, p=p, pf=pf, qv=qv, qc=qc, rh=rh, rho=rho, psb=psb)
    return f, tab, (cufra, culwc)


def bits_equal(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = a.view(np.int64) == b.view(np.int64)
    assert same.all(), (what, int((~same).sum()), a[~same][:3], b[~same][:3])


@pytest.mark.parametrize("iconvlwp,arctic,rem", [(1, True, True), (0, False, False)], ids=["clwfromt-arctic-rem", "incloud"])
def test_header_equals_the_fortran_text_bit_for_bit(iconvlwp, arctic, rem):
    par = sx.params(larcticcorr=arctic, iconvlwp=iconvlwp)
    f, tab, cu = table(par)
    dt, dtsec = 150.0, 75.0
    chis = sh.chis()
    rng = np.random.Generator(np.random.PCG64(9))
    acc = {n: rng.uniform(0.0, 3.0, f["psb"].shape) for n in ("RAINNC", "LSMRNC", "TRRATE")}
    c, s = sx.run(f, tab, par, dt, dtsec, chis, pow10=sh.pow10, cu=cu, acc=acc, rem=rem)
    m = s["masks"]
    count = {
        "qc <= 1e-10": (f["qc"] <= 1.0e-10).sum(), "1e-10 < qc <= 1e-7": ((f["qc"] > 1.0e-10) & (f["qc"] <= 1.0e-7)).sum(),
        "qc > 1e-7": c["gate"].sum(), "t > tc0": c["warm"].sum(), "t <= tc0": c["cold"].sum(),
        "rhrng <= rh0adj": c["none"].sum(), "rhrng > 0.99999": c["full"].sum(), "Sundqvist": c["sund"].sum(),
        "rh < rhmin": (c["gate"] & (f["rh"] < par.rhmin)).sum(), "rh > rhmax": (c["gate"] & (f["rh"] > par.rhmax)).sum(),
        "hicld clamp": c["hi_clamp"].sum(), "fcc > lowcld": c["cloudy"].sum(), "fcc <= lowcld": (~c["cloudy"]).sum(),
        "tcel < -50": (c["cloudy"] & (f["t"] - sx.TZERO < -50.0)).sum(),
        "cumulus > lowcld": c["conv"].sum(), "0 < cumulus <= lowcld": (~c["conv"] & (cu[0] > 0)).sum(),
        "cldlwc = 0": (~c["wet"]).sum(), "rh0adj = 0": (c["rh0adj"] == 0.0).sum(), "rh0adj = 0.99999": (c["rh0adj"] == 0.99999).sum(),
        "cloud gate": m["cloud"].sum(), "dqc = 0 in cloud": (m["cloud"] & (s["dqc"] == 0.0)).sum(), "dqc > 0": (s["dqc"] > 0).sum(),
        "pptmax before accretion": m["pptmax_auto"].sum(), "pptmax after accretion": m["pptmax_acc"].sum(),
        "top level rains": m["rains"][0].sum(), "level rains": m["rains"][1:].sum(),
        "no rain from above": m["noppt"][1:].sum(), "dqv <= 0": m["dqv_neg"].sum(),
        "rdevap by dqv": m["lim_dqv"].sum(), "rdevap by pptkm1": m["lim_km1"].sum(), "rdevap by neither": m["lim_none"].sum(),
        "rdevap <= dlowval": m["evap_gate"].sum(), "pptsum floor": m["floor"].sum(),
        "prainx > dlowval": s["surface"].sum(), "prainx <= dlowval": s["dry_surface"].sum(), "all rain lost": s["lost_all"].sum(),
    }
    if arctic:
        count.update({"arctic": c["arctic"].sum(), "arctic 0.15 clamp": c["arctic_lo"].sum(), "arctic 1.0 clamp": c["arctic_hi"].sum(),
                      "arctic between": (c["arctic"] & ~c["arctic_lo"] & ~c["arctic_hi"]).sum()})
    for what, n in count.items():
        print(f"{what}: {int(n)}")
    for what, n in count.items():
        assert n >= 20, (what, int(n))
    bins = np.unique(c["ichi"][c["cloudy"]])
    assert np.array_equal(bins, np.arange(255)), (bins.size, np.setdiff1d(np.arange(255), bins))
    # a bin's two edges: fcc * 255 just under and at a whole number
    frac = (c["fcc"] * 255.0)[c["cloudy"]]
    assert (frac - np.floor(frac) < 0.01).sum() >= 20 and (frac - np.floor(frac) > 0.99).sum() >= 20
    # the header
    full = lambda a: np.broadcast_to(a[None], f["t"].shape)
    h = sh.point(par, chis, f["t"], f["p"], f["qv"], f["qc"], f["rh"], f["rho"], full(tab["RH0"]), full(tab["CGUL"]), *cu)
    for key in ("fcc", "cldfra", "cldlwc", "rh0adj", "dqc"):
        bits_equal(h[key], c[key] if key in c else s[key], key)
    bits_equal(h["qcth"][m["cloud"]], s["qcth"][m["cloud"]], "qcth")
    hc = sh.columns(par, dt, dtsec, rem, h["fcc"], h["dqc"], f["t"], f["p"], f["pf"], f["qv"], f["qc"], f["rh"], f["rho"],
                    f["psb"], tab["QCK1"], tab["CEVAP"], tab["CACCR"], acc["RAINNC"], acc["LSMRNC"], acc["TRRATE"])
    for key in ("lsc_t", "lsc_qv", "lsc_qc", "rainnc", "lsmrnc", "trrate", "pptsum") + (("remrat", "rembc") if rem else ()):
        bits_equal(hc[key], s[key], key)
    if rem:
        assert (s["rembc"] > 0).sum() >= 20 and (s["remrat"] > 0).sum() >= 20


def gpu_cases():
    """The GPU tests' inputs: the 37 x 29 cuts of C1 and N1 and the odd 34 x 23 grid, rainy."""
    out = []
    for name in ("C", "N"):
        rc, data, st0 = case(name, **({"ifrayd": 0} if name == "N" else {}))
        out.append((name, rc, sx.rainy_state(rc, st0)))
    rc = dataclasses.replace(CONFIGS["C1"], jx=34, iy=23, nspgx=None, nspgd=None)
    out.append(("odd", rc, sx.rainy_state(rc, icbc.generate(rc)["state"])))
    return out


@pytest.mark.parametrize("iconvlwp", [1, 0])
def test_gpu_inputs_populate_the_branches_from_the_transcription_alone(iconvlwp):
    """With the options the GPU tests run (larcticcorr on, either iconvlwp), on every grid."""
    for name, rc, st in gpu_cases():
        f = sx.host_slice(rc, st)
        par = sx.params(rhmax=rc.rhmax, rhmin=rc.rhmin, larcticcorr=True, iconvlwp=iconvlwp)
        c, s = sx.run(f, sx.tables(rc), par, rc.dt, rc.dt, sx.chis_table(), cu=sx.cucloud(rc), rem=True)
        I = cq.interior(rc)
        I2 = I[1:]
        m = s["masks"]
        count = {
            "qc <= 1e-10": (f["qc"][I] <= 1.0e-10).sum(), "1e-10 < qc <= 1e-7": ((f["qc"][I] > 1.0e-10) & (f["qc"][I] <= 1.0e-7)).sum(),
            "qc > 1e-7": c["gate"][I].sum(), "t > tc0": c["warm"][I].sum(), "t <= tc0": c["cold"][I].sum(),
            "rhrng <= rh0adj": c["none"][I].sum(), "rhrng > 0.99999": c["full"][I].sum(), "Sundqvist": c["sund"][I].sum(),
            "cumulus > lowcld": c["conv"][I].sum(), "cumulus <= lowcld": (~c["conv"])[I].sum(),
            "0 < cumulus <= lowcld": (~c["conv"] & (sx.cucloud(rc)[0] > 0))[I].sum(),
            "0 < rh0adj < 0.99999": ((c["rh0adj"] > 0) & (c["rh0adj"] < 0.99999))[I].sum(),
            "dqc > 0": (s["dqc"][I] > 0).sum(), "level rains": m["rains"][I].sum(),
            "pptmax before accretion": m["pptmax_auto"][I].sum(), "pptmax after accretion": m["pptmax_acc"][I].sum(),
            "arctic with fcc > 0": (c["arctic"] & (c["fcc"] > 0))[I].sum(),
            "arctic 0.15 clamp, fcc > 0": (c["arctic_lo"] & (c["fcc"] > 0))[I].sum(),
            "arctic 1.0 clamp, fcc > 0": (c["arctic_hi"] & (c["fcc"] > 0))[I].sum(),
            "arctic between, fcc > 0": (c["arctic"] & ~c["arctic_lo"] & ~c["arctic_hi"] & (c["fcc"] > 0))[I].sum(),
            "fcc > lowcld with cloud water": (c["cloudy"] & (c["totc"] > 0) & (c["cldlwc"] > 0))[I].sum(),
            "rdevap <= dlowval": m["evap_gate"][I].sum(),
            "evaporation": m["evap"][I].sum(), "rdevap by dqv": m["lim_dqv"][I].sum(), "rdevap by pptkm1": m["lim_km1"][I].sum(),
            "rdevap by neither": m["lim_none"][I].sum(), "pptsum floor": m["floor"][I].sum(),
            "prainx > dlowval": s["surface"][I2].sum(), "prainx <= dlowval": s["dry_surface"][I2].sum(),
            "all rain lost": s["lost_all"][I2].sum(), "remrat > 0": (s["remrat"][I] > 0).sum(), "rembc > 0": (s["rembc"][I] > 0).sum(),
        }
        for what, n in count.items():
            print(f"{name} {what}: {int(n)}")
        for what, n in count.items():
            assert n > 0, (name, what)
        assert s["surface"][I2].sum() >= 1 and s["lost_all"][I2].sum() >= 1
        for key in ("lsc_t", "lsc_qv", "lsc_qc", "rainnc"):
            assert np.all(np.isfinite(s[key][I if s[key].ndim == 3 else I2])), key
