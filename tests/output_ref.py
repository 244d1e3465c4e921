"""The yardstick of the output-stream tests: a NumPy transcription of the lines of mod_output that
form the dyn-owned fields of the ATM, SRF and SHF streams (Main/mod_output.F90:226-452, 576,
933-941, 1057-1150) and of the two lines of tend that leave atm1%pr behind (Main/mod_tendency.F90:
1038, 1057 with rpsa of :825, 839), written from the Fortran text, vectorised over (j, i) with
explicit k loops.  A plain module (nothing collected).

NumPy's elementwise + - * / are the IEEE operations, one rounding each, in the order written, so
every field without a log rounds as the Fortran text does; pfwsat is tests/condtq_ref.py's
transcription of Share/pfwsat.inc.  Arrays are [k - 1, i - 1, j - 1] over the whole grid, as
DynCore.get returns them; the results are zero outside jci1:jci2 x ici1:ici2 of the whole domain.
"""
import numpy as np

from regcm_amd import constants as C
from tests.condtq_ref import pfwsat

ROVG = C.rgas / C.egrav            # Share/mod_constants.F90:187
D_RFOUR, D_HALF, D_ONE, D_10, D_100, D_1000 = 0.25, 0.5, 1.0, 10.0, 100.0, 1000.0
TWO_D = ("PS", "PS_PA", "UA100", "VA100")


def interior(rc):
    """(i slice, j slice) of jci1:jci2 x ici1:ici2 over the whole domain: 2 .. n - 2, every point
    of a periodic direction (Main/mpplib/mod_mppparam.F90:1131-1132, 1340-1360)."""
    js = slice(0, rc.jx) if rc.i_band else slice(1, rc.jx - 2)
    is_ = slice(0, rc.iy) if rc.i_crm else slice(1, rc.iy - 2)
    return is_, js


def _crop(rc, a):
    """A field cut to the interior, as the Fortran sections a(jci1:jci2,ici1:ici2,:)."""
    is_, js = interior(rc)
    return a[..., is_, js]


def _xsum(rc, u):
    """u(j,i,k) + u(j+1,i,k) + u(j,i+1,k) + u(j+1,i+1,k) on the interior, in that order; the j + 1
    (i + 1) of a periodic direction's last point is the first one (the exchanged ghost line)."""
    uj = np.roll(u, -1, axis=2)
    ui = np.roll(u, -1, axis=1)
    uji = np.roll(uj, -1, axis=1)
    return _crop(rc, u) + _crop(rc, uj) + _crop(rc, ui) + _crop(rc, uji)


def atm1_pr(rc, sigma, pre):
    """atm1%pr as the tend that starts from `pre` leaves it (whole grid): the hydrostatic
    (hsigma(k) * psa + ptop) * 1000, the NH atm0%pr + atm1%pp * rpsa with rpsa = 1 / psa.
    pre: PSA (and NH ATM1_PP, ATM0_PR) fetched before the step."""
    psa = pre["PSA"][0]
    kz = rc.kz
    pr = np.zeros((kz,) + psa.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(1, kz + 1):
            if rc.idynamic == 2:
                rpsa = D_ONE / psa
                pr[k - 1] = pre["ATM0_PR"][k - 1] + pre["ATM1_PP"][k - 1] * rpsa
            else:
                hsigma = (sigma[k] + sigma[k - 1]) * D_HALF          # Main/mod_params.F90:2008
                pr[k - 1] = (hsigma * psa + rc.ptop) * D_1000
    return pr


def output_ref(rc, sigma, st, names, left=None):
    """The fields `names` (OUTPUT_FIELDS names) from the current state st.  left: the leftovers of
    the last tend, for RH (PR: atm1_pr of the pre-step state), PF (ATMS_PF3D), ZF and ZH (ATMS_ZQ),
    OMEGA (the diagnostics export).  Returns {name: (kz | 1, iy, jx) array}.  UA100 / VA100 also
    leave the level search's facts under "_Z100": (the interface heights [kz, ni, nj] with nan above
    the level found, the branch mask 'lowest layer above 100 m')."""
    kz, ptop, nh = rc.kz, rc.ptop, rc.idynamic == 2
    is_, js = interior(rc)
    sig = lambda k: sigma[k - 1]                       # sigma(k), k = 1 .. kz + 1
    ps = _crop(rc, st["PSA"][0])                       # ps_out = sfs%psa(jci1:jci2,ici1:ici2), :226
    cut = lambda name, k: _crop(rc, st[name][k - 1])
    res = {}

    def lev3(fn):
        a = np.zeros((kz,) + ps.shape)
        for k in range(1, kz + 1):
            a[k - 1] = fn(k)
        return a

    def xwind(name, k):                                # :255-258
        return D_RFOUR * _xsum(rc, st[name][k - 1:k])[0] / ps

    for name in names:
        if name == "PS":
            v = ps.copy()
        elif name == "PS_PA":                          # :933-941
            v = (_crop(rc, st["ATM0_PS"][0]) + ptop * D_1000 + cut("ATM1_PP", kz) / ps) if nh else D_1000 * (ps + ptop)
        elif name == "T":
            v = lev3(lambda k: cut("ATM1_T", k) / ps)                                   # :234
        elif name in ("U", "V"):
            v = lev3(lambda k: xwind("ATM1_" + name, k))
        elif name == "W":
            v = lev3(lambda k: D_HALF * (cut("ATM1_W", k + 1) + cut("ATM1_W", k)) / ps)     # :277
        elif name == "PP":
            v = lev3(lambda k: cut("ATM1_PP", k) / ps)                                  # :291
        elif name == "QV":                                                              # :301, 305
            q = lev3(lambda k: cut("ATM1_QV", k) / ps)
            v = q / (D_ONE + q)
        elif name in ("QC", "QI", "QR", "QS"):                                          # :314, 336, 325, 347
            v = lev3(lambda k: cut("ATM1_" + name, k) / ps)
        elif name == "TKE":
            v = lev3(lambda k: cut("ATM1_TKE", k))                                      # :576
        elif name == "PH":
            if nh:                                                                      # :409-414
                v = lev3(lambda k: np.full(ps.shape, ptop * D_1000) if k == 1 else
                         cut("ATM0_PF", k) + D_HALF * (cut("ATM1_PP", k - 1) + cut("ATM1_PP", k)) / ps)
            else:
                v = lev3(lambda k: (sig(k) * ps + ptop) * D_1000)                       # :388
        elif name == "ZH":                                                              # :396-403
            cell = ptop / ps
            zq = left["ATMS_ZQ"]

            def zh(k):
                lay = ROVG * cut("ATM1_T", k) / ps * np.log((sig(k + 1) + cell) / (sig(k) + cell))
                return lay if k == kz else _crop(rc, zq[k]) + lay                       # zq(k + 1)
            v = lev3(zh)
        elif name == "RH":                                                              # :366-368
            v = lev3(lambda k: D_100 * np.minimum(rc.rhmax, np.maximum(
                rc.rhmin, (cut("ATM1_QV", k) / ps) / pfwsat(cut("ATM1_T", k) / ps, _crop(rc, left["PR"][k - 1])))))
        elif name == "PF":
            v = lev3(lambda k: _crop(rc, left["ATMS_PF3D"][k - 1]))                     # :378
        elif name == "ZF":
            v = lev3(lambda k: _crop(rc, left["ATMS_ZQ"][k - 1]))                       # :452
        elif name == "OMEGA":
            v = lev3(lambda k: _crop(rc, left["OMEGA"][k - 1]) * D_10)                  # :268
        elif name in ("UA100", "VA100"):
            v, z, low = wind100(rc, sigma, st, "ATM1_" + name[0])
            res["_Z100"] = (z, low)
        else:
            raise KeyError(name)
        full = np.zeros((1 if name in TWO_D else kz, rc.iy, rc.jx))
        full[:, is_, js] = v
        res[name] = full
    return res


def wind100(rc, sigma, st, wind):
    """:1057-1150 for one wind: (the 100 m value, the heights visited [kz, ni, nj] (nan where the
    search had ended), the mask of the first branch: lowest half level above 100 m)."""
    kz, ptop, nh = rc.kz, rc.ptop, rc.idynamic == 2
    sig = lambda k: sigma[k - 1]
    ps = _crop(rc, st["PSA"][0])
    cut = lambda name, k: _crop(rc, st[name][k - 1])
    xw = lambda k: D_RFOUR * _xsum(rc, st[wind][k - 1:k])[0] / ps
    cell = ptop / ps

    def layer(k):
        tv = cut("ATM1_T", k) / ps * (D_ONE + C.ep1 * cut("ATM1_QV", k) / ps)
        return ROVG * tv * np.log((sig(k + 1) + cell) / (sig(k) + cell))

    zz = cut("ATM0_Z", kz) if nh else layer(kz)
    heights = np.full((kz,) + ps.shape, np.nan)
    heights[kz - 1] = zz
    low = zz > 100.0
    out = np.where(low, xw(kz), 0.0)
    done = low.copy()
    for k in range(kz - 1, 0, -1):
        zz1 = cut("ATM0_Z", k) if nh else zz + layer(k)
        heights[k - 1] = np.where(done, np.nan, zz1)
        hit = ~done & (zz1 > 100.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ww = (100.0 - zz) / (zz1 - zz)
            val = ww * xw(k) + (D_ONE - ww) * xw(k + 1)
        out = np.where(hit, val, out)
        done |= hit
        zz = np.where(done, zz, zz1)
    return out, heights, low
