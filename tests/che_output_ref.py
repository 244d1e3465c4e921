"""The yardstick of the CHE output-stream tests: a NumPy transcription of the lines of
fill_chem_outvars that form the tracer fields the dyn core owns (Main/chemlib/mod_che_output.F90:
74-83, 131-184, the idynamic /= 3 branch) and of the burden's column sum (Main/chemlib/
mod_che_tend.F90:561-571), written from the Fortran text, vectorised over (j, i) with an explicit
k loop.  A plain module (nothing collected).

NumPy's elementwise + - * / are the IEEE operations, one rounding each, in the order written, so
every field rounds as the Fortran text does.  Arrays are [k - 1, i - 1, j - 1] over the whole grid,
as DynCore.get returns them; the results are zero outside jci1:jci2 x ici1:ici2 of the whole domain.
"""
import numpy as np

from tests.output_ref import interior

TERMS = ("ADVH", "ADVV", "BDY", "DIFH", "CONV")
D_ZERO = 0.0


def _over_cpsb(rc, a, cpsb):
    """a(jci1:jci2,ici1:ici2,k) / cpsb(jci1:jci2,ici1:ici2) for k = 1 .. kz (:75-78, 132-135)."""
    is_, js = interior(rc)
    out = np.zeros_like(a)
    for k in range(rc.kz):
        out[k, is_, js] = a[k, is_, js] / cpsb[0, is_, js]
    return out


def mixrat(rc, chia, cpsb):
    """che_mixrat_out (:74-79): chia / cpsb, a division; cpsb is sfs%psb
    (Main/mod_che_interface.F90:128)."""
    return _over_cpsb(rc, chia, cpsb)


def term(rc, cdiag, cpsb):
    """che_advhten_out .. che_bdyten_out (:131-158, 178-184): the accumulator / cpsb."""
    return _over_cpsb(rc, cdiag, cpsb)


def nh_dzq(zf):
    """atms%dzq of the NH core: atm0%dzf (Main/mod_atm_interface.F90:977), which is
    atm0%zf(k) - atm0%zf(k+1) (Main/mod_params.F90:2636)."""
    return zf[:-1] - zf[1:]


def burden(rc, chib3d, cdzq, crhob3d):
    """che_burden_out (:81-83): dtrace * 1.0e6, with dtrace from zero over k = 1 .. kz in that order,
    dtrace = dtrace + chib3d * cdzq * crhob3d (Main/chemlib/mod_che_tend.F90:561-571)."""
    is_, js = interior(rc)
    dtrace = np.zeros((rc.iy, rc.jx))
    dtrace[:, :] = D_ZERO
    for k in range(rc.kz):
        dtrace[is_, js] = dtrace[is_, js] + chib3d[k, is_, js] * cdzq[k, is_, js] * crhob3d[k, is_, js]
    out = np.zeros((1, rc.iy, rc.jx))
    out[0, is_, js] = dtrace[is_, js] * 1.0e6
    return out
