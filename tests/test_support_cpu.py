"""tests/support.py on synthetic arrays: the cross-grid crop for a limited area, a band and the
cloud-resolving configuration, the error norm with and without it, the CROSS set and the state
names.  No engine and no oracle library."""
import dataclasses

import numpy as np
import pytest

from regcm_amd.config import CONFIGS, NH_STATE_FIELDS, QX_STATE_FIELDS, STATE_FIELDS, TKE_STATE_FIELDS
from tests.support import CROSS, NH_FIELDS, crop, rel_l2, relerr, state_names

LAM = CONFIGS["C1"]
BAND = dataclasses.replace(LAM, i_band=1)
CRM = CONFIGS["CRM"]


def field(rc, nk=3, seed=1):
    return np.random.default_rng(seed).uniform(1.0, 2.0, size=(nk, rc.iy, rc.jx))


def test_cross_is_the_union_of_the_files_sets():
    assert CROSS == {"ATM1_T", "ATM1_QV", "ATM1_QC", "ATM2_T", "ATM2_QV", "ATM2_QC", "PSA", "PSB", "DSTOR",
                     "HSTOR", "PSC", "PTEN", "TTEN", "QVTEN", "QCTEN", "OMEGA", "QDOT", "XKC", "PHI",
                     "ATM1_PP", "ATM2_PP", "ATM1_W", "ATM2_W", "ATM1_TKE", "ATM2_TKE",
                     "ATM1_QI", "ATM1_QR", "ATM1_QS", "ATM2_QI", "ATM2_QR", "ATM2_QS"}
    assert set(QX_STATE_FIELDS) <= CROSS and len(CROSS) == 31


@pytest.mark.parametrize("rc,rows,cols", [(LAM, LAM.iy - 1, LAM.jx - 1), (BAND, BAND.iy - 1, BAND.jx),
                                          (CRM, CRM.iy, CRM.jx)], ids=["lam", "band", "crm"])
def test_crop_shapes(rc, rows, cols):
    a = field(rc)
    for name in ("ATM1_T", "HSTOR", "ATM2_TKE", "ATM1_QS"):
        c = crop(a, rc, name)
        assert c.shape == (3, rows, cols)
        assert np.array_equal(c, a[:, :rows, :cols])
    assert crop(a[0], rc, "PSA").shape == (rows, cols)            # a 2-D field
    for name in ("ATM1_U", "ATMS_TB3D", "UTEN"):
        assert crop(a, rc, name) is a


@pytest.mark.parametrize("rc", [LAM, BAND], ids=["lam", "band"])
def test_last_row_and_column_are_outside_the_default_comparison(rc):
    b = field(rc)
    spots = [(1, rc.iy - 1, 5)] + ([(2, 7, rc.jx - 1)] if not rc.i_band else [])
    for spot in spots:
        a = b.copy()
        a[spot] += 0.5
        for norm in (relerr, rel_l2):
            assert norm(a, b, rc, "ATM1_T") == 0.0
            assert norm(a, b, rc, "ATM1_T", crop=False) > 0.0
            assert norm(a, b, rc, "ATM1_U") > 0.0                 # not a cross field: never cropped
    if rc.i_band:                                                 # a band's last column is compared
        a = b.copy()
        a[2, 7, rc.jx - 1] += 0.5
        assert relerr(a, b, rc, "ATM1_T") > 0.0


def test_crm_compares_every_point():
    b = field(CRM)
    for spot in ((0, CRM.iy - 1, 3), (1, 4, CRM.jx - 1)):
        a = b.copy()
        a[spot] += 0.5
        assert relerr(a, b, CRM, "ATM1_T") == relerr(a, b, CRM, "ATM1_T", crop=False) > 0.0


@pytest.mark.parametrize("rc", [LAM, BAND, CRM], ids=["lam", "band", "crm"])
def test_interior_difference_is_the_written_out_formula(rc):
    b = field(rc)
    b[0, 3, 3] = 5.0                     # the largest value lies inside every extent
    a = b.copy()
    a[1, 9, 11] += 0.25
    # the formula as the test files wrote it: the limited-area crop, max |a - b| / max |b|
    ac, bc = a[:, : rc.iy - 1, : rc.jx - 1], b[:, : rc.iy - 1, : rc.jx - 1]
    old = float(np.max(np.abs(ac - bc)) / max(np.max(np.abs(bc)), 1e-300))
    old_l2 = float(np.sqrt(np.sum((ac - bc) ** 2))) / max(float(np.sqrt(np.sum(bc * bc))), 1e-300)
    whole = float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
    assert relerr(a, b, rc, "ATM1_T", crop=False) == whole
    assert relerr(a, b, rc, "ATM1_U") == whole
    assert relerr(a, b, rc, "ATM1_T") == whole == 0.25 / 5.0     # the same value both ways
    if rc is LAM:
        assert relerr(a, b, rc, "ATM1_T") == old > 0.0
        assert rel_l2(a, b, rc, "ATM1_T") == old_l2 > 0.0
    assert relerr(b, b, rc, "ATM1_T") == 0.0
    z = np.zeros_like(b)
    assert relerr(z, z, rc, "ATM1_T") == 0.0                      # the 1e-300 floor of the denominator


def test_state_names():
    c1, n1 = CONFIGS["C1"], CONFIGS["N1"]
    assert state_names(c1) == STATE_FIELDS
    assert NH_FIELDS == [n for n in STATE_FIELDS if n not in ("DSTOR", "HSTOR")] + NH_STATE_FIELDS
    assert state_names(n1) == NH_FIELDS
    assert state_names(dataclasses.replace(c1, ipptls=2)) == STATE_FIELDS + QX_STATE_FIELDS
    assert state_names(dataclasses.replace(n1, ipptls=2)) == NH_FIELDS + QX_STATE_FIELDS
    tke = dataclasses.replace(c1, ibltyp=2)
    assert state_names(tke) == STATE_FIELDS                       # the TKE only on request
    assert state_names(tke, tke=True) == STATE_FIELDS + TKE_STATE_FIELDS
    assert state_names(c1, tke=True) == STATE_FIELDS
    both = dataclasses.replace(n1, ipptls=2, ibltyp=2)
    assert state_names(both, tke=True) == NH_FIELDS + QX_STATE_FIELDS + TKE_STATE_FIELDS
    assert state_names(c1) is not STATE_FIELDS and state_names(n1) is not NH_FIELDS    # fresh lists
