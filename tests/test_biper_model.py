"""The NumPy model of the biperiodicisation routines (tests/biper_ref.py) equals every golden of tests/golden/biper byte for byte, in
both precisions: the goldens are the output of the reference's CPU routines (tests/golden/biper/README.txt), so the model is the
reference's arithmetic, and the emulator and GPU tiers may use it for cases beyond the goldens.  Two deliberately wrong models show
that the comparison can fail."""
import numpy as np
import pytest

from tests import biper_ref as R
from tests.biper_common import BOYD, DT, ET_CASES, FP_CASES, HORIZ, KSTART, TAG, boyd_name, et_name, fp_name, golden, same, ulps


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("zon", [1, 0])
@pytest.mark.parametrize("case", FP_CASES, ids=lambda c: "%dx%d_%dx%d" % c[:4])
def test_model_fpbipere_is_the_golden(case, zon, esz):
    X, Y, UX, UY, nf = case
    gin, gout = golden(fp_name(case, zon, esz) + "_in"), golden(fp_name(case, zon, esz) + "_out")
    assert gin.dtype == DT[esz] and gin.shape == (nf, X * Y + 5)
    assert same(R.fpbipere(gin, UX, UY, X, Y, zon), gout)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("case", ET_CASES, ids=lambda c: "%dx%d_%dx%d" % c[:4])
def test_model_etibihie_is_the_golden(case, esz):
    X, Y, UX, UY, nf, bix, biy = case
    gin, gout = golden(et_name(case, esz) + "_in"), golden(et_name(case, esz) + "_out")
    assert gin.shape == (Y, nf, X + 4)
    assert same(R.etibihie(gin, X, Y, UX, UY, KSTART, bix, biy), gout)


@pytest.mark.parametrize("esz", [8, 4])
def test_model_boyd_is_the_golden(esz):
    """the field with the golden weights: equal bytes; the model's own weights: within 2 ulp of the golden ones (erf)"""
    X, Y, UX, UY, nf, bw, pl = BOYD
    nm = boyd_name(esz)
    bx, by = golden(nm + "_bx"), golden(nm + "_by")
    assert same(R.boyd(golden(nm + "_in"), X, Y, bx, by), golden(nm + "_out"))
    for g in (bx, by):
        assert ulps(R.boyd_window(g.size, pl, DT[esz]), g) <= 2


@pytest.mark.parametrize("esz", [8, 4])
def test_model_horiz_field_is_the_golden(esz):
    for kx, ky in HORIZ:
        assert same(R.horiz_field(kx, ky, DT[esz]), golden("horiz_field_%dx%d_%s" % (kx, ky, TAG[esz])))


@pytest.mark.parametrize("esz", [8, 4])
def test_wrong_models_differ_from_the_golden(esz):
    """the y pass with the y direction's own lambda (the reference uses the x direction's), and one smoothing pass fewer"""
    case = FP_CASES[0]
    X, Y, UX, UY, nf = case
    gin, gout = golden(fp_name(case, 1, esz) + "_in"), golden(fp_name(case, 1, esz) + "_out")
    fixed = R.fpbipere(gin, UX, UY, X, Y, 1, lam_of_y=True)
    fewer = R.fpbipere(gin, UX, UY, X, Y, 1, fewer=1)
    assert not same(fixed, gout) and not same(fewer, gout)
    d, g = (fixed - gout)[:, :X * Y], gout[:, :X * Y]  # (behind X * Y the arrays hold a sentinel)
    assert np.abs(d).max() > 1e-4 * np.abs(g).max()
