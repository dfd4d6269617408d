"""The covering list of the direct mixed-radix FFT plans (tests/mr_cover.py) on the CPU functional emulator (tests/emu) -- the twin of
tests/test_gpu_mr_plans.py: the emulator runs the same kernel bodies, so a wrong stride, pad or digit reversal shows here without a GPU.

Two parts.  The plan assertions for the whole list, both precisions (set-ups only): every listed length selects the recorded plan
("fftplan" inquiry) and the list covers what tests/mr_cover.py requires of it.  And the limited-area transforms of the listed fp64
lengths up to EMU_MAX points, NDGL = 4, KMSMAX = (n - 1) // 2 -- every bin of the row live in both directions --, rows whole and rows
cut by an odd NPROMA, against the NumPy model of tests/lam_ref.py at the emulator tier's 1e-12.  Observed 3.5e-16 ... 1.2e-15.  The
longer lengths of the list (fp64: 1350 points and up), the fp32 library, white input, the adjoints, the truncation edges and the sphere run
on the GPU only.  The module takes 23 s."""
import os
import subprocess

import numpy as np
import pytest

from tests import mr_cover
from tests.lam_common import lam_case, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12    # fp64, of each field's maximum (the emulator tier's bound, tests/test_emu_parity.py)
EMU_MAX = 1300


@pytest.fixture(scope="module")
def et():
    os.environ.setdefault("OMP_NUM_THREADS", "256")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    import ectrans_amd
    ectrans_amd._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
    ectrans_amd.setup_trans0(kmax_resol=4)
    yield ectrans_amd
    ectrans_amd.trans_end()
    ectrans_amd._L = None


@pytest.mark.parametrize("precision", [8, 4])
def test_list_covers_the_plan_space(precision):
    """every (radix, pass) pair, pass count, pad, fields-per-workgroup value, five odd half lengths and the longest rows -- and no
    length to spare: without any one of them something is uncovered, so a length cannot leave the list unnoticed"""
    cover = mr_cover.COVER[precision]
    assert mr_cover.missing(cover, precision) == []
    for i, (n, _) in enumerate(cover):
        assert mr_cover.missing(cover[:i] + cover[i + 1:], precision), "length %d covers nothing of its own" % n


@pytest.mark.parametrize("precision", [8, 4])
def test_listed_lengths_select_the_recorded_plans(et, precision):
    """limited-area handles (every row has the same plan) ..."""
    for n in mr_cover.lengths(precision):
        r = et.esetup_trans((n - 1) // 2, 1, 4, kdlon=n, pexwn=1.0, peywn=1.0, precision=precision)
        try:
            plan = et.etrans_inq(r, "fftplan")
            assert plan.shape == (4, 5)
            mr_cover.assert_plan(plan, n, precision)
        finally:
            et.trans_release(r)


# rows of the other kernel families (tests/test_lam_gpu.py, LONG_X, and tests/test_gpu_parity.py name the kernels): (family, fields per workgroup)
OTHER_FAMILIES = {19: (0, 16), 1601: (0, 1),  # odd rows: the generic complex path
                  1284: (1, 1), 4102: (1, 1),  # k_fft_*_hot
                  4092: (2, 1),                # k_fft_*_r16<16>
                  4100: (3, 1),                # k_fft_*_r16p<10>
                  20484: (5, 1)}               # k_fft_*_gm: the work array of 24576 complex numbers exceeds the LDS in both precisions


@pytest.mark.parametrize("precision", [8, 4])
def test_sphere_handles_report_the_same_plans(et, precision):
    """... and one sphere handle with all listed lengths as its rows: "fftplan" per latitude, the work lengths of "fftwork" beside it; rows
    of the other families report their family, no factors, and their fields per workgroup"""
    ns = mr_cover.lengths(precision) + sorted(OTHER_FAMILIES)
    nloen = np.array(ns + ns[::-1], dtype=np.int32)
    r = et.setup_trans(1, len(nloen), nloen, precision=precision)
    try:
        plan, work = et.trans_inq(r, "fftplan"), et.trans_inq(r, "fftwork")
        assert plan.shape == (len(nloen), 5) and plan.dtype == np.int32
        for j, n in enumerate(ns):
            if n in OTHER_FAMILIES:
                fam, fbk = OTHER_FAMILIES[n]
                assert plan[j].tolist() == plan[len(nloen) - 1 - j].tolist() == [fam, 0, 0, 0, fbk], (n, plan[j])
            else:
                mr_cover.assert_plan(plan[[j, len(nloen) - 1 - j]], n, precision)
                assert work[j] == n // 2
    finally:
        et.trans_release(r)


def cut(n):
    """an odd NPROMA smaller than the row: rows cross blocks, fields start on odd elements"""
    return 4093 if n > 4093 else n - 1


@pytest.mark.parametrize("nproma", ["whole", "cut"])
@pytest.mark.parametrize("n", mr_cover.lengths(8, EMU_MAX))
def test_limited_area_rows_fp64(et, n, nproma):
    ndgl, M, N = 4, (n - 1) // 2, 1
    r = et.esetup_trans(M, N, ndgl, kdlon=n, pexwn=units(n, ndgl)[0], peywn=units(n, ndgl)[1], precision=8)
    try:
        mr_cover.assert_plan(et.etrans_inq(r, "fftplan"), n, 8)
        errs, _ = lam_case(et, n, ndgl, M, N, nproma=None if nproma == "whole" else cut(n), kresol=r)
    finally:
        et.trans_release(r)
    print("mr plan", n, mr_cover.plan_of(8, n), nproma, "%.1e" % max(errs.values()))
    assert max(errs.values()) < TOL, errs
