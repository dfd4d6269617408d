"""The covering list of the chirp-z and generic FFT classes (tests/conv_cover.py) on the CPU functional emulator (tests/emu) -- the twin of
tests/test_gpu_conv_classes.py: the emulator runs the same kernel bodies and the same set-up, so a wrong table, pad, factor walk or
`k2 <= nmen` branch shows here without a GPU.

Three parts.  The coverage conditions of the frozen list.  Set-ups only, both precisions: every listed length selects the recorded
class and factor list ("fftplan", "fftwork", "fftfac"), and the same-parity neighbour outside every recorded first and last length
selects another class.  And the limited-area transforms of the listed fp64 lengths up to EMU_MAX points, NDGL = 4, KMSMAX = (n - 1) // 2 --
every bin of the row live in both directions --, rows whole and, on the last length of every class, rows cut by NPROMA = n - 1, against the NumPy model of tests/lam_ref.py at
the emulator tier's 1e-12.  Observed 1.4e-16 ... 1.8e-15 over the 125 lengths.  A 2050-point row takes 16 - 34 s here, so the longer lengths,
the fp32 library, white input, the adjoints, the truncation edges and the sphere run on the GPU only.  The module takes 3.2 minutes on
8 cores (one OS thread per lane: 3 s for a 1280-point row; with the cut rows on every length, 250 cases for 216, it took 6.4 minutes)."""
import os
import subprocess

import numpy as np
import pytest

from tests import conv_cover
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
def test_list_meets_the_coverage_conditions(precision):
    """first and last length of every class, the classes behind the switches, the mixed-radix rows forced onto the convolution, every
    radix in every pass position of the run-time factor lists, five odd half lengths -- and the conditions bite: a list without its
    rows of one switch, or without one class end, misses something"""
    cover = conv_cover.COVER[precision]
    assert conv_cover.missing(cover, precision) == []
    assert sorted(cover) == cover and len(set(e[:2] for e in cover)) == len(cover)
    for sw in conv_cover.SWITCHES:
        assert conv_cover.missing([e for e in cover if e[1] != sw], precision), sw
    for key, (first, last) in conv_cover.CLASSES[precision].items():
        assert conv_cover.missing([e for e in cover if e[:2] != (last, "")], precision), key
    even, odd = (sum(k[0] == par for k in conv_cover.CLASSES[precision]) for par in (0, 1))
    assert (even, odd) == {8: (65, 80), 4: (46 + 1, 80)}[precision]  # (+ 1: the class of GM_FP32, beyond the enumerated range)


def sphere_classes(et, precision, ns, sw, monkeypatch):
    """sphere handles with NSMAX = 1 and up to 60 of the lengths `ns` each, set up under the switches `sw`: yields (handle, lengths)"""
    with monkeypatch.context() as m:
        for k, v in conv_cover.SWITCHES[sw].items():
            m.setenv(k, v)
        for i in range(0, len(ns), 60):
            part = ns[i:i + 60]
            r = et.setup_trans(1, 2 * len(part), np.array(part + part[::-1], dtype=np.int32), precision=precision)
            try:
                yield r, part
            finally:
                et.trans_release(r)


@pytest.mark.parametrize("precision", [8, 4])
def test_listed_lengths_select_the_recorded_classes(et, precision, monkeypatch):
    for sw in conv_cover.SWITCHES:
        ns = [e[0] for e in conv_cover.entries(precision, sw=sw)]
        for r, part in sphere_classes(et, precision, ns, sw, monkeypatch):
            assert et.trans_inq(r, "fftfac").shape == (2 * len(part), 15)
            for j, n in enumerate(part):
                conv_cover.assert_class(et, r, n, precision, sw, rows=(j, 2 * len(part) - 1 - j), inq=et.trans_inq)


@pytest.mark.parametrize("precision", [8, 4])
def test_first_and_last_lengths_are_the_ends_of_their_classes(et, precision, monkeypatch):
    """the length of the same parity below every recorded first and above every recorded last length selects another class (or the
    direct mixed-radix family); not above GM_FP32, whose class goes on and whose neighbours cost seconds of set-up each"""
    want = {}
    for key, (first, last) in conv_cover.CLASSES[precision].items():
        for n in (first - 2, last + 2):
            if n >= 3 and not (precision == 4 and key[1] == conv_cover.GM_FAMILY):
                want.setdefault(n, []).append(key)
    ns = sorted(want)
    for r, part in sphere_classes(et, precision, ns, "", monkeypatch):
        plan, work = et.trans_inq(r, "fftplan"), et.trans_inq(r, "fftwork")
        for j, n in enumerate(part):
            got = (n % 2, int(plan[j][0]), int(work[j]), int(plan[j][4]))
            assert got not in want[n], "row length %d selects the class %s: its neighbour is not the end of that class -- choose the covering list again (tests/conv_cover.py)" % (n, got)


EMU = [(e, "whole") for e in conv_cover.entries(8, EMU_MAX)] + [(e, "cut") for e in conv_cover.last_entries(8) if e[0] <= EMU_MAX]


@pytest.mark.parametrize("entry,nproma", EMU, ids=[conv_cover.ident(e) + "-" + w for e, w in EMU])
def test_limited_area_rows_fp64(et, entry, nproma, monkeypatch):
    """every length whole; the last length of every class also cut by NPROMA = n - 1 (the cut adds the grid-side copy of a row that crosses
    blocks, which is code of the class and not of the length)"""
    n, sw, cls = entry
    for k, v in conv_cover.SWITCHES[sw].items():
        monkeypatch.setenv(k, v)
    ndgl, M, N = 4, (n - 1) // 2, 1
    r = et.esetup_trans(M, N, ndgl, kdlon=n, pexwn=units(n, ndgl)[0], peywn=units(n, ndgl)[1], precision=8)
    try:
        conv_cover.assert_class(et, r, n, 8, sw)
        nuv, nsc = (1, 1) if cls[2] == 1 else (2, 3)  # one field per workgroup: more fields only repeat the same work
        errs, _ = lam_case(et, n, ndgl, M, N, nuv=nuv, nsc=nsc, nproma=None if nproma == "whole" else n - 1, kresol=r)
    finally:
        et.trans_release(r)
    print("conv class", n, sw, cls, nproma, "%.1e" % max(errs.values()))
    assert max(errs.values()) < TOL, errs
