"""Every chirp-z and generic FFT class of the covering list (tests/conv_cover.py) at full bandwidth on the GPU.

The specialised in-place kernels k_fft_*_hot, the register-resident k_fft_*_r16, the split k_fft_*_r16p, the generic k_fft_inv / k_fft_dir
(Bluestein and run-time factor lists, even rows and the odd-row complex path) and the global-scratch k_fft_*_gm carry most rows of every
real grid.  The other modules name the first and the last row length of their work-length classes but run them at NSMAX = 15 -- of a row
of thousands of bins only k <= 15 and their mirrors -- or with cubic truncation.  Here every listed length, with the class (family, work
length, fields per workgroup) and the factor list it is recorded to select, runs with EVERY bin of the row live:

* limited-area handles, NDGL = 12, KSMAX = 5, KMSMAX = (n - 1) // 2, device arrays, against the NumPy model of tests/lam_ref.py (pocketfft
  in double): band-limited input in both directions with winds, scalars and all four flags (lam_case) and full-bandwidth direct input
  (lam_white_case) on whole rows for every length of the list; rows cut by an odd NPROMA, and both adjoints element by element against
  tests/lam_ad_ref.py, on the longest row of every kernel (conv_cover.thinned_entries: every class of the families 1, 2, 3, and per
  parity, list kind and fields per workgroup of the generic passes), the two groups in alternate precisions; one length per family with
  KMSMAX on both sides of the `k2 <= nmen` switch of FOURIER_IN, which is also the join of the two half-length convolutions of the split
  kernels;
* three sphere grids of 16 latitudes with linear truncation on every row (NMEN = (n - 1) // 2) against the CPU oracle, the family of
  every row asserted: INV_TRANS + DIR_TRANS with all derivative flags, white DIR_TRANS, the adjoint identity, once more through the
  exchange-order tables (EMI_TEST_PATHS=1).

Bounds: those of tests/test_lam_gpu.py, tests/lam_ad_common.py and tests/test_gpu_parity.py -- 1e-11 of each field's maximum in fp64, 3e-5
in fp32 (and really computed in float: above 1e-9); white fp32 input also within 3 x the float32 CPU yardstick (floored at 4 epsilons);
the adjoint identity on the sphere 1e-12 / 2e-4.

Observed on an MI355X, the largest error of a case over the cases of a group (584 tests; the module takes 115 s, three times the 38 s of
tests/test_gpu_mr_plans.py.  With the cut rows and the adjoints in both precisions on the last length of every class, 810 tests, it took
145 s; they were thinned to conv_cover.thinned_entries in alternate precisions, the whole rows were not).
Limited-area, fp64: whole rows band-limited 3.5e-16 ... 2.6e-15, white 2.7e-16 ... 1.4e-15 (mean wind at most 2.8e-17); cut rows 6.7e-16 ... 2.2e-15
and 6.0e-16 ... 1.1e-15; adjoints 7.7e-16 ... 2.5e-15; the truncation edges 9.7e-16 ... 2.5e-15 band-limited, 7.3e-16 ... 1.1e-15 white.
Limited-area, fp32: whole rows band-limited 1.2e-7 ... 6.8e-7, white 1.0e-7 ... 3.3e-7 (mean wind at most 1.2e-8), on the first white scalar the
library 6.7e-8 ... 3.2e-7, the yardstick 5.5e-8 ... 3.4e-7 (at most 0.67 x the floored yardstick); cut rows 3.1e-7 ... 6.8e-7 and 1.5e-7 ... 3.1e-7
(0.51 x); adjoints 4.4e-7 ... 9.0e-7; the truncation edges 3.0e-7 ... 6.0e-7 band-limited, 2.0e-7 ... 3.3e-7 white (0.60 x).
Sphere (short8 / short2 / long; EMI_TEST_PATHS=1 gives the same bits), fp64: inverse 1.4e-15 / 2.0e-15 / 5.2e-15, direct 4.7e-16 / 5.8e-16 /
5.0e-16, white 1.2e-15 / 1.9e-15 / 1.5e-15 per field and 2.2e-15 / 2.7e-15 / 2.6e-15 per total wavenumber, adjoint identities at most 5.8e-18;
fp32: inverse 6.6e-7 / 6.7e-7 / 1.1e-6, direct 9.5e-8 / 1.8e-7 / 2.3e-7, white 3.5e-7 / 4.5e-7 / 2.8e-7 per field, on the first scalar the library
1.7e-7 / 1.9e-7 / 2.6e-7 per field and 4.2e-7 / 4.0e-7 / 4.6e-7 per total wavenumber, the yardstick 1.4e-7 / 2.0e-7 / 2.2e-7 and 2.6e-7 / 3.6e-7 /
4.6e-7, adjoint identities at most 2.2e-9."""
import numpy as np
import pytest

from tests import conv_cover, plan_rows
from tests.common import adjoint_case, run_case
from tests.lam_ad_common import ALL, lam_ad_case
from tests.plan_rows import KSMAX, NDGL, cut
from tests.test_gpu_white_direct import check as sphere_white_check
from tests.test_lam_gpu import TOL, mover

pytestmark = pytest.mark.gpu
LISTED = [(e, p) for p in (8, 4) for e in conv_cover.entries(p)]
# conv_cover.thinned_entries, in alternate precisions: a row of the two lists gets its cut rows in one precision and its adjoints in the
# other, its neighbour the other way round (the times: module docstring)
ROWS = sorted({e[:2] for p in (8, 4) for e in conv_cover.thinned_entries(p)})
CUT = [(e, p) for p in (8, 4) for e in conv_cover.thinned_entries(p) if ROWS.index(e[:2]) % 2 == (p == 4)]
ADJOINT = [(e, p) for p in (8, 4) for e in conv_cover.thinned_entries(p) if ROWS.index(e[:2]) % 2 != (p == 4)]
ids = lambda cases: [conv_cover.ident(e, p) for e, p in cases]


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=4, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


def switch(entry, monkeypatch):
    """the switches of the entry, read by the set-up that follows; returns the plan assertion of the entry"""
    for k, v in conv_cover.SWITCHES[entry[1]].items():
        monkeypatch.setenv(k, v)
    return lambda et, r, n, precision: conv_cover.assert_class(et, r, n, precision, entry[1])


def forward(et, entry, precision, nproma, what, monkeypatch, kmsmax=None):
    plan_rows.forward(et, entry[0], precision, nproma, switch(entry, monkeypatch), "conv class %s %s %s" % (what, conv_cover.ident(entry), entry[2]), kmsmax)


def test_list_meets_the_coverage_conditions_and_selects_the_recorded_classes(et, monkeypatch):
    """on the GPU library as on the emulator (tests/test_emu_conv_classes.py): the frozen list meets the coverage conditions, and every
    length of it selects the recorded class and factor list -- sphere handles with NSMAX = 1 and up to 60 row lengths each"""
    for precision in (8, 4):
        assert conv_cover.missing(conv_cover.COVER[precision], precision) == []
        for sw in conv_cover.SWITCHES:
            ns = [e[0] for e in conv_cover.entries(precision, sw=sw)]
            with monkeypatch.context() as m:
                for k, v in conv_cover.SWITCHES[sw].items():
                    m.setenv(k, v)
                for i in range(0, len(ns), 60):
                    part = ns[i:i + 60]
                    r = et.setup_trans(1, 2 * len(part), np.array(part + part[::-1], dtype=np.int32), precision=precision)
                    try:
                        for j, n in enumerate(part):
                            conv_cover.assert_class(et, r, n, precision, sw, rows=(j, 2 * len(part) - 1 - j), inq=et.trans_inq)
                    finally:
                        et.trans_release(r)


@pytest.mark.parametrize("entry,precision", LISTED, ids=ids(LISTED))
def test_whole_rows(et, entry, precision, monkeypatch):
    """Rows inside one NPROMA block."""
    forward(et, entry, precision, None, "whole", monkeypatch)


@pytest.mark.parametrize("entry,precision", CUT, ids=ids(CUT))
def test_cut_rows(et, entry, precision, monkeypatch):
    """Rows cut by NPROMA = 4093 (n - 1 for the shorter rows): rows cross blocks, fields start on odd elements."""
    forward(et, entry, precision, cut(entry[0]), "cut", monkeypatch)


@pytest.mark.parametrize("entry,precision", ADJOINT, ids=ids(ADJOINT))
def test_adjoints(et, entry, precision, monkeypatch):
    """EINV_TRANSAD / EDIR_TRANSAD, all flags, rows whole: the `adj` scalings at every bin."""
    to, back = mover("device", precision)
    with plan_rows.Handle(et, entry[0], precision, switch(entry, monkeypatch)) as h:
        errs = lam_ad_case(et, entry[0], NDGL, h.M, KSMAX, flags=ALL, precision=precision, to_dev=to, to_host=lambda t: t.cpu().numpy(), kresol=h.r)
    print("conv class adjoints", conv_cover.ident(entry), entry[2], "fp%d" % (8 * precision), "%.1e" % max(errs.values()))
    assert max(errs.values()) < TOL[precision], errs
    if precision == 4:
        assert max(errs.values()) > 1e-9  # really computed in float


# per precision one length of: generic Bluestein even, generic odd, k_fft_*_hot with several fields per workgroup, k_fft_*_hot with one,
# k_fft_*_r16, k_fft_*_r16p (sz / 2 is the join of its two convolutions), k_fft_*_gm
EDGE_KINDS = ((0, 0, "several"), (1, 0, "any"), (0, 1, "several"), (0, 1, "one"), (0, 2, "one"), (0, 3, "one"), (0, 5, "one"))
EDGE_LENGTHS = {8: [188, 1281, 1278, 5118, 3070, 5116, 10486], 4: [188, 1281, 1278, 5118, 3070, 5116, 20484]}
EDGE_KMSMAX = {"sz/2-1": lambda sz: sz // 2 - 1, "sz/2": lambda sz: sz // 2, "sz/2+1": lambda sz: sz // 2 + 1, "sz-2": lambda sz: sz - 2}
EDGES = [(n, p, e) for p in (8, 4) for n in EDGE_LENGTHS[p] for e in EDGE_KMSMAX]


def default_entry(n, precision):
    return [e for e in conv_cover.entries(precision, sw="") if e[0] == n][0]


@pytest.mark.parametrize("n,precision,edge", EDGES, ids=["%d-fp%d-%s" % (n, 8 * p, e) for n, p, e in EDGES])
def test_truncation_edges(et, n, precision, edge, monkeypatch):
    """KMSMAX on both sides of the `k2 <= nmen` switch of FOURIER_IN (sz = n // 2: the mirror sz - k of a bin k > 0 is live from
    KMSMAX = sz / 2 on), and a last bin that is not the neighbour of the row's Nyquist bin: the zero-fill above NMEN; band-limited and
    white input.  The odd row too takes sz = n // 2 here, not the n points of its complex transform: KMSMAX cannot exceed (n - 1) // 2, and
    its mirror switch `n - k <= nmen` fills the upper half of the work array from bin n - KMSMAX on, so the four values leave a quarter
    of the array, or two points of it, zero between the two live ends."""
    forward(et, default_entry(n, precision), precision, None, "edge " + edge, monkeypatch, kmsmax=EDGE_KMSMAX[edge](n // 2))


def test_edge_lengths_are_what_they_are_chosen_for():
    for p in (8, 4):
        for n, (parity, family, fields) in zip(EDGE_LENGTHS[p], EDGE_KINDS):
            fam, work, fbk = default_entry(n, p)[2]
            assert (n % 2, fam) == (parity, family) and work != conv_cover.half(n) and {"several": fbk > 1, "one": fbk == 1, "any": True}[fields], (n, p)


# ---- the sphere: 16 latitudes, linear truncation on every row ------------------------------------------------------------------------
# (rows from the pole to the equator, wind pairs, scalars).  The rows in ascending order, as on any reduced Gaussian grid (see
# tests/test_gpu_mr_plans.py).  Every row is a length of the list with default switches, so its family is on record.
SPHERE = {"short8": ([62, 94, 124, 188, 254, 318, 382, 508], 2, 3),       # generic Bluestein rows; hot with 8 and 4 fields per workgroup
          "short2": ([118, 158, 574, 638, 766, 958, 1022, 1278], 2, 3),   # ... hot with 4 and 2 fields per workgroup: every such class is in one of the two
          "long": ([2562, 3070, 3074, 4094, 4098, 4100, 5116, 5124], 1, 2)}  # r16 S = 3072, 4096; hot 4608; r16p 2560, 3072: NSMAX = 2561


def test_short_grids_hold_every_hot_class_with_several_fields():
    for p in (8, 4):
        want = {k[1:] for k in conv_cover.CLASSES[p] if k[1] == 1 and k[3] > 1}
        rows = SPHERE["short8"][0] + SPHERE["short2"][0]
        assert want <= {default_entry(n, p)[2] for n in rows} and {2, 4, 8} <= {c[2] for c in want}
        assert sum(default_entry(n, p)[2][0] == 0 for n in rows) >= 6


def Oracle(*a, **k):
    from oracle.oracle import Oracle as O
    return O(*a, **k)


@pytest.fixture(scope="module")
def dev():
    import torch
    return (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")), (lambda t: t.cpu().numpy())


@pytest.mark.parametrize("paths", [0, 1])
@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("grid", sorted(SPHERE))
def test_sphere_linear_truncation(et, dev, grid, precision, paths, monkeypatch):
    """NSMAX = the largest (n - 1) // 2 of the grid: every row keeps all of its bins, NMEN differs from row to row.  INV_TRANS + DIR_TRANS
    with winds, scalars and all derivative flags, DIR_TRANS of white fields, the adjoint identity; paths = 1: once more through the
    exchange-order tables (EMI_TEST_PATHS=1)."""
    if paths:
        monkeypatch.setenv("EMI_TEST_PATHS", str(paths))
    rows, nuv, nsc = SPHERE[grid]
    nloen = np.array(rows + rows[::-1], dtype=np.int32)
    nsmax = max((n - 1) // 2 for n in rows)
    r = et.setup_trans(nsmax, len(nloen), nloen, precision=precision)
    try:
        assert list(et.trans_inq(r, "nmen")) == [min(nsmax, (n - 1) // 2) for n in nloen]
        for j, n in enumerate(rows):
            conv_cover.assert_class(et, r, n, precision, rows=(j, len(nloen) - 1 - j), inq=et.trans_inq)
    finally:
        et.trans_release(r)
    e_inv, e_dir = run_case(et, Oracle, dev, nsmax, nloen, nuv, nsc, dict(scders=True, uvder=True, vorgp=True, divgp=True), None, precision=precision)
    print("sphere", grid, "fp%d" % (8 * precision), "paths", paths, "inverse %.1e direct %.1e" % (e_inv, e_dir))
    assert e_inv < TOL[precision] and e_dir < TOL[precision], (e_inv, e_dir)
    sphere_white_check(et, dev, nsmax, nloen, nuv, nsc, None, precision, "sphere %s paths %d" % (grid, paths))
    a_inv, a_dir = adjoint_case(et, dev, nsmax, nloen, nuv, nsc, precision=precision)
    print("sphere", grid, "fp%d" % (8 * precision), "paths", paths, "adjoint identities %.1e %.1e" % (a_inv, a_dir))
    tol = 1e-12 if precision == 8 else 2e-4
    assert a_inv < tol and a_dir < tol, (a_inv, a_dir)
