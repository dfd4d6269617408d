"""Every direct mixed-radix FFT plan of the covering list (tests/mr_cover.py) at full bandwidth on the GPU.

k_fft_dir_mr / k_fft_inv_mr (csrc/emi_mr_body.h) are generic code over a plan (A, B, C) that a cost model picks.  The other modules run
them at NSMAX = 15 -- of a row of thousands of bins only the coefficients k <= 15 and their mirrors -- or on octahedral rows with cubic
truncation.  Here every listed length, with the plan it is recorded to select, runs with EVERY bin of the row live:

* limited-area handles, NDGL = 12, KSMAX = 5, KMSMAX = (n - 1) // 2, device arrays, against the NumPy model of tests/lam_ref.py
  (pocketfft in double): band-limited input in both directions with winds, scalars and all four flags (lam_case), full-bandwidth
  direct input (lam_white_case), rows whole and rows cut by an odd NPROMA; both adjoints element by element against
  tests/lam_ad_ref.py; six lengths per precision with KMSMAX on both sides of the `k2 <= nmen` switch of FOURIER_IN;
* two sphere grids of 16 latitudes with linear truncation on every row (NMEN = (n - 1) // 2: per-row NMEN and Fourier offsets, the
  Gaussian weights, the exchange-order tables with EMI_TEST_PATHS=1) against the CPU oracle.

Bounds: those of tests/test_lam_gpu.py, tests/lam_ad_common.py and tests/test_gpu_parity.py -- 1e-11 of each field's maximum in fp64, 3e-5
in fp32 (and really computed in float: above 1e-9); white fp32 input also within 3 x the float32 CPU yardstick (floored at 4 epsilons);
the adjoint identity on the sphere 1e-12 / 2e-4.

Observed on an MI355X, the largest error of a case over the lengths of the list (the module takes 38 s).
Limited-area, fp64: band-limited 4.2e-16 ... 2.6e-15 (rows whole and rows cut alike: the same arithmetic), white 3.3e-16 ... 1.3e-15 (mean
wind at most 1.6e-17), adjoints 4.3e-16 ... 2.0e-15; the truncation edges 4.8e-16 ... 1.6e-15 band-limited, 4.1e-16 ... 9.0e-16 white.
Limited-area, fp32: band-limited 1.5e-7 ... 1.5e-6, white 1.2e-7 ... 7.3e-7 (mean wind at most 7.2e-9), on the first white scalar the library
9.2e-8 ... 5.8e-7, the yardstick 7.4e-8 ... 1.9e-7 (at most 1.2 x the floored yardstick), adjoints 2.0e-7 ... 1.8e-6; the truncation edges
2.5e-7 ... 1.2e-6 band-limited, 1.8e-7 ... 6.5e-7 white.
Sphere (short / mid grid; EMI_TEST_PATHS=1 gives the same bits), fp64: inverse 2.3e-15 / 2.4e-15, direct 2.3e-16 / 3.9e-16, white 1.1e-15 /
9.6e-16 per field and 2.3e-15 / 1.8e-15 per total wavenumber, adjoint identities at most 8.1e-18; fp32: inverse 5.9e-7 / 1.2e-6, direct
9.2e-8 / 2.6e-7, white 3.3e-7 / 3.9e-7 per field, on the first scalar the library 1.7e-7 / 3.1e-7 per field and 4.2e-7 / 1.0e-6 per total
wavenumber, the yardstick 1.3e-7 / 1.6e-7 and 3.2e-7 / 2.9e-7 (mid grid, per total wavenumber: 3.5 x the yardstick, inside the bound through
the floor of 4 float32 epsilons on the denominator), adjoint identities at most 4.9e-9."""
import numpy as np
import pytest

from tests import mr_cover, plan_rows
from tests.common import adjoint_case, run_case
from tests.lam_ad_common import ALL, lam_ad_case
from tests.test_gpu_parity import MR_MID, MR_SHORT
from tests.test_gpu_white_direct import check as sphere_white_check
from tests.plan_rows import KSMAX, NDGL, cut
from tests.test_lam_gpu import TOL, mover

pytestmark = pytest.mark.gpu
LISTED = [(n, p) for p in (8, 4) for n in mr_cover.lengths(p)]
IDS = ["%d-fp%d" % (n, 8 * p) for n, p in LISTED]


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=4, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


def check(et, r, n, precision):
    mr_cover.assert_plan(et.etrans_inq(r, "fftplan"), n, precision)


def Handle(et, n, precision, kmsmax=None):
    return plan_rows.Handle(et, n, precision, check, kmsmax)


def forward(et, n, precision, nproma, what, kmsmax=None):
    """lam_case (winds, scalars, all four flags) and lam_white_case on one handle, under the bounds of tests/test_lam_gpu.py"""
    plan_rows.forward(et, n, precision, nproma, check, "mr plan %s %d %s" % (what, n, mr_cover.plan_of(precision, n)), kmsmax)


def test_list_covers_the_plan_space_and_selects_the_recorded_plans(et):
    """on the GPU library as on the emulator (tests/test_emu_mr_plans.py): the frozen list meets the coverage conditions, and every
    length of it selects the recorded plan"""
    for precision in (8, 4):
        assert mr_cover.missing(mr_cover.COVER[precision], precision) == []
        for n in mr_cover.lengths(precision):
            with Handle(et, n, precision):
                pass


@pytest.mark.parametrize("n,precision", LISTED, ids=IDS)
def test_whole_rows(et, n, precision):
    """Rows inside one NPROMA block: the first pass of the direct and the last pass of the inverse transform work on the grid rows."""
    forward(et, n, precision, None, "whole")


@pytest.mark.parametrize("n,precision", LISTED, ids=IDS)
def test_cut_rows(et, n, precision):
    """Rows cut by NPROMA = 4093 (n - 1 for the shorter rows)."""
    forward(et, n, precision, cut(n), "cut")


@pytest.mark.parametrize("n,precision", LISTED, ids=IDS)
def test_adjoints(et, n, precision):
    """EINV_TRANSAD / EDIR_TRANSAD, all flags, rows whole: the `adj` scalings at every bin."""
    to, back = mover("device", precision)
    with Handle(et, n, precision) as h:
        errs = lam_ad_case(et, n, NDGL, h.M, KSMAX, flags=ALL, precision=precision, to_dev=to, to_host=lambda t: t.cpu().numpy(), kresol=h.r)
    print("mr plan adjoints", n, mr_cover.plan_of(precision, n), "fp%d" % (8 * precision), "%.1e" % max(errs.values()))
    assert max(errs.values()) < TOL[precision], errs
    if precision == 4:
        assert max(errs.values()) > 1e-9  # really computed in float


# per precision: two lengths with one field per workgroup, two with several, two with an odd half length
EDGE_LENGTHS = {8: [3168, 4732, 128, 1024, 686, 2574], 4: [5096, 8512, 128, 2304, 650, 2646]}
EDGES = [(n, p, e) for p in (8, 4) for n in EDGE_LENGTHS[p] for e in ("sz/2-1", "sz/2", "sz/2+1", "sz-2")]


@pytest.mark.parametrize("n,precision,edge", EDGES, ids=["%d-fp%d-%s" % (n, 8 * p, e) for n, p, e in EDGES])
def test_truncation_edges(et, n, precision, edge):
    """KMSMAX on both sides of the `k2 <= nmen` switch of FOURIER_IN (sz = n / 2: the mirror sz - k of a bin k > 0 is live from
    KMSMAX = sz / 2 on), and a last bin that is not the neighbour of the row's Nyquist bin; band-limited and white input."""
    sz = n // 2
    forward(et, n, precision, None, "edge " + edge, kmsmax={"sz/2-1": sz // 2 - 1, "sz/2": sz // 2, "sz/2+1": sz // 2 + 1, "sz-2": sz - 2}[edge])


def test_edge_lengths_are_what_they_are_chosen_for():
    for p in (8, 4):
        assert all(n in mr_cover.lengths(p) for n in EDGE_LENGTHS[p])
        fbk = [mr_cover.plan_of(p, n)[3] for n in EDGE_LENGTHS[p]]
        assert fbk[0] == fbk[1] == 1 and fbk[2] > 1 and fbk[3] > 1
        assert all((n // 2) % 2 == 1 for n in EDGE_LENGTHS[p][4:])


# ---- the sphere: 16 latitudes, linear truncation on every row ------------------------------------------------------------------------
# (rows from the pole to the equator, wind pairs, scalars): the fields few, so that the oracle's share of a case stays at a second or two.
# The rows in ascending order, as on any reduced Gaussian grid: with a truncation that follows the row length NMEN must not fall towards
# the equator -- the Legendre transforms take the NDGLU(m) latitudes next to the equator as those of wavenumber m, as the reference does
# (with the lists in their own order, NMEN = 944, 714, 968 ..., both directions are wrong by the size of the fields).
SPHERE = {"short": (sorted(MR_SHORT[-8:]), 2, 3),  # 44 ... 646 points, NSMAX = 322: 16 fields per workgroup, ragged chunks
          "mid": (sorted(MR_MID), 1, 2)}           # 512 ... 2244 points, NSMAX = 1121


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
    assert nsmax <= 1121
    r = et.setup_trans(nsmax, len(nloen), nloen, precision=precision)
    try:
        assert list(et.trans_inq(r, "nmen")) == [min(nsmax, (n - 1) // 2) for n in nloen]
        assert all(f == mr_cover.MR_FAMILY for f in et.trans_inq(r, "fftplan")[:, 0])
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
