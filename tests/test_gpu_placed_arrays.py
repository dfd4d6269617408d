"""Caller-placed device arrays on the GPU: every array of a call sits inside a larger sentinel-filled device buffer at element offset 0
(control) and 1 (tests/common.py::GuardedSpace), as a field inside a caller's work array or ZGP(:,:,2:) does, and is used in place.
The FFT kernels choose between a row-as-one-buffer path and an element path from the alignment of each row; with freshly allocated
tensors and the even row lengths of the long-row lists that choice never sees an odd start.  Checked per case: nothing outside the
defined elements is written (guard bands, the padding of the last NPROMA block, a surplus field -- all NaN / sentinel, bit for bit),
inputs come back bit for bit, NaN in the padding and the surplus field of an input reaches no output, and the results match the oracle
to the bounds of tests/test_gpu_parity.py (1e-11 in fp64, 3e-5 in fp32); in fp64 the two offsets agree to 1e-13.  The adjoints and
GPNORM_TRANS are compared with the same calls on plainly allocated arrays with zero padding.  tests/test_emu_placed_arrays.py runs the
same case functions on the CPU emulator."""
import numpy as np
import pytest

from tests.common import (GuardedSpace, assert_placed, guard_for, octahedral, placed_arrays_case, placed_call_mode2_case,
                          placed_gpnorm_case, random_spectrum, rel_err)
from tests.test_gpu_parity import (BLUE, H9, HOT_A, HOT_B, HOT_D, MR_LONG, MR_MID, MR_SHORT, MR_XL, ODD, R16_ROWS, R16S_ROWS)

pytestmark = pytest.mark.gpu
TOL = {8: 1e-11, 4: 3e-5}
FLAGS = dict(scders=True, vorgp=True, divgp=True, uvder=True)


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=6, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


@pytest.fixture(scope="module")
def dev():
    """(to_flat, back): a flat numpy buffer -> device tensor; a tensor or a view of one -> numpy of the same dtype"""
    import torch
    return (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")), (lambda t: t.cpu().numpy())


def Oracle(*a, **k):
    from oracle.oracle import Oracle as O
    return O(*a, **k)


CONV = {"EMI_FFT_MR": "0"}  # keep rows with a 23-smooth half-length off the direct mixed-radix kernels
HOT = dict(CONV, EMI_FFT_R16S="0")
GM = {8: [10244, 10256, 5136, 20484], 4: [20484, 40964, 1284]}
# family -> (rows of one hemisphere, environment, an odd NPROMA above the longest row and below NGPTOT): the smallest grids that select
# each FFT kernel family.  With an odd NPROMA (block * fields + field) * NPROMA changes parity from field to field and block to
# block: one launch -- for the short rows one workgroup -- mixes aligned rows, misaligned rows and a few cut rows, already at lead 0.
FAMILIES = {
    "generic_H9": (H9, {}, 53), "generic_ODD": (ODD, {}, 39), "bluestein_BLUE": (BLUE, {}, 63),
    "hot_A": (HOT_A, HOT, 20001), "hot_B": (HOT_B, HOT, 20001), "hot_D": (HOT_D, HOT, 2501),
    "r16": (R16_ROWS, CONV, 20001), "r16p": (R16S_ROWS, CONV, 20001),
    "mr_SHORT": (MR_SHORT, {}, 1001), "mr_MID": (MR_MID, {}, 5001), "mr_LONG": (MR_LONG, {}, 20001), "mr_XL": (MR_XL, {}, 20001),
    "gm": (GM, {}, 30001),
}
WHOLE_AND_ODD = [(f, p, n) for f in FAMILIES for p, n in ((8, None), (4, None), (8, "odd"))]
CUT_FP32 = [(f, 4, 1001) for f in ("hot_A", "r16", "r16p", "mr_LONG")]  # NPROMA blocks that cut the rows, in fp32


def both_leads(et, dev, monkeypatch, family, precision, nproma, adjoint=False):
    rows, env, odd = FAMILIES[family]
    half = rows[precision] if isinstance(rows, dict) else rows
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nproma = odd if nproma == "odd" else nproma
    nsc = 9 if half[0] < 1000 else 3  # short rows: 2 / 4 / 8 fields per workgroup, ragged
    what = "%s nproma %s%s" % (family, nproma, " adjoints" if adjoint else "")
    control = None
    for lead in (0, 1):
        run = placed_arrays_case(et, Oracle, dev, 15, half + half[::-1], 2, nsc, FLAGS, nproma, precision, lead, adjoint=adjoint)
        assert_placed(run, precision, TOL[precision], what="%s lead %d" % (what, lead), control=control)
        control = run


@pytest.mark.parametrize("family,precision,nproma", WHOLE_AND_ODD + CUT_FP32)
def test_placed_arrays_match_oracle_and_stay_inside(et, dev, monkeypatch, family, precision, nproma):
    both_leads(et, dev, monkeypatch, family, precision, nproma)


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("family,nproma", [("r16", None), ("r16p", 20001), ("mr_MID", None), ("generic_H9", 37)])
def test_placed_arrays_adjoints(et, dev, monkeypatch, family, nproma, precision):
    both_leads(et, dev, monkeypatch, family, precision, nproma, adjoint=True)


@pytest.mark.parametrize("paths", [0, 4])
@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("nsmax", [128, 254])
def test_placed_spectral_arrays_of_the_direct_legendre_kernel(et, dev, monkeypatch, nsmax, precision, paths):
    """the epilogue of k_leg_dir writes the caller's spectral arrays directly (EMI_TEST_PATHS=4: k_postpack_dir does): the 6-latitude grid
    of test_direct_legendre_row_tiles, two of its tile-edge truncations"""
    monkeypatch.setenv("EMI_TEST_PATHS", str(paths))
    half = [min(20 + 4 * i, 2 * nsmax + 4) for i in range(6)]
    control = None
    for lead in (0, 1):
        run = placed_arrays_case(et, Oracle, dev, nsmax, half + half[::-1], 1, 2, {}, None, precision, lead)
        assert_placed(run, precision, TOL[precision], what="legendre N %d paths %d lead %d" % (nsmax, paths, lead), control=control)
        control = run


def test_placed_arrays_call_mode_2(et, dev):
    for lead in (0, 1):
        errs, viol = placed_call_mode2_case(et, Oracle, dev, lead)
        print("call mode 2, lead", lead, errs, viol)
        assert not viol, viol
        assert max(errs.values()) < TOL[8], errs


def test_placed_arrays_gpnorm(et, dev):
    err, viol = placed_gpnorm_case(et, dev)
    print("GPNORM_TRANS on placed arrays against plain ones: %.2e" % err)
    assert not viol, viol
    assert err < 1e-14


def test_placed_arrays_specnorm_of_a_slice(et, dev):
    """SPECNORM of PSPSC3A(:,:,v): a contiguous slice that starts inside a guarded array, against the oracle (1e-10, the bound of the
    spectral norms in tests/test_gpu_parity.py)"""
    N, nvar, nlev = 21, 3, 5
    nloen = octahedral(N)
    o = Oracle(N, nloen)
    sc3 = np.stack([random_spectrum(np.random.default_rng(3 + v), o.nasm0, N, o.nspec2, nlev, False) for v in range(nvar)])
    r = et.setup_trans(N, len(nloen), nloen)
    try:
        for lead in (0, 1):
            space = GuardedSpace(lead, guard_for(nloen.max()), *dev)
            a = space.put(sc3, "in")
            for v in range(nvar):
                got = et.specnorm(r, a[v])
                assert np.abs(got / o.specnorm(sc3[v]) - 1.0).max() < 1e-10, (lead, v, got)
            assert not space.check()
    finally:
        et.trans_release(r)


def test_placed_arrays_vordiv_to_uv(et, dev):
    """VORDIV_TO_UV with all four arrays guarded, the outputs pre-filled with NaN"""
    N, nf = 21, 3
    o = Oracle(N, octahedral(N))
    rng = np.random.default_rng(5)
    vor, div = (random_spectrum(rng, o.nasm0, N, o.nspec2, nf, True) for _ in range(2))
    ur, vr = o.vordiv_to_uv(vor, div)
    for lead in (0, 1):
        space = GuardedSpace(lead, guard_for(2 * (N + 1) * nf), *dev)
        u, v = (space.put(np.full_like(vor, np.nan), "out") for _ in range(2))
        et.vordiv_to_uv(space.put(vor, "in"), space.put(div, "in"), N, pspu=u, pspv=v)
        assert not space.check()
        gu, gv = dev[1](u), dev[1](v)
        assert np.all(np.isfinite(gu)) and np.all(np.isfinite(gv))
        assert max(rel_err(gu, ur), rel_err(gv, vr)) < TOL[8], lead


class PlacedCalls:
    """The package with every array of a transform call given its role in `space` (spectral arrays and mean winds are inputs of the
    inverse transforms and outputs of the direct ones, grid arrays the other way round) and GuardedSpace.check() after each call: for the
    case functions that take the package and a mover (lam_case, lonlat_case)."""
    CALLS = {"inv_trans": True, "einv_trans": True, "dir_trans": False, "edir_trans": False}  # -> spectral arrays are inputs

    def __init__(self, et, space):
        self.et, self.space, self.violations, self.calls = et, space, [], 0

    def __getattr__(self, name):
        f = getattr(self.et, name)
        if name not in self.CALLS:
            return f

        def call(r, **kw):
            for k, v in kw.items():
                if any(v is rec[1] for rec in self.space.recs):
                    self.space.set_role(v, "in" if (k.startswith("psp") or k.startswith("pmean")) == self.CALLS[name] else "out")
            f(r, **kw)
            self.violations += self.space.check()
            self.calls += 1
        return call


def test_placed_arrays_limited_area(et, dev):
    """EINV_TRANS / EDIR_TRANS on guarded device arrays: the split-array geometry of tests/test_lam_emu.py, against tests/lam_ref.py"""
    from tests.lam_common import lam_case
    for lead in (0, 1):
        space = GuardedSpace(lead, guard_for(40), *dev)
        calls = PlacedCalls(et, space)
        errs, _ = lam_case(calls, 40, 36, 13, 17, split=True, nproma=64, to_dev=lambda a: space.put(a, "out"),
                           to_host=lambda t: dev[1](t).astype(np.float64))
        print("limited area, lead", lead, {k: "%.1e" % v for k, v in errs.items()})
        assert calls.calls == 2 and not calls.violations, calls.violations
        assert max(errs.values()) < TOL[8], errs


def test_placed_arrays_latlon_inverse(et, dev):
    """INV_TRANS(LDLATLON) onto a guarded device array: the smallest grid of tests/test_lonlat_gpu.py, against tests/lonlat_ref.py"""
    from tests.lonlat_ref import lonlat_case
    for lead in (0, 1):
        space = GuardedSpace(lead, guard_for(3600), *dev)
        calls = PlacedCalls(et, space)
        errs, _ = lonlat_case(calls, 255, 37, 3600, to=lambda a: space.put(np.ascontiguousarray(a, dtype=np.float64), "out"),
                              back=lambda t: dev[1](t).astype(np.float64))
        assert calls.calls == 1 and not calls.violations, calls.violations
        assert max(errs.values()) < TOL[8], errs
