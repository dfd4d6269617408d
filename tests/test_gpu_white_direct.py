"""DIR_TRANS on full-bandwidth grid fields: the HIP path through the C-ABI against the CPU oracle on U(-1,1) white noise.

Every other parity test hands the direct transform a band-limited field -- the oracle's own inverse transform of a truncated
spectrum -- which holds exactly zero energy where DIR_TRANS must discard energy: on latitude row j at the zonal wavenumbers
m > NMEN(j).  The truncation fused into every FFT epilogue, the per-wavenumber latitude lists of k_leg_dir and the FOURIER_OUT rows of
the exchange-order tables can all be wrong without those tests noticing.  White fields have energy at every m of every row and a flat
spectrum, so an error is judged sharply at every total wavenumber; the padding of the last NPROMA block is NaN, as a Fortran caller's
uninitialised padding may be.  The oracle itself is checked on such fields against a plain summation in tests/test_emu_parity.py.

The cases are those that select a kernel family in tests/test_gpu_parity.py, with the same environment switches.

Bounds.  fp64: 1e-11 of each field's largest coefficient (TOL) and 1e-10 of the largest coefficient of each total wavenumber (the
tol_group of tests/test_gpu_fullsize.py).  fp32: 3e-5 per field and, on the first scalar field, at most 3 x the error of
fp32_columns_direct -- a plain float32 CPU chain, reference arithmetic only -- both against the fp64 oracle, the denominator floored
at 4 float32 epsilons (the rule of tests/test_gpu_fullsize.py), in both measures.

Observed on an MI355X, per field / per total wavenumber.  fp64, all fields:
    named cases 6.5e-16 ... 2.5e-15 / 1.3e-15 ... 1.6e-14    k_fft_dir_hot 1.0 ... 1.1e-15 / 1.9 ... 3.4e-15    k_fft_dir_mr 8.1 ... 9.5e-16 / 1.2 ... 2.7e-15
    k_fft_dir_r16 1.3e-15 / 2.5e-15    k_fft_dir_r16p 1.0e-15 / 4.1e-15    exchange-order tables 8.4e-16 / 2.6e-15    k_fft_dir_gm 1.2e-15 / 3.3e-15
    Legendre tiles 6.2 ... 6.5e-16 / 2.0e-15    O160 2.5e-15 / 4.2e-15    O640 7.1e-15 / 8.9e-15    random grids 4.8e-16 ... 1.2e-15 / 7.7e-16 ... 5.7e-15
    EMI_TEST_PATHS 1, 2, 4, 7 1.2e-15 / 1.2e-14    host arrays 1.1e-15 / 2.5e-15
fp32, all fields; then the library and the yardstick on the first scalar field:
    named cases 1.7e-7 ... 2.0e-6 / 2.9e-7 ... 1.0e-5; library 1.2 ... 4.3e-7 / 2.6 ... 7.9e-7, yardstick 1.0 ... 1.8e-7 / 1.8 ... 3.7e-7
    k_fft_dir_hot 2.7 ... 4.2e-7 / 4.1e-7 ... 1.2e-6; library 2.1 ... 2.9e-7 / 3.3e-7 ... 1.2e-6, yardstick 1.7 ... 2.7e-7 / 2.9e-7 ... 1.7e-6
    k_fft_dir_mr 2.7 ... 4.2e-7 / 5.6e-7 ... 3.9e-6; library 1.2 ... 3.9e-7 / 2.4 ... 7.0e-7, yardstick 1.0 ... 1.5e-7 / 2.5 ... 3.3e-7
    k_fft_dir_r16 2.9e-7 / 8.9e-7; library 2.9e-7 / 5.8e-7, yardstick 2.4e-7 / 5.1e-7
    k_fft_dir_r16p 2.8e-7 / 6.2e-7; library 2.6e-7 / 4.3e-7, yardstick 1.6e-7 / 2.7e-7
    exchange-order tables 3.6e-7 / 1.9e-6; library 2.9e-7 / 5.6e-7, yardstick 1.3e-7 / 3.1e-7
    k_fft_dir_gm 3.4e-7 / 3.4e-6; library 2.4e-7 / 5.0e-7, yardstick 1.9e-7 / 2.6e-7
    Legendre tiles 1.8 ... 2.5e-7 / 4.2 ... 4.7e-7; library 1.5 ... 1.6e-7 / 3.1e-7, yardstick 1.1 ... 1.2e-7 / 4.7e-7
    O160 2.0e-6 / 3.2e-6; library 4.3e-7 / 7.9e-7, yardstick 1.8e-7 / 2.8e-7
    O640 8.1e-6 / 1.4e-5; library 8.6e-7 / 1.3e-6, yardstick 2.4e-7 / 4.0e-7 (3.6 and 3.3 x the yardstick: inside the bound 3 x 4 epsilons =
    1.43e-6 only through the floor on the denominator)
"""
import numpy as np
import pytest

from tests.common import assert_white, octahedral, white_direct_case
from tests.test_gpu_parity import (CASES, FP32_CASES, HOST, HOT_A, HOT_B, HOT_C, HOT_D, HOT_E, MR_LONG, MR_MID, MR_SHORT, MR_XL, R16_ROWS,
                                   R16S_ROWS, TILE_EDGE_N)

pytestmark = pytest.mark.gpu
TOL, TOL_N, TOL32 = 1e-11, 1e-10, 3e-5


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=4, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


@pytest.fixture(scope="module")
def dev():
    import torch
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    back = lambda t: t.cpu().numpy()
    return to, back


def Oracle(*a, **k):
    from oracle.oracle import Oracle as O
    return O(*a, **k)


def check(et, xp, nsmax, nloen, nuv, nsc, nproma, precision, what, **kw):
    res = white_direct_case(et, Oracle, xp, nsmax, nloen, nuv, nsc, nproma, precision=precision, **kw)
    if precision == 8:
        assert_white(res, 8, TOL, TOL_N, what)
    else:
        assert_white(res, 4, TOL32, None, what)
        assert res["field"] > 1e-9  # really computed in float
    return res


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_cases(et, dev, name):
    """Every entry of CASES (octahedral, full and linear grids, Bluestein and odd rows, NPROMA blocks, two column tiles, a truncation
    above the grid's) in fp64.  Observed 6.5e-16 ... 2.5e-15 per field, 1.3e-15 ... 1.6e-14 per total wavenumber."""
    nsmax, nloen, nuv, nsc, _, nproma = CASES[name]
    check(et, dev, nsmax, nloen, nuv, nsc, nproma, 8, name)


@pytest.mark.parametrize("name", FP32_CASES)
def test_named_cases_fp32(et, dev, name):
    """FP32_CASES in the fp32 library.  Observed on the first scalar field: the library 1.2e-7 ... 4.3e-7 per field and 2.6e-7 ... 7.9e-7 per total
    wavenumber, the yardstick 1.0e-7 ... 1.8e-7 and 1.8e-7 ... 3.7e-7."""
    nsmax, nloen, nuv, nsc, _, nproma = CASES[name]
    check(et, dev, nsmax, nloen, nuv, nsc, nproma, 4, name)


@pytest.mark.parametrize("half,precision", [(HOT_A, 8), (HOT_B, 8), (HOT_A, 4), (HOT_B, 4), (HOT_C, 4), (HOT_C, 8), (HOT_D, 8), (HOT_E, 8),
                                            (HOT_D, 4)])
def test_specialised_fft_kernels(et, dev, half, precision, monkeypatch):
    """k_fft_dir_hot: the truncating epilogue of every specialised Bluestein work length (rows kept off the mixed-radix and split kernels)."""
    monkeypatch.setenv("EMI_FFT_MR", "0")
    monkeypatch.setenv("EMI_FFT_R16S", "0")
    nsc = 3 if half[0] > 1000 else 9
    check(et, dev, 15, half + half[::-1], 2, nsc, None, precision, "hot %d" % half[0])


@pytest.mark.parametrize("rows,precision,nproma", [(MR_SHORT, 8, None), (MR_MID, 8, None), (MR_LONG, 8, None), (MR_SHORT, 4, None), (MR_MID, 4, None),
                                                   (MR_LONG, 4, None), (MR_SHORT, 8, 37), (MR_MID, 8, 1000), (MR_LONG, 8, 4094), (MR_LONG, 4, 1000), (MR_XL, 8, None), (MR_XL, 4, None)])
def test_direct_mixed_radix_fft_kernels(et, dev, rows, precision, nproma):
    """k_fft_dir_mr: one-, two- and three-pass plans, whole rows and rows cut by NPROMA blocks (NaN behind the last one)."""
    nsc = 3 if rows[0] > 1000 else 9
    check(et, dev, 15, rows + rows[::-1], 2, nsc, nproma, precision, "mr %d" % rows[0])


@pytest.mark.parametrize("precision,nproma", [(8, 1000), (4, 1000), (8, 4094)])
def test_register_resident_fft_kernels(et, dev, precision, nproma, monkeypatch):
    """k_fft_dir_r16 on NPROMA-cut rows"""
    monkeypatch.setenv("EMI_FFT_MR", "0")
    check(et, dev, 15, R16_ROWS + R16_ROWS[::-1], 2, 3, nproma, precision, "r16")


@pytest.mark.parametrize("precision,nproma", [(8, None), (4, None), (8, 1000), (4, 4094)])
def test_split_register_resident_fft_kernels(et, dev, precision, nproma, monkeypatch):
    """k_fft_dir_r16p, with the in-place kernels of the odd half-lengths beside them"""
    monkeypatch.setenv("EMI_FFT_MR", "0")
    check(et, dev, 15, R16S_ROWS + R16S_ROWS[::-1], 2, 3, nproma, precision, "r16p")


@pytest.mark.parametrize("precision", [8, 4])
def test_long_row_fft_kernels_through_the_exchange_order_tables(et, dev, precision, monkeypatch):
    """The FOURIER_OUT rows of the exchange-order tables (EMI_TEST_PATHS bit 0) under every long-row kernel family"""
    monkeypatch.setenv("EMI_TEST_PATHS", "1")
    rows = [1540, 2052, 3076, 4092, 4100, 4102, 5120, 5124, 6146, 2048, 3840, 4800]
    check(et, dev, 15, rows + rows[::-1], 1, 2, None, precision, "fftrow")


@pytest.mark.parametrize("half,precision", [([10244, 10248, 10252, 10256, 5136, 20484], 8), ([20484, 20500, 40964, 1284], 4)])
def test_rows_longer_than_the_lds(et, dev, half, precision):
    """k_fft_dir_gm: the passes on a global scratch buffer"""
    check(et, dev, 7, half + half[::-1], 2, 3, 10000, precision, "gm")


@pytest.mark.parametrize("nsmax", TILE_EDGE_N)
@pytest.mark.parametrize("precision", [8, 4])
def test_direct_legendre_row_tiles(et, dev, nsmax, precision):
    """k_leg_dir's row tiles with white rows on the six-latitude grid of tests/test_gpu_parity.py: most wavenumbers lie above every
    row's NMEN, the others see a few latitudes of a long Legendre side."""
    half = np.array([min(20 + 4 * i, 2 * nsmax + 4) for i in range(6)], dtype=np.int32)
    check(et, dev, nsmax, np.concatenate([half, half[::-1]]), 1, 2, None, precision, "tiles N=%d" % nsmax)


@pytest.mark.parametrize("nsmax,precision", [(159, 8), (159, 4), (639, 8), (639, 4)])
def test_large_octahedral_grids(et, dev, nsmax, precision):
    """O160 and O640 with 2 wind pairs + 3 scalars: most rows have NMEN < NSMAX, so most (row, m) pairs of the white field hold energy
    that the per-wavenumber latitude lists of k_leg_dir must leave out; the MFMA tiles at real occupancy."""
    check(et, dev, nsmax, octahedral(nsmax), 2, 3, None, precision, "O%d" % (nsmax + 1))


@pytest.mark.parametrize("seed", range(40))
def test_random_reduced_grids(et, dev, seed):
    """Random reduced grids, truncations, field counts and NPROMA drawn as test_random_reduced_grids_match_oracle draws them, from seeds
    of their own (offset 7000).  Observed 4.8e-16 ... 1.2e-15 per field, 7.7e-16 ... 5.7e-15 per total wavenumber."""
    rng = np.random.default_rng(7000 + seed)
    nh = int(rng.integers(4, 14))
    half = np.sort(rng.integers(8, 700, nh))
    nloen = np.concatenate([half, half[::-1]]).astype(np.int32)
    nsmax = int(rng.integers(2, 2 * nh))
    nuv, nsc = int(rng.integers(0, 3)), int(rng.integers(0, 4))
    if nuv + nsc == 0:
        nsc = 1
    for _ in range(4):  # the four option draws of that test: a direct transform takes no options, the stream stays in step
        rng.integers(2)
    nproma = [None, 17, 100, 1000][int(rng.integers(4))]
    res = white_direct_case(et, Oracle, dev, nsmax, nloen, nuv, nsc, nproma, seed=seed)
    assert_white(res, 8, TOL, TOL_N, (nloen.tolist(), nsmax, nuv, nsc, nproma))


@pytest.mark.parametrize("paths", [1, 2, 4, 7])
def test_multi_task_code_paths_on_one_task(et, dev, paths, monkeypatch):
    """EMI_TEST_PATHS: the exchange-order tables, the three-stream pipeline and k_postpack_dir at O32 with 40 wind pairs + 200 scalars"""
    monkeypatch.setenv("EMI_TEST_PATHS", str(paths))
    check(et, dev, 31, octahedral(31), 40, 200, None, 8, "paths %d" % paths)


def test_host_arrays(et):
    """EMI_MEM_HOST: numpy arrays staged over PCIe, NaN padding included"""
    check(et, HOST, 31, octahedral(31), 2, 3, 500, 8, "host")
