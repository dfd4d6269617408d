"""ESETUP_TRANS / EINV_TRANS / EDIR_TRANS on the GPU: the HIP path through the C-ABI against the NumPy model of tests/lam_ref.py
(pinned to the reference's known-answer pair in tests/test_lam_emu.py).  Bounds as tests/test_gpu_parity.py: 1e-11 of each field's
maximum in fp64, 3e-5 in fp32; the golden pair itself at the reference's 1e-10 absolute."""
import os
import subprocess

import numpy as np
import pytest

from tests.lam_common import lam_case, lam_white_case, units

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "antwrp1300")
TOL = {8: 1e-11, 4: 3e-5}


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=4, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


def mover(memory, precision):
    """(to, back) for the arrays of a call in `memory`"""
    dt = np.float32 if precision == 4 else np.float64
    if memory == "host":
        return (lambda a: np.ascontiguousarray(a, dtype=dt)), (lambda a: np.asarray(a, dtype=np.float64))
    import torch
    return (lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")), (lambda t: t.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("memory", ["device", "host"])
def test_golden_pair(et, memory):
    sp, gp = np.load(os.path.join(GOLD, "antwrp1300-s1t@sp.npy")), np.load(os.path.join(GOLD, "antwrp1300-s1t@sp2gp.npy"))
    to, back = mover(memory, 8)
    exwn, eywn = units(54, 48)
    r = et.esetup_trans(26, 23, 48, kdgux=37, kdlon=54, pexwn=exwn, peywn=eywn)
    assert (et.etrans_inq(r, "ngptot"), et.etrans_inq(r, "nspec2")) == (2592, 1968)
    out, s = to(np.zeros((1, 1, 2592))), to(np.zeros((1968, 1)))
    et.einv_trans(r, pspscalar=to(sp[:, None]), pgp=out)
    et.edir_trans(r, pspscalar=s, pgp=to(gp.reshape(1, 1, -1)))
    e_inv, e_dir = np.abs(back(out)[0, 0] - gp.ravel()).max(), np.abs(back(s)[:, 0] - sp).max()
    et.trans_release(r)
    print("golden pair (%s arrays): inverse %.2e direct %.2e" % (memory, e_inv, e_dir))
    assert e_inv < 1e-10 and e_dir < 1e-10


# (ndlon, ndgl, M, N, keywords): every case with wind and a non-zero mean wind, scalars and all four derivative / wind flags
CASES = {
    "smooth_384x320": (384, 320, 127, 105, {}),                                   # quadratic truncation
    "linear_400x300": (400, 300, 199, 149, {}),
    "prime_y_300x251": (300, 251, 99, 83, dict(nproma=1000)),                     # Bluestein in y; NPROMA cuts rows
    "prime_x_257x256": (257, 256, 85, 85, {}),                                    # Bluestein in x
    "odd_x_factor7_y_405x294": (405, 294, 134, 97, dict(split=True)),             # 294 = 2 3 7 7
    "factor11_352x242": (352, 242, 117, 80, dict(split=True, nproma=4096)),       # 352 = 32 11, 242 = 2 11 11
    "m_zero": (128, 96, 0, 31, {}),
    "n_zero": (128, 96, 42, 0, {}),
}


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity(et, name, memory, precision):
    ndlon, ndgl, M, N, kw = CASES[name]
    to, back = mover(memory, precision)
    errs, _ = lam_case(et, ndlon, ndgl, M, N, precision=precision, to_dev=to, to_host=back, **kw)
    print(name, memory, precision, {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < TOL[precision], errs
    if precision == 4:
        assert max(errs.values()) > 1e-9  # really computed in float


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
def test_user_size(et, memory, precision):
    """1536 x 1440 with linear truncation 767 x 719, 32 grid fields (8 wind pairs, 16 scalars), both directions"""
    to, back = mover(memory, precision)
    errs, _ = lam_case(et, 1536, 1440, 767, 719, nuv=8, nsc=16, flags=False, precision=precision, to_dev=to, to_host=back)
    print("1536 x 1440", memory, precision, {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < TOL[precision], errs


def white_check(et, ndlon, ndgl, M, N, memory, precision, what, **kw):
    """lam_white_case under the bounds of this module; fp32: in addition at most 3 x the error of the float32 yardstick on the first
    scalar field, the denominator floored at 4 float32 epsilons (the rule of tests/test_gpu_fullsize.py)"""
    to, back = mover(memory, precision)
    errs, yard = lam_white_case(et, ndlon, ndgl, M, N, precision=precision, to_dev=to, to_host=back, **kw)
    print("white", what, memory, precision, {k: "%.1e" % v for k, v in errs.items()}, yard)
    assert max(errs.values()) < TOL[precision], errs
    if precision == 4:
        assert max(errs.values()) > 1e-9  # really computed in float
        assert yard["lib"] <= 3.0 * max(yard["cpu"], 4 * float(np.finfo(np.float32).eps)), yard


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_white_direct(et, name, memory, precision):
    """EDIR_TRANS of full-bandwidth (white) fields on every size of CASES: energy above KMSMAX in every row and outside the ellipse, which
    the fields of test_parity do not hold; NaN in the padding of the last NPROMA block.  Observed on an MI355X: fp64 3.5e-16 ... 1.3e-15
    (mean wind at most 2.2e-18); fp32 all fields 1.9e-7 ... 5.2e-7 (mean wind at most 9.9e-10), on the first scalar the library 1.0e-7 ... 2.7e-7, the
    yardstick 1.1e-7 ... 2.2e-7."""
    ndlon, ndgl, M, N, kw = CASES[name]
    white_check(et, ndlon, ndgl, M, N, memory, precision, name, **kw)


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
def test_white_direct_user_size(et, memory, precision):
    """1536 x 1440, 8 wind pairs + 16 scalars of white noise.  Observed: fp64 9.3e-16; fp32 all fields 5.7e-7, on the first scalar the library
    4.4e-7, the yardstick 1.4e-7 (3.1 x: inside the bound 3 x 4 float32 epsilons = 1.43e-6 only through the floor on the denominator)."""
    white_check(et, 1536, 1440, 767, 719, memory, precision, "1536 x 1440", nuv=8, nsc=16)


# x-rows longer than 1536 points: the kernel families a limited-area handle had never run.  What fft_choose (csrc/ectrans_mi.hip) picks for
# NDLON, half-length sz = NDLON / 2 (EMI_FFT_MR=0 where sz is a product of three radices of the direct mixed-radix kernels, as on the sphere):
LONG_X = [
    (1540, dict(EMI_FFT_MR="0")),   # k_fft_*_r16<8>: convolution length 2 sz - 1 = 1539 <= 2048 (sz = 770 = 10 7 11: mixed radix unless switched off)
    (2052, dict(EMI_FFT_MR="0")),   # k_fft_*_r16<10>: 2051 <= 2560 (sz = 1026 = 6 9 19)
    (4092, {}),                     # k_fft_*_r16<16>: 4091 <= 4096 (sz = 2046 = 2 3 11 31: no mixed-radix plan)
    (4100, {}),                     # k_fft_*_r16p<10>: 4099 > 4096 and sz = 2050 even: two convolutions of sz / 2 points, length sz - 1 = 2049 <= 256 x 10
    (5124, {}),                     # k_fft_*_r16p<12>: sz - 1 = 2561 > 2560, <= 256 x 12
    (8192, dict(EMI_FFT_MR="0")),   # k_fft_*_r16p<16>: sz - 1 = 4095 <= 256 x 16 (sz = 16^3: mixed radix unless switched off)
    (4102, {}),                     # k_fft_*_hot, in place: sz = 2051 is odd, no split
    (1284, {}),                     # k_fft_*_hot: 1283 <= 1536, several fields per workgroup (sz = 642 = 2 3 107)
    (1284, dict(EMI_FFT_R16S="0")),  # ... the switch of the split kernels has no effect at this length (they are considered above 4096 only): the same kernel again
    (1601, {}),                     # odd (prime) NDLON: the generic complex path, convolution length 3240
]


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("ndlon,env", LONG_X, ids=["%d%s" % (n, "".join("-" + k + v for k, v in e.items())) for n, e in LONG_X])
def test_long_x_rows(et, ndlon, env, precision, monkeypatch):
    """Each family of LONG_X on a limited-area handle with few rows (NDGL = 40, so that the x-rows dominate): band-limited input in both
    directions (lam_case) and white input (lam_white_case), linear truncation.  Observed on an MI355X: fp64 1.8e-15 ... 2.3e-15 (band-limited), 7.9e-16 ... 1.2e-15 (white); fp32 4.5e-7 ... 6.6e-7
    (band-limited), 2.3e-7 ... 3.8e-7 (white); on the first white scalar the library 1.8e-7 ... 2.6e-7, the yardstick 1.3e-7 ... 2.9e-7."""
    ndgl = 40
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    to, back = mover("device", precision)
    M, N = (ndlon - 1) // 2, ndgl // 2 - 1
    errs, _ = lam_case(et, ndlon, ndgl, M, N, nuv=2, nsc=3, nproma=3000, precision=precision, to_dev=to, to_host=back)
    print("long x", ndlon, precision, {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < TOL[precision], errs
    white_check(et, ndlon, ndgl, M, N, "device", precision, "long x %d" % ndlon, nproma=3000)


# (NDGL, NDLON, precision): y-lengths whose work array needs more than 80 KiB of LDS per workgroup -- two fields, 512 threads (build_fft_plans)
LARGE_Y = [(1499, 24, 8),    # prime: convolution length 3000, 48 KiB per field in fp64
           (1499, 24, 4),    # (24 KiB per field in fp32: three fields -> two, 512 threads)
           (5103, 20, 8),    # 3^6 7, mixed radix: 5104 + 1 complex numbers per field, the set-up limit is 5120
           (10206, 20, 4)]   # 2 3^6 7: 10208 + 1 of at most 10240 in fp32


@pytest.mark.parametrize("ndgl,ndlon,precision", LARGE_Y)
def test_large_y_lengths(et, ndgl, ndlon, precision):
    """k_lam_inv / k_lam_dir with the largest work arrays the set-up accepts, band-limited and white input.  Observed on an MI355X: fp64 1.1e-15 ... 2.3e-15
    (band-limited), 5.2e-16 ... 9.7e-16 (white); fp32 4.6e-7 ... 4.8e-7 (band-limited), 2.1e-7 ... 2.5e-7 (white); on the first white scalar the library
    1.4e-7 ... 1.7e-7, the yardstick 1.4e-7 ... 2.1e-7."""
    to, back = mover("device", precision)
    M, N = ndlon // 2 - 1, (ndgl - 1) // 2
    errs, _ = lam_case(et, ndlon, ndgl, M, N, nuv=1, nsc=2, nproma=4096, precision=precision, to_dev=to, to_host=back)
    print("large y", ndgl, precision, {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < TOL[precision], errs
    white_check(et, ndlon, ndgl, M, N, "device", precision, "large y %d" % ndgl, nuv=1, nsc=2, nproma=4096)


def test_batches_and_phase_slots(et):
    """several batches (set_max_batch; on the GPU a call of 256 fields and more runs them through the three-stream pipeline when
    EMI_TEST_PATHS asks for it), and the y-direction transform reported in the Legendre slot of the phase timers"""
    to, back = mover("device", 8)
    et.set_max_batch(64)
    try:
        errs, _ = lam_case(et, 96, 80, 31, 26, nuv=40, nsc=60, to_dev=to, to_host=back)
    finally:
        et.set_max_batch(0)
    assert max(errs.values()) < TOL[8], errs
    os.environ["EMI_TEST_PATHS"] = "2"
    et.set_max_batch(128)
    try:
        errs, _ = lam_case(et, 96, 80, 31, 26, nuv=50, nsc=80, to_dev=to, to_host=back)
        # The direct call above has 2 x 50 + 80 = 180 Fourier fields, below the 256 from which a call is pipelined: only its inverse
        # leg (with the derivative fields) runs on three streams.  2 x 50 + 160 = 260 white fields take k_lam_dir through the pipeline.
        werrs, _ = lam_white_case(et, 96, 80, 31, 26, nuv=50, nsc=160, nproma=1000, to_dev=to, to_host=back)
    finally:
        et.set_max_batch(0)
        del os.environ["EMI_TEST_PATHS"]
    assert max(errs.values()) < TOL[8], errs
    assert max(werrs.values()) < TOL[8], werrs
    r = et.esetup_trans(31, 26, 80, kdlon=96, pexwn=1.0, peywn=1.0)
    sc, gp = to(np.zeros((et.etrans_inq(r, "nspec2"), 3))), to(np.zeros((1, 3, 96 * 80)))
    et.set_profile(1)
    try:
        import torch
        for fn in (et.einv_trans, et.edir_trans):
            fn(r, pspscalar=sc, pgp=gp)
            torch.cuda.synchronize()
            ms, n = et.last_phase_ms(), et.last_phase_launches()
            assert n == [0, 1, 1] and ms[0] == 0.0 and ms[1] > 0.0 and ms[2] > 0.0, (ms, n)
    finally:
        et.set_profile(0)
    et.trans_release(r)


def test_fortran_shim_lam():
    """tests/fortran/test_shim_lam.F90 on the real library: the ETRANS_INQ numbers, a single harmonic with LDSCDERS against its closed
    form, a wind round trip with the mean wind, the dp and sp entry points; a refusal aborts with the ABORT_TRANS text"""
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_lam"])
    exe = os.path.join(d, "test_shim_lam")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "FORTRAN SHIM LAM OK (dp and sp)" in p.stdout, p.stdout + p.stderr
    p = subprocess.run([exe, "invtrans"], capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout and "limited-area handle" in p.stderr, p.stdout + p.stderr
