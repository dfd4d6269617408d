"""ESETUP_TRANS / EINV_TRANS / EDIR_TRANS on the GPU: the HIP path through the C-ABI against the NumPy model of tests/lam_ref.py
(pinned to the reference's known-answer pair in tests/test_lam_emu.py).  Bounds as tests/test_gpu_parity.py: 1e-11 of each field's
maximum in fp64, 3e-5 in fp32; the golden pair itself at the reference's 1e-10 absolute."""
import os
import subprocess

import numpy as np
import pytest

from tests.lam_common import lam_case, units

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
    finally:
        et.set_max_batch(0)
        del os.environ["EMI_TEST_PATHS"]
    assert max(errs.values()) < TOL[8], errs
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
