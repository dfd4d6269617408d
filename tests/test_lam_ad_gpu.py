"""EINV_TRANSAD / EDIR_TRANSAD on the GPU: the HIP path through the C-ABI, element by element against the NumPy model of
tests/lam_ad_ref.py (held to the dense transposes of the forward model in tests/test_lam_ad_model.py).  Bounds as tests/test_lam_gpu.py:
1e-11 of each output field's maximum in fp64, 3e-5 in fp32; the means against the largest coefficient of the wind."""
import os
import subprocess

import numpy as np
import pytest

from tests.lam_ad_common import ALL, CASES, FLAG_COMBOS, NONE, TOL, dot_identities, flag_id, lam_ad_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_CASES = {k: v for k, v in CASES.items() if "mem_space" not in v[4]}  # (in place = device tensors here)
DIVGP = dict(scders=True, vorgp=False, divgp=True, uvder=True)


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
        return (lambda a: np.ascontiguousarray(a, dtype=dt)), (lambda a: np.asarray(a))
    import torch
    return (lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")), (lambda t: t.cpu().numpy())


def run(et, what, ndlon, ndgl, M, N, memory, precision, **kw):
    to, back = mover(memory, precision)
    errs = lam_ad_case(et, ndlon, ndgl, M, N, precision=precision, to_dev=to, to_host=back, **kw)
    print(what, memory, precision, {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < TOL[precision], errs
    if precision == 4:
        assert max(errs.values()) > 1e-9  # really computed in float


@pytest.mark.parametrize("flags", FLAG_COMBOS, ids=flag_id)
def test_every_flag_combination(et, flags):
    run(et, flag_id(flags), 20, 18, 9, 8, "device", 8, flags=flags, which=("inv",))


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_parity(et, name, memory, precision):
    ndlon, ndgl, M, N, kw = GPU_CASES[name]
    run(et, name, ndlon, ndgl, M, N, memory, precision, **kw)


# two sizes of the forward suite (tests/test_lam_gpu.py), all flags
FORWARD_SIZES = {
    "smooth_384x320": (384, 320, 127, 105, {}),
    "odd_x_factor7_y_405x294": (405, 294, 134, 97, dict(split=True)),
}


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("memory", ["device", "host"])
@pytest.mark.parametrize("name", sorted(FORWARD_SIZES))
def test_forward_suite_sizes(et, name, memory, precision):
    ndlon, ndgl, M, N, kw = FORWARD_SIZES[name]
    run(et, name, ndlon, ndgl, M, N, memory, precision, **kw)


# one long x-row per x-kernel family that has an adjoint branch (tests/test_lam_gpu.py, LONG_X, names the kernels)
LONG_X = [(1540, {}), (1540, dict(EMI_FFT_MR="0")), (4100, {}), (4102, {}), (1284, {}), (1601, {})]


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("ndlon,env", LONG_X, ids=["%d%s" % (n, "".join("-" + k + v for k, v in e.items())) for n, e in LONG_X])
def test_long_x_rows(et, ndlon, env, precision, monkeypatch):
    ndgl = 40
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run(et, "long x %d" % ndlon, ndlon, ndgl, (ndlon - 1) // 2, ndgl // 2 - 1, "device", precision, nproma=3000)


@pytest.mark.parametrize("ndgl,ndlon", [(1499, 24), (5103, 20)])
def test_large_y_lengths(et, ndgl, ndlon):
    """The two largest work arrays of the forward suite in fp64.  Without flags both adjoints run (two fields fill the LDS at 5103).
    With LDDIVGP a wind field needs three columns in one work array: they fit at 1499 (3 x 47 KiB) and not at 5103; with LDVORGP it
    needs four, which fit at neither: the documented refusal."""
    M, N = ndlon // 2 - 1, (ndgl - 1) // 2
    run(et, "large y %d" % ndgl, ndlon, ndgl, M, N, "device", 8, nuv=1, nsc=2, nproma=4096, flags=NONE)
    with pytest.raises(et.TransError, match="EINV_TRANSAD: LDVORGP / LDDIVGP WITH KDGL = %d: A WIND FIELD NEEDS 4 FIELDS .* THE LDS HOLDS 160 KIB" % ndgl):
        run(et, "large y %d" % ndgl, ndlon, ndgl, M, N, "device", 8, nuv=1, nsc=2, nproma=4096, flags=ALL, which=("inv",))
    if ndgl == 1499:
        run(et, "large y %d, LDDIVGP" % ndgl, ndlon, ndgl, M, N, "device", 8, nuv=1, nsc=2, nproma=4096, flags=DIVGP, which=("inv",))
    else:
        with pytest.raises(et.TransError, match="EINV_TRANSAD: LDVORGP / LDDIVGP WITH KDGL = %d: A WIND FIELD NEEDS 3 FIELDS" % ndgl):
            run(et, "large y %d" % ndgl, ndlon, ndgl, M, N, "device", 8, nuv=1, nsc=2, nproma=4096, flags=DIVGP, which=("inv",))


@pytest.mark.parametrize("precision", [8, 4])
def test_dot_product_identities(et, precision):
    """the identities of tests/test_lam_ad_emu.py on the HIP path, all flags: below 20000 eps of the precision"""
    to, back = mover("device", precision)
    eps = np.finfo(np.float64 if precision == 8 else np.float32).eps
    rel = dot_identities(et, 20, 18, 9, 8, flags=ALL, precision=precision, to_dev=to, to_host=back)
    print("relative differences: inverse pair %.3e, direct pair %.3e (bound %.3e)" % (rel[0], rel[1], 20000 * eps))
    assert max(rel) < 20000 * eps, rel


class Guarded:
    """Arrays placed as a caller places them (in the manner of GuardedSpace, tests/common.py): each on an odd element inside a flat device
    buffer, 64 sentinel elements below it (and the odd one) and 64 above.  check(): every guard element still holds the sentinel."""
    SENTINEL = -7.25e3

    def __init__(self, dt):
        self.dt, self.recs = dt, []

    def to(self, a):
        import torch
        a = np.ascontiguousarray(a, dtype=self.dt)
        o = 64 + 1
        flat = np.full(o + a.size + 64, self.SENTINEL, dtype=self.dt)
        flat[o:o + a.size] = a.reshape(-1)
        buf = torch.from_numpy(flat).to("cuda:0")
        self.recs.append((buf, o, a.size))
        return buf[o:o + a.size].reshape(a.shape)

    def check(self):
        for k, (buf, o, n) in enumerate(self.recs):
            h = buf.cpu().numpy()
            assert np.all(h[:o] == self.SENTINEL) and np.all(h[o + n:] == self.SENTINEL), "guard band of array %d written" % k


@pytest.mark.parametrize("precision", [8, 4])
def test_guarded_placement(et, precision):
    """both adjoints, all flags, NPROMA padding, every array of the calls (inputs, outputs, means) on an odd element between guard
    bands; lam_ad_case holds the inputs to their bits and the outputs to the model"""
    gs = Guarded(np.float32 if precision == 4 else np.float64)
    errs = lam_ad_case(et, 37, 24, 12, 11, nproma=100, precision=precision, to_dev=gs.to, to_host=lambda t: t.cpu().numpy())
    gs.check()
    assert len(gs.recs) >= 12
    assert max(errs.values()) < TOL[precision], errs


def test_batches_and_phase_slots(et):
    """several batches (set_max_batch), the three-stream pipeline (EMI_TEST_PATHS=2 with calls of 256 Fourier fields and more), and the
    y-direction kernels of the adjoints reported in the Legendre slot of the phase timers, as the forward routines"""
    to, back = mover("device", 8)
    et.set_max_batch(64)
    try:
        run(et, "batches", 96, 80, 31, 26, "device", 8, nuv=40, nsc=60)
    finally:
        et.set_max_batch(0)
    os.environ["EMI_TEST_PATHS"] = "2"
    et.set_max_batch(128)
    try:
        run(et, "pipelined", 96, 80, 31, 26, "device", 8, nuv=50, nsc=160, nproma=1000)
    finally:
        et.set_max_batch(0)
        del os.environ["EMI_TEST_PATHS"]
    r = et.esetup_trans(31, 26, 80, kdlon=96, pexwn=1.0, peywn=1.0)
    sc, gp = to(np.zeros((et.etrans_inq(r, "nspec2"), 3))), to(np.zeros((1, 3, 96 * 80)))
    et.set_profile(1)
    try:
        import torch
        for fn in (et.einv_transad, et.edir_transad):
            fn(r, pspscalar=sc, pgp=gp)
            torch.cuda.synchronize()
            ms, n = et.last_phase_ms(), et.last_phase_launches()
            assert n == [0, 1, 1] and ms[0] == 0.0 and ms[1] > 0.0 and ms[2] > 0.0, (ms, n)
    finally:
        et.set_profile(0)
    et.trans_release(r)


def test_fortran_shim_lam_adjoints():
    """tests/fortran/test_shim_lam_ad.F90 on the real library: the reference's two adjoint programs through the dp and sp entry points"""
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_lam_ad"])
    p = subprocess.run([os.path.join(d, "test_shim_lam_ad")], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "FORTRAN SHIM LAM ADJOINTS OK (dp and sp)" in p.stdout, p.stdout + p.stderr
