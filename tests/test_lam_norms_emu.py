"""ESPECNORM, EGPNORM_TRANS, EDIST_SPEC, EGATH_SPEC, EDIST_GRID, EGATH_GRID -- the norms and the gather / scatter routines of the
limited-area handles -- on the CPU functional emulator (tests/emu): the same host logic and kernels as the GPU tier
(tests/test_lam_norms_gpu.py), against the NumPy restatements of tests/lam_norm_ref.py.  The bounds are derived in
tests/lam_norms_common.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lam_norm_ref as nr
from tests.lam_norms_common import (HANDLES, NFLDS, check_decomposition_invariance, egpnorm_cases, especnorm_case, independence_case,
                                     placement_case, run_workers, setup)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so")


@pytest.fixture(scope="module")
def et():
    os.environ.setdefault("OMP_NUM_THREADS", "256")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    import ectrans_amd
    ectrans_amd._use_library_for_tests(EMU)
    ectrans_amd.setup_trans0(kmax_resol=4)
    yield ectrans_amd
    ectrans_amd.trans_end()
    ectrans_amd._L = None


# ---- 1. the metric is read where the model reads it ---------------------------------------------------------------------------------------
def test_pmet_is_read_at_npme(et):
    """the model's NPME is the inquiry's, and ESPECNORM reads the weight of (m, n) at exactly NPME(m) + n, zero-based: one harmonic,
    one weight of 4 among ones doubles its norm, and the same weight one element to either side leaves it alone"""
    r, ref = setup(et, (60, 50, 19, 16), 8)
    pos = nr.npme(ref.kntmp)
    assert np.array_equal(et.etrans_inq(r, "npme"), pos)
    assert nr.pmet_size(ref.kntmp) == ref.nspec2g // 4 + 1
    for m, n in ((0, 0), (7, 3), (19, 0)):
        sp = np.zeros((ref.nspec2, 1))
        sp[ref.nesm0[m] - 1 + 4 * n + 2, 0] = 3.0  # b_r
        for shift, want in ((0, 6.0), (-1, 3.0), (1, 3.0)):
            met = np.ones(nr.pmet_size(ref.kntmp))
            if pos[m] + n + shift < met.size:
                met[pos[m] + n + shift] = 4.0
            assert et.especnorm(r, sp, met)[0] == want, (m, n, shift)
    et.trans_release(r)


# ---- 2. ESPECNORM against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("handle", HANDLES, ids=lambda h: "%dx%d_%dx%d" % h)
def test_especnorm_matches_the_model(et, handle, precision):
    """norms and per-wavenumber sums, with and without a random positive PMET, 1 / 63 / 64 / 65 / 130 fields: every local m, among them
    m = KMSMAX with KNTMP = 0 and the wavenumbers with KNTMP(m) < 4"""
    r, ref = setup(et, handle, precision)
    assert ref.kntmp[-1] == 0 or ref.M == 0
    try:
        for nf in NFLDS:
            for with_met in (False, True):
                err, bound, worst = especnorm_case(et, r, ref, nf, precision, with_met)
                print(handle, precision, nf, with_met, "norm %.2e (bound %.2e), per-m sums %.2f of their bounds" % (err, bound, worst))
                assert err <= bound and worst <= 1.0, (nf, with_met, err, bound, worst)
    finally:
        et.trans_release(r)


@pytest.mark.parametrize("precision", [8, 4])
def test_especnorm_device_path_on_the_emulator(et, precision):
    """EMI_MEM_DEVICE: the array is used in place, the path device tensors take on a GPU"""
    r, ref = setup(et, (60, 50, 19, 16), precision)
    try:
        err, bound, worst = especnorm_case(et, r, ref, 65, precision, True, mem_space=1)
        assert err <= bound and worst <= 1.0
    finally:
        et.trans_release(r)


@pytest.mark.parametrize("precision", [8, 4])
def test_especnorm_does_not_depend_on_the_other_fields(et, precision):
    r, ref = setup(et, (60, 50, 19, 16), precision)
    try:
        independence_case(et, r, ref, precision)
    finally:
        et.trans_release(r)


@pytest.mark.parametrize("mem_space", [None, 1])
def test_especnorm_of_a_placed_input(et, mem_space):
    r, ref = setup(et, (24, 20, 7, 6), 8)
    try:
        placement_case(et, r, ref, 8, mem_space=mem_space)
    finally:
        et.trans_release(r)


# ---- 3. EGPNORM_TRANS -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [8, 4])
def test_egpnorm_matches_the_model(et, precision):
    err, bound = egpnorm_cases(et, precision)
    print("EGPNORM_TRANS precision %d: average %.2e (bound %.2e)" % (precision, err, bound))
    assert err <= bound


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_six_refuse_a_gaussian_handle(et):
    T = et.TransError
    r = et.setup_trans(5, 8)
    ns2, ng = et.trans_inq(r, "nspec2"), et.trans_inq(r, "ngptot")
    sc, gp = np.zeros((ns2, 1)), np.zeros((1, 1, ng))
    no = "resolution %d is not a limited-area handle" % r
    with pytest.raises(T, match="ESPECNORM: " + no):
        et.especnorm(r, sc)
    with pytest.raises(T, match="ESPECNORM: " + no):
        et.especnorm_partial(r, sc)
    with pytest.raises(T, match="EGPNORM_TRANS: " + no):
        et.egpnorm_trans(r, gp)
    with pytest.raises(T, match="EDIST_SPEC: " + no):
        et.edist_spec(r, np.zeros((et.trans_inq(r, "nspec2g"), 1)), 1)
    with pytest.raises(T, match="EGATH_SPEC: " + no):
        et.egath_spec(r, sc, 1)
    with pytest.raises(T, match="EDIST_GRID: " + no):
        et.edist_grid(r, np.zeros((1, et.trans_inq(r, "ngptotg"))), 1)
    with pytest.raises(T, match="EGATH_GRID: " + no):
        et.egath_grid(r, gp, 1)
    et.trans_release(r)


def test_refusals_on_a_lam_handle(et):
    T = et.TransError
    r, ref = setup(et, (24, 20, 7, 6), 8)
    sp = np.ones((ref.nspec2, 2))
    need = nr.pmet_size(ref.kntmp)
    with pytest.raises(T, match="ESPECNORM: PMET TOO SMALL"):
        et.especnorm(r, sp, np.ones(need - 1))
    assert np.all(et.especnorm(r, sp, np.ones(need)) == et.especnorm(r, sp))  # the shortest PMET that will do; weights of 1
    with pytest.raises(T, match="ESPECNORM: PSPEC NOT PRESENT"):
        et.especnorm(r, None)
    with pytest.raises(T, match="EGATH_SPEC: LDZA0IP not supported"):
        et.egath_spec(r, sp, 2, ldza0ip=True)
    with pytest.raises(T, match="EGATH_SPEC: KSMAX / KMSMAX \\(truncated gather\\) not supported"):
        et.egath_spec(r, sp, 2, ksmax=5)
    with pytest.raises(T, match="EGATH_SPEC: KSMAX / KMSMAX \\(truncated gather\\) not supported"):
        et.egath_spec(r, sp, 2, kmsmax=6)
    assert np.array_equal(et.egath_spec(r, sp, 2, ksmax=6, kmsmax=7), sp)  # the handle's own: the whole spectrum
    with pytest.raises(T, match="GPNORM_TRANS_CTL:SECOND DIMENSION OF PGP TOO SMALL"):
        et.egpnorm_trans(r, np.zeros((1, 1, 480)), kfields=2)
    with pytest.raises(T, match="EDIST_SPEC: KSORT\\(1\\) = 3 outside 1..2"):
        et.edist_spec(r, np.zeros((ref.nspec2g, 2)), 2, ksort=[3, 1])
    et.trans_release(r)


def test_several_tasks_without_host_collectives():
    """a task of two with an exchange hook but no host collectives: the norms and the gather / scatter routines say so and return"""
    code = """
import ctypes as C, sys
sys.path.insert(0, %r)
import numpy as np
import ectrans_amd as et
L = et._use_library_for_tests(%r)
cfg = et._Init(2, 0, 0.0, 2, 1, -1, 1)
assert L.emi_init(C.byref(cfg)) == 0, L.emi_last_error()
hook = C.CFUNCTYPE(C.c_int)(lambda: 1)  # never called: no transform runs
assert L.emi_set_alltoallv(C.cast(hook, C.c_void_p), None) == 0
et._DIST.update(nproc=2)
r = et.esetup_trans(7, 6, 20, kdlon=24)
sp, gp = np.ones((et.etrans_inq(r, "nspec2"), 2)), np.ones((1, 2, et.etrans_inq(r, "ngptot")))
for fn, args, text in ((et.especnorm, (r, sp), "ESPECNORM: several tasks and no host collectives"),
                       (et.egpnorm_trans, (r, gp), "EGPNORM_TRANS: several tasks and no host collectives"),
                       (et.egath_spec, (r, sp, 2), "EGATH_SPEC: 2 tasks but no host collectives registered"),
                       (et.egath_grid, (r, gp, 2), "EGATH_GRID: 2 tasks but no host collectives registered"),
                       (et.edist_spec, (r, np.ones((et.etrans_inq(r, "nspec2g"), 2)), 2), "EDIST_SPEC: 2 tasks but no host collectives registered"),
                       (et.edist_grid, (r, np.ones((2, 480)), 2), "EDIST_GRID: 2 tasks but no host collectives registered")):
    try:
        fn(*args)
    except et.TransError as e:
        assert text in str(e), (text, str(e))
    else:
        raise SystemExit("not refused: " + text)
assert et.especnorm_partial(r, sp).shape == (et.etrans_inq(r, "nump"), 2)  # the per-task part needs no collective
print("NO COLLECTIVES OK")
""" % (ROOT, EMU)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="64"))
    assert p.returncode == 0 and "NO COLLECTIVES OK" in p.stdout, p.stdout + p.stderr


# ---- 5. several tasks -------------------------------------------------------------------------------------------------------------------
def test_tasks_give_the_one_task_bytes(tmp_path):
    """1, 2 and 3 tasks over gloo on 60 x 50 points, truncation 19 x 16 (tests/lam_norms_worker.py)"""
    check_decomposition_invariance({n: run_workers(n, str(tmp_path)) for n in (1, 2, 3)})
