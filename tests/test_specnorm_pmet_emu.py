"""SPECNORM with the metric PMET on the sphere -- k_specnorm_met, emi_specnorm_met, the Python mirror and transi's rmet -- on the CPU
functional emulator (tests/emu): the same host logic and kernel as the GPU tier (tests/test_specnorm_pmet_gpu.py).  The model and
the derivation of the bound are in tests/specnorm_pmet_common.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import specnorm_pmet_common as pc

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


@pytest.fixture(scope="module", params=[8, 4])
def handle(et, request):
    r = et.setup_trans(pc.NSMAX, len(pc.NLOEN), pc.NLOEN, precision=request.param)
    assert et.trans_inq(r, "nspec2") == pc.NSPEC2G
    yield r, request.param
    et.trans_release(r)


@pytest.mark.parametrize("nf", pc.NFLDS)
def test_matches_the_model(et, handle, nf):
    r, precision = handle
    err, err_sq = pc.model_case(et, r, nf, precision)
    print("precision %d, %d fields: norm %.2e (bound %.2e), squared %.2e (bound %.2e)" % (precision, nf, err, pc.BOUND, err_sq, pc.BOUND_SQ))
    assert err <= pc.BOUND and err_sq <= pc.BOUND_SQ


def test_device_path_on_the_emulator(et, handle):
    """EMI_MEM_DEVICE: the array is used in place, the path device tensors take on a GPU"""
    r, precision = handle
    err, err_sq = pc.model_case(et, r, 65, precision, mem_space=1)
    assert err <= pc.BOUND and err_sq <= pc.BOUND_SQ


def test_unit_metrics_isolate_every_n(et, handle):
    r, precision = handle
    worst = pc.unit_metric_case(et, r, precision)
    print("precision %d: worst error over the unit metrics %.2e (bound %.2e)" % (precision, worst, pc.BOUND))
    assert worst <= pc.BOUND


@pytest.mark.parametrize("nf", [1, 65])
def test_metric_of_ones_is_specnorm(et, handle, nf):
    r, precision = handle
    err = pc.ones_case(et, r, nf, precision)
    print("precision %d, %d fields: PMET = 1 against SPECNORM %.2e (bound %.2e)" % (precision, nf, err, 2 * pc.BOUND))
    assert err <= 2 * pc.BOUND


def test_does_not_depend_on_the_other_fields(et, handle):
    """... nor on the memory: staged host arrays and arrays used in place (EMI_MEM_DEVICE) give the same bytes"""
    r, precision = handle
    staged = pc.independence_case(et, r, precision)
    in_place = pc.independence_case(et, r, precision, mem_space=1)
    assert staged.tobytes() == in_place.tobytes()


def test_refusals(et, handle):
    r, precision = handle
    T = et.TransError
    sp = np.ones((pc.NSPEC2G, 2), dtype=pc.dt(precision))
    with pytest.raises(T, match="SPECNORM: PMET TOO SMALL \\(21 elements, 22 are needed\\)"):
        et.specnorm(r, sp, pmet=np.ones(pc.NSMAX))
    with pytest.raises(T, match="SPECNORM: PMET TOO SMALL"):
        et.specnorm_met_partial(r, sp, np.ones(pc.NSMAX))
    assert np.all(np.isfinite(et.specnorm(r, sp, pmet=np.ones(pc.NSMAX + 1))))  # the shortest PMET that will do
    lam = et.esetup_trans(7, 6, 20, kdlon=24)
    with pytest.raises(T, match="SPECNORM: resolution %d is a limited-area handle \\(ESETUP_TRANS\\): this routine serves the spherical transforms only" % lam):
        et.specnorm(lam, np.ones((et.etrans_inq(lam, "nspec2"), 1)), pmet=np.ones(200))
    et.trans_release(lam)
    ll = et.setup_trans(5, 8, kdlon=16, ldll=True)
    with pytest.raises(T, match="not available on a handle set up with LDLL"):
        et.specnorm(ll, np.ones((et.trans_inq(ll, "nspec2"), 1)), pmet=np.ones(6))
    et.trans_release(ll)


def test_several_tasks_without_host_collectives():
    """a task of two with an exchange hook but no host collectives: SPECNORM with PMET says so; the per-task sums need none"""
    code = """
import ctypes as C, sys
sys.path.insert(0, %r)
import numpy as np
import ectrans_amd as et
from tests import specnorm_pmet_common as pc
L = et._use_library_for_tests(%r)
cfg = et._Init(2, 0, 0.0, 2, 1, -1, 1)
assert L.emi_init(C.byref(cfg)) == 0, L.emi_last_error()
hook = C.CFUNCTYPE(C.c_int)(lambda: 1)  # never called: no transform runs
assert L.emi_set_alltoallv(C.cast(hook, C.c_void_p), None) == 0
et._DIST.update(nproc=2)
r = et.setup_trans(pc.NSMAX, len(pc.NLOEN), pc.NLOEN)
sp = np.ones((et.trans_inq(r, "nspec2"), 2))
try:
    et.specnorm(r, sp, pmet=np.ones(pc.NSMAX + 1))
except et.TransError as e:
    assert "SPECNORM: several tasks and no host collectives" in str(e), str(e)
else:
    raise SystemExit("not refused")
assert et.specnorm_met_partial(r, sp, np.ones(pc.NSMAX + 1)).shape == (et.trans_inq(r, "nump"), 2)
print("NO COLLECTIVES OK")
""" % (ROOT, EMU)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="64"))
    assert p.returncode == 0 and "NO COLLECTIVES OK" in p.stdout, p.stdout + p.stderr


def test_tasks_give_the_one_task_bytes(tmp_path):
    """1, 2 and 3 W-set tasks over gloo (tests/specnorm_pmet_worker.py), both precisions; every task checks itself against the model"""
    results = {n: pc.run_workers(n, str(tmp_path)) for n in (1, 2, 3)}
    one = results[1][0]
    for n, parts in results.items():
        for p in parts:
            for k in ("norm_8", "norm_4"):
                assert p[k].tobytes() == one[k].tobytes(), (n, k)


def test_kvset_with_pmet_on_two_vsets(tmp_path):
    """NPRTRW x NPRTRV = 1 x 2 and 2 x 2: KVSET together with PMET, once with both V-sets holding fields (3 and 4, interleaved) and once
    with all fields in the last V-set; every task checks the norms of all fields against the model, and every task gets the same"""
    for world in (2, 4):
        parts = pc.run_workers(world, str(tmp_path), nprv=2)
        for p in parts:
            for k in ("norm_mixed_8", "norm_mixed_4", "norm_empty_8", "norm_empty_4"):
                assert p[k].tobytes() == parts[0][k].tobytes(), (world, k)
