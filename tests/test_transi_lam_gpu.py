"""Limited-area handles through the transi-style C layer on the GPU: tests/transi/transi_test_lam.c on the real library, with the
cases and comparisons of the emulator tier (tests/transi_lam_common.py, tests/test_transi_lam_emu.py); in addition every array of the
transforms from hipMalloc, and the same program under mpiexec on two and three tasks."""
import os
import shutil
import subprocess

import pytest

from tests import transi_lam_common as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11  # fp64, of each field's maximum: the GPU tier's bound (tests/test_lam_gpu.py, tests/lam_ad_common.py)


def build(target):
    d = os.path.join(ROOT, "ectrans_amd", "transi")
    subprocess.check_call(["make", "-s", "-C", d, target])
    return os.path.join(d, target)


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=4, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


@pytest.mark.parametrize("name", sorted(tc.DOMAINS))
def test_transi_lam(et, name, tmp_path):
    """host arrays: byte for byte the Python mirror's and within the models' tolerances; every array from hipMalloc (the means in host
    memory): the bytes of the host-array run"""
    exe = build("transi_test_lam")
    ref, inp = tc.make_inputs(name)
    host = tc.run_program(exe, name, str(tmp_path / "host"), inp)
    assert "invg_7" in host
    tc.same_bytes(host, tc.mirror(et, name, inp), name)
    tc.against_models(name, ref, inp, host, TOL)
    dev = tc.run_program(exe, name, str(tmp_path / "device"), inp, memory="device")
    tc.same_bytes(dev, host, name + " device")


@pytest.mark.parametrize("ntasks", [2, 3])
def test_transi_lam_several_tasks(ntasks, tmp_path):
    """the same program under mpiexec, every task on the one GPU: the gathered grid and spectral fields, the means and the norms are
    the bytes of one task.  Skipped without MPI."""
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation")
    exe, exe_mpi = build("transi_test_lam"), build("transi_test_lam_mpi")
    env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    name = "ref_20x18"
    ref, inp = tc.make_inputs(name)
    one = tc.run_program(exe, name, str(tmp_path / "one"), inp)
    many = tc.run_program(exe_mpi, name, str(tmp_path / "many"), inp, launcher=[mpiexec, "-n", str(ntasks)], env=env, marker_count=ntasks)
    skip = ("sizes", "nvalue", "mvalue", "nmyms", "invg_7")  # the local sizes and index lists of task 1; lglobal needs one task
    tc.same_bytes({k: v for k, v in many.items() if k not in skip}, one, "%d tasks" % ntasks)
