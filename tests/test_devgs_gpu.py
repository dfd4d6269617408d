"""DIST_* / GATH_* on device-resident fields, GPU tier: the device path of emi_dist_spec_m ... emi_egath_grid_m on the HIP build, torch
device tensors used in place, against the host path of the same library byte for byte (every case of tests/devgs_common.py; tests/test_devgs_emu.py
runs a selection on the emulator); the Fortran shim and the transi layer on hipMalloc'ed arrays."""
import os
import subprocess

import numpy as np
import pytest

from tests.devgs_common import FULL_CASES, check_tasks, devgs_case, forget_handles, python_case, refusal_cases, run_workers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=8, device=0)
    forget_handles()
    yield ectrans_amd
    forget_handles()
    ectrans_amd.trans_end()


@pytest.fixture(scope="module")
def dev():
    """(to_flat, back): a flat numpy buffer -> device tensor; a tensor or a view of one -> numpy of the same dtype"""
    import torch
    return (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")), (lambda t: t.cpu().numpy())


@pytest.mark.parametrize("glob_dev", [False, True], ids=["host_image", "device_image"])
@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("name,nfld,kproma,kinds", FULL_CASES)
def test_device_path_gives_the_host_path_bytes(et, dev, name, nfld, kproma, kinds, precision, glob_dev):
    bad = devgs_case(et, name, nfld, kproma, precision, glob_dev, dev, kinds)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("name", ["o21", "lam"])
def test_python_keywords(et, dev, name, precision):
    python_case(et, name, precision, to_dev=dev[0], is_dev=lambda x: hasattr(x, "is_cuda") and x.is_cuda)


def test_auto_classifies_each_array(et, dev):
    """EMI_MEM_AUTO for both arrays: a device tensor beside a host image takes the device path, two host arrays the host path"""
    import ctypes as C
    from tests.devgs_common import AUTO, handle, ok
    r, _ = handle(et, "o21", 8)
    nf, ng = 3, et.trans_inq(r, "ngptot")
    one = np.ones(nf, dtype=np.int32)
    gpg = np.random.default_rng(2).uniform(-1, 1, (nf, ng))
    loc_h, loc_d = np.zeros((1, nf, ng)), dev[0](np.zeros((1, nf, ng)))
    ip = one.ctypes.data_as(C.POINTER(C.c_int))
    ok(et, "emi_dist_grid_m", r, AUTO, C.c_void_p(gpg.ctypes.data), nf, ip, None, ng, AUTO, C.c_void_p(loc_h.ctypes.data))
    ok(et, "emi_dist_grid_m", r, AUTO, C.c_void_p(gpg.ctypes.data), nf, ip, None, ng, AUTO, C.c_void_p(loc_d.data_ptr()))
    assert loc_h.tobytes() == gpg.tobytes() == dev[1](loc_d).tobytes()
    rc = et.lib().emi_dist_grid_m(r, AUTO, C.c_void_p(dev[0](gpg).data_ptr()), nf, ip, None, ng, AUTO, C.c_void_p(loc_h.ctypes.data))
    assert rc != 0 and "THE GLOBAL ARRAY IS IN DEVICE MEMORY AND THE LOCAL ARRAY IN HOST MEMORY" in et.lib().emi_last_error().decode()


def test_chunks_of_fields(et, dev, monkeypatch):
    """a few fields per chunk (EMI_GATH_CHUNK): the global images of the chunks follow each other in the global array"""
    monkeypatch.setenv("EMI_GATH_CHUNK", str(3 * 506 * 8 + 8))
    bad = devgs_case(et, "o21", 5, 37, 8, False, dev) + devgs_case(et, "o21", 5, 37, 8, True, dev)
    assert not bad, "\n".join(bad)


def test_refusals(et):
    for what, rc, msg, text in refusal_cases(et):
        assert rc != 0 and text in msg, (what, rc, msg)


def test_tasks_give_the_one_task_bytes(tmp_path):
    """tests/devgs_worker.py on 1, 2 and 3 tasks that share cuda:0 (the exchange hook and the host collectives over gloo): at most
    three processes at a time"""
    check_tasks({n: run_workers(n, str(tmp_path), where="cuda", timeout=300) for n in (1, 2, 3)})


@pytest.mark.parametrize("target,ok_text", [("test_shim_devgs", "FORTRAN SHIM DEVGS OK"), ("test_shim_devgs_sp", "FORTRAN SHIM DEVGS OK")])
def test_fortran_shim_on_device_arrays(target, ok_text):
    """tests/fortran/test_shim_devgs.F90 in both precisions: PGP / PSPEC from hipMalloc + C_F_POINTER, PGPG / PSPECG on the host; and
    a non-contiguous section of a device array, which must abort with the routine and the extents in the ABORT_TRANS text"""
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, target])
    exe = os.path.join(d, target)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and ok_text in p.stdout, p.stdout + p.stderr
    p = subprocess.run([exe, "section"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout, p.stdout + p.stderr
    assert "ABORT_TRANS CALLED" in p.stderr and "GATH_GRID:PGP IS IN DEVICE MEMORY AND MUST BE CONTIGUOUS WITH FIRST EXTENTS 37 x 3" in p.stderr, p.stderr


def test_transi_on_device_arrays():
    """tests/transi/transi_test_devgs.c: trans_distgrid / trans_gathgrid / trans_distspec / trans_gathspec on hipMalloc'ed rgp / rspec
    give the bytes of the calls on host arrays"""
    d = os.path.join(ROOT, "ectrans_amd", "transi")
    subprocess.check_call(["make", "-s", "-C", d, "transi_test_devgs"])
    p = subprocess.run([os.path.join(d, "transi_test_devgs")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "TRANSI DEVGS OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("nranks", [2, 3])
def test_mpi_transport_carries_the_device_path(nranks):
    """tests/mpi/test_mpi_devgs.c under `mpiexec -n N`, the ranks on the one GPU: DIST_* / GATH_* on hipMalloc'ed arrays over the MPI
    transport of the exchange hook (ectrans_amd/mpi), fp64 and fp32, three fields -- blocks of odd numbers of reals, which are no
    multiples of the 16 bytes of the transforms' rows.  Skipped without MPI."""
    import shutil
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation")
    d = os.path.join(ROOT, "ectrans_amd", "mpi")
    subprocess.check_call(["make", "-s", "-C", d, "test_mpi_devgs"])
    env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([mpiexec, "-n", str(nranks), os.path.join(d, "test_mpi_devgs")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and p.stdout.count("MPI DEVGS OK") == nranks, p.stdout + p.stderr
