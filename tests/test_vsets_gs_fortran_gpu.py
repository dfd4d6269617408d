"""DIST_SPEC / GATH_SPEC with KVSET and DIST_GRID / GATH_GRID on sub-bands through the Fortran drop-in on the HIP build:
tests/fortran/test_shim_vsets_gs.F90 under mpiexec -n 2 and -n 4 (1 x 2 and 2 x 2 tasks on one GPU, the MPI transport of
ectrans_amd/mpi), built and launched as tests/test_gpu_shims.py runs test_shim_vsets.F90.  Host arrays and hipMalloc'ed PSPEC / PGP.
Skipped without MPI."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ntasks", [2, 4])
def test_fortran_global_fields_with_two_vsets(ntasks):
    """DIST_SPEC(KVSET) -> INV_TRANS -> GATH_GRID -> DIST_GRID -> DIR_TRANS -> GATH_SPEC(KVSET) between different source and target
    tasks, on host arrays and again on device-resident PSPEC / PGP, and a call in which the tasks of V-set 1 hold no field."""
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(mpiexec) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation")
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_vsets_gs"])
    env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([mpiexec, "-n", str(ntasks), os.path.join(d, "test_shim_vsets_gs"), "device"], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.count("FORTRAN SHIM VSETS GS OK") == ntasks, p.stdout + p.stderr
