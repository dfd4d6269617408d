"""DIST_SPEC / GATH_SPEC with KVSET and DIST_GRID / GATH_GRID on sub-bands through the Fortran drop-in, against the CPU functional
emulator: tests/fortran/test_shim_vsets_gs.F90 under mpiexec -n 2 and -n 4 (1 x 2 and 2 x 2 tasks), built in a scratch copy of
ectrans_amd/fortran whose libectrans_mi.so is the emulator build (the pattern of tests/test_specnorm_pmet_fortran_emu.py), on the
host-memory MPI transport of tests/fortran/mpi_begin_host.c.  Host arrays; tests/test_vsets_gs_fortran_gpu.py adds hipMalloc'ed ones.
Skipped without MPI."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPIEXEC = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not os.path.exists(MPIEXEC) or not os.path.exists("/opt/conda/lib/libmpi.so"):
        pytest.skip("no MPI installation")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    top = tmp_path_factory.mktemp("vsets_gs_shim")
    fdir = top / "ectrans_amd" / "fortran"
    src = os.path.join(ROOT, "ectrans_amd", "fortran")
    os.makedirs(fdir)
    for fn in os.listdir(src):
        if fn.endswith((".F90", ".h")) or fn == "Makefile":
            shutil.copy(os.path.join(src, fn), fdir / fn)
    shutil.copytree(os.path.join(src, "include"), fdir / "include")
    shutil.copytree(os.path.join(ROOT, "include"), top / "include")
    os.makedirs(top / "tests" / "fortran")
    for fn in ("test_shim_vsets_gs.F90", "mpi_begin_host.c"):
        shutil.copy(os.path.join(ROOT, "tests", "fortran", fn), top / "tests" / "fortran" / fn)
    os.symlink(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"), top / "ectrans_amd" / "libectrans_mi.so")
    subprocess.check_call(["make", "-s", "-C", str(fdir), "test_shim_vsets_gs_host"])
    return str(fdir / "test_shim_vsets_gs_host")


@pytest.mark.parametrize("ntasks", [2, 4])
def test_fortran_global_fields_with_two_vsets_on_the_emulator(exe, ntasks):
    """DIST_SPEC(KVSET) -> INV_TRANS -> GATH_GRID -> DIST_GRID -> DIR_TRANS -> GATH_SPEC(KVSET) on host arrays, and a call in which the
    tasks of V-set 1 hold no field and pass no PSPEC."""
    env = dict(os.environ, OMP_NUM_THREADS="256", LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:/opt/conda/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([MPIEXEC, "-n", str(ntasks), exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.count("FORTRAN SHIM VSETS GS OK") == ntasks, p.stdout + p.stderr
