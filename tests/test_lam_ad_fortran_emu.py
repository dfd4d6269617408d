"""EINV_TRANSAD / EDIR_TRANSAD of the Fortran drop-in, both precision libraries, against the CPU functional emulator:
tests/fortran/test_shim_lam_ad.F90 -- the reference's two limited-area adjoint programs restated through the Fortran dummy lists --
built in a scratch copy of ectrans_amd/fortran whose libectrans_mi.so is the emulator build (the shim links the library by that name and
finds it beside itself).  tests/test_lam_ad_gpu.py runs the same program on the real library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    top = tmp_path_factory.mktemp("lam_ad_shim")
    fdir = top / "ectrans_amd" / "fortran"
    src = os.path.join(ROOT, "ectrans_amd", "fortran")
    os.makedirs(fdir)
    for fn in os.listdir(src):
        if fn.endswith((".F90", ".h")) or fn == "Makefile":
            shutil.copy(os.path.join(src, fn), fdir / fn)
    shutil.copytree(os.path.join(src, "include"), fdir / "include")
    os.makedirs(top / "tests" / "fortran")
    shutil.copy(os.path.join(ROOT, "tests", "fortran", "test_shim_lam_ad.F90"), top / "tests" / "fortran" / "test_shim_lam_ad.F90")
    os.symlink(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"), top / "ectrans_amd" / "libectrans_mi.so")
    subprocess.check_call(["make", "-s", "-C", str(fdir), "test_shim_lam_ad"])
    return str(fdir / "test_shim_lam_ad")


def test_fortran_lam_adjoints_on_the_emulator(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="256"))
    print(p.stdout)
    assert p.returncode == 0 and "FORTRAN SHIM LAM ADJOINTS OK (dp and sp)" in p.stdout, p.stdout + p.stderr
