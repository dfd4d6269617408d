"""SPECNORM(PMET=) of the Fortran drop-in, both precision libraries, against the CPU functional emulator:
tests/fortran/test_shim_specnorm_pmet.F90, built in a scratch copy of ectrans_amd/fortran whose libectrans_mi.so is the emulator
build (the shim links the library by that name and finds it beside itself).  tests/test_specnorm_pmet_fortran_gpu.py runs the same
program on the real library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    top = tmp_path_factory.mktemp("pmet_shim")
    fdir = top / "ectrans_amd" / "fortran"
    src = os.path.join(ROOT, "ectrans_amd", "fortran")
    os.makedirs(fdir)
    for fn in os.listdir(src):
        if fn.endswith((".F90", ".h")) or fn == "Makefile":
            shutil.copy(os.path.join(src, fn), fdir / fn)
    shutil.copytree(os.path.join(src, "include"), fdir / "include")
    os.makedirs(top / "tests" / "fortran")
    shutil.copy(os.path.join(ROOT, "tests", "fortran", "test_shim_specnorm_pmet.F90"), top / "tests" / "fortran" / "test_shim_specnorm_pmet.F90")
    os.symlink(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"), top / "ectrans_amd" / "libectrans_mi.so")
    subprocess.check_call(["make", "-s", "-C", str(fdir), "test_shim_specnorm_pmet"])
    return str(fdir / "test_shim_specnorm_pmet")


def _run(exe, *args):
    env = dict(os.environ, OMP_NUM_THREADS="256")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=900, env=env)


def test_fortran_specnorm_pmet_on_the_emulator(exe):
    p = _run(exe)
    print(p.stdout)
    assert p.returncode == 0 and "FORTRAN SHIM SPECNORM PMET OK (dp and sp)" in p.stdout, p.stdout + p.stderr


def test_a_short_pmet_aborts(exe):
    p = _run(exe, "pmet")
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout, p.stdout + p.stderr
    assert "ABORT_TRANS CALLED" in p.stderr and "SPECNORM: PMET TOO SMALL (21 elements, 22 are needed)" in p.stderr, p.stderr
