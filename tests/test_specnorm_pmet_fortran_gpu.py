"""SPECNORM(PMET=) of the Fortran drop-in on the GPU: tests/fortran/test_shim_specnorm_pmet.F90 on the real library, both precisions,
and the refusal that must abort with the ABORT_TRANS text (the emulator tier: tests/test_specnorm_pmet_fortran_emu.py)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fortran_shim_specnorm_pmet():
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_specnorm_pmet"])
    exe = os.path.join(d, "test_shim_specnorm_pmet")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "FORTRAN SHIM SPECNORM PMET OK (dp and sp)" in p.stdout, p.stdout + p.stderr
    p = subprocess.run([exe, "pmet"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout, p.stdout + p.stderr
    assert "ABORT_TRANS CALLED" in p.stderr and "SPECNORM: PMET TOO SMALL (21 elements, 22 are needed)" in p.stderr, p.stderr
