"""ESPECNORM, EGPNORM_TRANS, EDIST_SPEC, EGATH_SPEC, EDIST_GRID and EGATH_GRID of the Fortran drop-in, both precision libraries, against
the CPU functional emulator: tests/fortran/test_shim_lam_norms.F90, built in a scratch copy of ectrans_amd/fortran whose libectrans_mi.so
is the emulator build (the pattern of tests/test_lam_fortran_emu.py).  tests/test_lam_norms_gpu.py runs the same program on the real
library.  Also: the entry points the three Fortran libraries export and the generated headers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = ["especnorm", "egpnorm_trans", "edist_spec", "egath_spec", "edist_grid", "egath_grid"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    top = tmp_path_factory.mktemp("lam_norms_shim")
    fdir = top / "ectrans_amd" / "fortran"
    src = os.path.join(ROOT, "ectrans_amd", "fortran")
    os.makedirs(fdir)
    for fn in os.listdir(src):
        if fn.endswith((".F90", ".h")) or fn == "Makefile":
            shutil.copy(os.path.join(src, fn), fdir / fn)
    shutil.copytree(os.path.join(src, "include"), fdir / "include")
    os.makedirs(top / "tests" / "fortran")
    shutil.copy(os.path.join(ROOT, "tests", "fortran", "test_shim_lam_norms.F90"), top / "tests" / "fortran" / "test_shim_lam_norms.F90")
    os.symlink(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"), top / "ectrans_amd" / "libectrans_mi.so")
    subprocess.check_call(["make", "-s", "-C", str(fdir), "test_shim_lam_norms"])
    return str(fdir / "test_shim_lam_norms")


def _run(exe, *args):
    env = dict(os.environ, OMP_NUM_THREADS="256")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=900, env=env)


def test_fortran_lam_norms_on_the_emulator(exe):
    p = _run(exe)
    print(p.stdout)
    assert p.returncode == 0 and "FORTRAN SHIM LAM NORMS OK (dp and sp)" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("arg,text", [
    ("ldza0ip", "EGATH_SPEC: LDZA0IP not supported"),
    ("ksmax", "EGATH_SPEC: KSMAX / KMSMAX (truncated gather) not supported"),
    ("pmet", "ESPECNORM: PMET TOO SMALL"),
    ("kvset", "ESPECNORM: FIRST DIMENSION OF PSPEC TOO SMALL"),
])
def test_fortran_lam_norms_refusals_abort(exe, arg, text):
    p = _run(exe, arg)
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout, p.stdout + p.stderr
    assert "ABORT_TRANS CALLED" in p.stderr and text in p.stderr, p.stderr


def test_fortran_libraries_export_the_six():
    """NAME_dp_ in libectrans_mi_f.so, NAME_sp_ in libectrans_mi_f_sp.so, the unsuffixed alias in each, none of them in the common library"""
    d = os.path.join(ROOT, "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "libectrans_mi_f_common.so", "libectrans_mi_f.so", "libectrans_mi_f_sp.so"])

    def dynsyms(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(d, lib)], capture_output=True, text=True, check=True).stdout
        return {l.split()[-1] for l in out.splitlines() if l.strip()}

    dp, sp, cm = dynsyms("libectrans_mi_f.so"), dynsyms("libectrans_mi_f_sp.so"), dynsyms("libectrans_mi_f_common.so")
    for n in SIX:
        assert n + "_dp_" in dp and n + "_sp_" in sp, n
        assert n + "_sp_" not in dp and n + "_dp_" not in sp, n
        assert n + "_" in dp and n + "_" in sp, "unsuffixed alias of %s missing" % n
        assert n + "_" not in cm and n + "_dp_" not in cm and n + "_sp_" not in cm, n


def test_generated_headers_of_the_six():
    inc = os.path.join(ROOT, "ectrans_amd", "fortran", "include")
    for n in SIX:
        for tag in ("dp", "sp"):
            assert ("SUBROUTINE %s_%s(" % (n.upper(), tag.upper())) in open(os.path.join(inc, "%s_%s.h" % (n, tag))).read(), (n, tag)
            txt = open(os.path.join(inc, "trans_" + tag, n + ".h")).read()
            assert "#define %s %s_%s" % (n.upper(), n.upper(), tag.upper()) in txt and '#include "../%s_%s.h"' % (n, tag) in txt, (n, tag)
    mod = open(os.path.join(ROOT, "ectrans_amd", "fortran", "ectrans_mi_interfaces.F90")).read()
    assert all("SUBROUTINE %s(" % n.upper() in mod for n in SIX)
