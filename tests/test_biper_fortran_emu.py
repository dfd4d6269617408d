"""FPBIPERE, ETIBIHIE and HORIZ_FIELD of the Fortran drop-in against the CPU functional emulator, in the pattern of
tests/test_lam_norms_fortran_emu.py: the hosts are built in a scratch copy of ectrans_amd/fortran whose libectrans_mi.so is the emulator
build.  tests/fortran/test_shim_biper.F90 calls the routines by their generic names through the back-compat headers of one precision
(include/trans_dp, include/trans_sp), with and without the optional arguments, on the inputs of tests/golden/biper, and dumps the
arrays: the bytes equal the goldens.  tests/fortran/test_shim_biper_both.F90 links both precision libraries."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import biper_ref as R
from tests.biper_common import BOYD, DT, ET_CASES, FP_CASES, HORIZ, KSTART, TAG, boyd_name, et_name, fp_name, golden, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = {8: "test_shim_biper", 4: "test_shim_biper_sp"}


@pytest.fixture(scope="module")
def fdir(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    top = tmp_path_factory.mktemp("biper_shim")
    fdir = top / "ectrans_amd" / "fortran"
    src = os.path.join(ROOT, "ectrans_amd", "fortran")
    os.makedirs(fdir)
    for fn in os.listdir(src):
        if fn.endswith((".F90", ".h")) or fn == "Makefile":
            shutil.copy(os.path.join(src, fn), fdir / fn)
    shutil.copytree(os.path.join(src, "include"), fdir / "include")
    os.makedirs(top / "tests" / "fortran")
    for fn in ("test_shim_biper.F90", "test_shim_biper_both.F90"):
        shutil.copy(os.path.join(ROOT, "tests", "fortran", fn), top / "tests" / "fortran" / fn)
    os.symlink(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"), top / "ectrans_amd" / "libectrans_mi.so")
    subprocess.check_call(["make", "-s", "-C", str(fdir), "test_shim_biper", "test_shim_biper_sp", "test_shim_biper_both"])
    return str(fdir)


def _run(exe, *args):
    env = dict(os.environ, OMP_NUM_THREADS="256")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=env)


def write_cases(d, esz):
    """cases.txt and the raw inputs of every golden case; returns [(output file, golden output or None, shape)]"""
    lines, want = [], []

    def put(name, a):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))

    for i, case in enumerate(FP_CASES):
        X, Y, UX, UY, nf = case
        for mode in (1, 0, -1):  # LDZON=.TRUE., LDZON=.FALSE., no optional argument (= .FALSE.)
            nm = fp_name(case, 1 if mode == 1 else 0, esz)
            gin = golden(nm + "_in")
            put("f%d_%d.in" % (i, mode), gin)
            lines.append("fpbipere %d %d %d %d %d %d %d f%d_%d.in f%d_%d.out" % (X, Y, UX, UY, nf, gin.shape[1], mode, i, mode, i, mode))
            want.append(("f%d_%d.out" % (i, mode), golden(nm + "_out")))
    for i, case in enumerate(ET_CASES):
        X, Y, UX, UY, nf, bix, biy = case
        put("e%d.in" % i, golden(et_name(case, esz) + "_in"))
        lines.append("etibihie %d %d %d %d %d %d %d %d %d 0 e%d.in e%d.out" % (X, Y, UX, UY, nf, KSTART, X + 2, bix, biy, i, i))
        want.append(("e%d.out" % i, golden(et_name(case, esz) + "_out")))
    X, Y, UX, UY, nf, bw, pl = BOYD
    gin = golden(boyd_name(esz) + "_in")
    put("b.in", gin)
    lines.append("boyd %d %d %d %d %d %d %d %r 0 b.in b.out" % (X, Y, UX, UY, nf, gin.shape[1], bw, pl))
    want.append(("b.out", None))
    for kx, ky in HORIZ:
        lines.append("horiz %d %d h%dx%d.out" % (kx, ky, kx, ky))
        want.append(("h%dx%d.out" % (kx, ky), golden("horiz_field_%dx%d_%s" % (kx, ky, TAG[esz]))))
    open(os.path.join(d, "cases.txt"), "w").write("\n".join(lines) + "\n")
    return want


@pytest.mark.parametrize("esz", [8, 4])
def test_fortran_biper_gives_the_golden_bytes(fdir, tmp_path, esz):
    want = write_cases(str(tmp_path), esz)
    p = _run(os.path.join(fdir, TARGET[esz]), str(tmp_path))
    assert p.returncode == 0 and "FORTRAN SHIM BIPER DONE" in p.stdout, p.stdout + p.stderr
    for fn, g in want:
        out = np.fromfile(os.path.join(str(tmp_path), fn), dtype=DT[esz])
        if g is None:  # Boyd: what the model makes of the emulator library's own weights (erf: tests/biper_common.py)
            import ctypes
            L = ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
            X, Y, UX, UY, nf, bw, pl = BOYD
            n = 2 * bw + X - UX
            b = np.zeros(n, dtype=DT[esz])
            L.emi_boyd_window.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
            assert L.emi_boyd_window(n, pl, esz, b.ctypes.data) == 0
            gin = golden(boyd_name(esz) + "_in")
            g = R.boyd(gin, X, Y, b, b)
        assert same(out, g.reshape(-1)), fn


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("line,text", [
    ("fpbipere 14 10 9 7 2 145 7 x.in x.out", "FPBIPERE: KDADD = 1 NOT SUPPORTED"),
    ("boyd 24 22 20 18 2 1088 3 2.5 2 x.in x.out", "FPBIPERE: Boyd periodization requires PLBOYD argument"),
    ("etibihie 30 28 25 21 2 -1 32 1 1 1 x.in x.out", "ETIBIHIE: KDADD = 1 NOT SUPPORTED"),
    ("etibihie 30 28 25 21 2 -1 32 0 1 0 x.in x.out", "ETIBIHIE: LDBIX = .FALSE. REQUIRES KDLUX = KDLON"),
])
def test_fortran_biper_refusals_abort(fdir, tmp_path, line, text, esz):
    np.zeros(4096, dtype=DT[esz]).tofile(os.path.join(str(tmp_path), "x.in"))
    open(os.path.join(str(tmp_path), "cases.txt"), "w").write(line + "\n")
    p = _run(os.path.join(fdir, TARGET[esz]), str(tmp_path))
    assert p.returncode != 0 and "NOT REFUSED" not in p.stdout, p.stdout + p.stderr
    assert "ABORT_TRANS CALLED" in p.stderr and text in p.stderr, p.stderr


def test_fortran_biper_both_precisions_in_one_executable(fdir):
    p = _run(os.path.join(fdir, "test_shim_biper_both"))
    assert p.returncode == 0 and "FORTRAN SHIM BIPER OK (dp and sp)" in p.stdout, p.stdout + p.stderr
