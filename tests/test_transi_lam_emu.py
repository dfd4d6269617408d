"""Limited-area handles through the transi-style C layer against the CPU functional emulator: tests/transi/transi_test_lam.c, built
in a scratch copy of ectrans_amd/transi whose libectrans_mi.so is the emulator build (transi links the library by that name and
finds it beside itself).  The cases and the comparisons are in tests/transi_lam_common.py; tests/test_transi_lam_gpu.py runs the
same program on the real library, and under mpiexec on several tasks (the MPI transport moves device buffers: it has no emulator tier)."""
import os
import shutil
import subprocess

import pytest

from tests import transi_lam_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so")
TOL = 1e-12  # fp64, of each field's maximum: the emulator tier's bound (tests/test_lam_emu.py); the adjoints' 1e-11 is wider


def scratch(tmp_path_factory, target):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    top = tmp_path_factory.mktemp("transi_lam")
    tdir = top / "ectrans_amd" / "transi"
    os.makedirs(tdir)
    for fn in ("Makefile", "transi_mi.c", "transi_mi.h"):
        shutil.copy(os.path.join(ROOT, "ectrans_amd", "transi", fn), tdir / fn)
    os.makedirs(top / "include")
    shutil.copy(os.path.join(ROOT, "include", "ectrans_mi.h"), top / "include" / "ectrans_mi.h")
    os.makedirs(top / "tests" / "transi")
    shutil.copy(os.path.join(ROOT, "tests", "transi", "transi_test_lam.c"), top / "tests" / "transi" / "transi_test_lam.c")
    os.symlink(EMU, top / "ectrans_amd" / "libectrans_mi.so")
    subprocess.check_call(["make", "-s", "-C", str(tdir), target])
    return str(tdir / target)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return scratch(tmp_path_factory, "transi_test_lam")


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


ENV = dict(os.environ, OMP_NUM_THREADS="256")


@pytest.mark.parametrize("name", sorted(tc.DOMAINS))
def test_transi_lam_on_the_emulator(et, exe, name, tmp_path):
    """sizes and inquiries, every transform with its means, NPROMA blocks with NaN padding, lglobal, dist / gath round trips, the norms
    and the return codes: byte for byte the Python mirror's, and within the models' tolerances"""
    ref, inp = tc.make_inputs(name)
    out = tc.run_program(exe, name, str(tmp_path / "c"), inp, env=ENV)
    assert "invg_7" in out
    tc.same_bytes(out, tc.mirror(et, name, inp), name)
    tc.against_models(name, ref, inp, out, TOL)
