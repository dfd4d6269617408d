"""FPBIPERE, ETIBIHIE, Boyd's window and HORIZ_FIELD on the GPU: the HIP kernels through the C-ABI and the Python layer, with host
arrays (staged) and device tensors (in place), with the cases and checks of the emulator tier (tests/biper_common.py,
tests/test_biper_emu.py).  Spline, smoothing and blending are held to equal bytes."""
import pytest

from tests import biper_common as bc

pytestmark = pytest.mark.gpu
MEMS = ["device", "host"]
VIAS = ["cabi", "py"]


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=1, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("memory", MEMS)
@pytest.mark.parametrize("zon", [1, 0])
@pytest.mark.parametrize("case", bc.FP_CASES, ids=lambda c: "%dx%d_%dx%d" % c[:4])
def test_fpbipere_is_the_golden(et, case, zon, memory, via, esz):
    bc.golden_fpbipere(et, bc.Mem(memory, False), case, zon, esz, via)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("memory", MEMS)
@pytest.mark.parametrize("case", bc.ET_CASES, ids=lambda c: "%dx%d_%dx%d" % c[:4])
def test_etibihie_is_the_golden(et, case, memory, via, esz):
    bc.golden_etibihie(et, bc.Mem(memory, False), case, esz, via)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("memory", MEMS)
def test_boyd_window(et, memory, via, esz):
    bc.golden_boyd(et, bc.Mem(memory, False), esz, via)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("via", VIAS)
def test_horiz_field_is_the_golden(et, via, esz):
    bc.golden_horiz(et, esz, via)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("memory", MEMS)
def test_fields_do_not_depend_on_each_other(et, memory, esz):
    bc.field_independence(et, bc.Mem(memory, False), esz)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("memory", MEMS)
def test_fpbipere_600x500_matches_the_model(et, memory, esz):
    bc.model_fpbipere(et, bc.Mem(memory, False), 600, 500, 589, 489, 5, esz)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("memory", MEMS)
def test_fpbipere_packed_input_that_fills_kd1(et, memory, esz):
    """LDZON = .FALSE. with KD1 = KDLON * KDGL exactly: the last row of the re-laid field ends at the end of the array"""
    bc.model_fpbipere(et, bc.Mem(memory, False), 70, 67, 58, 64, 2, esz, zon=False, tail=0)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("memory", MEMS)
def test_refusals_leave_the_array_untouched(et, memory, esz):
    bc.refusals(et, bc.Mem(memory, False), esz)


def test_fortran_shim_biper():
    """tests/fortran/test_shim_biper_both.F90 on the real library: both precision libraries in one executable"""
    import os
    import subprocess
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ectrans_amd", "fortran")
    subprocess.check_call(["make", "-s", "-C", d, "test_shim_biper_both"])
    p = subprocess.run([os.path.join(d, "test_shim_biper_both")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "FORTRAN SHIM BIPER OK (dp and sp)" in p.stdout, p.stdout + p.stderr
