"""FPBIPERE, ETIBIHIE, Boyd's window and HORIZ_FIELD on the CPU functional emulator (tests/emu): the host logic and the kernels of the
GPU tier (tests/test_biper_gpu.py) with the cases and checks of tests/biper_common.py."""
import os
import subprocess

import pytest

from tests import biper_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so")
MEMS = ["device", "host"]
VIAS = ["cabi", "py"]


@pytest.fixture(scope="module")
def et():
    os.environ.setdefault("OMP_NUM_THREADS", "256")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    import ectrans_amd
    ectrans_amd._use_library_for_tests(EMU)
    ectrans_amd.setup_trans0(kmax_resol=1)
    yield ectrans_amd
    ectrans_amd.trans_end()
    ectrans_amd._L = None


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("memory", MEMS)
@pytest.mark.parametrize("zon", [1, 0])
@pytest.mark.parametrize("case", bc.FP_CASES, ids=lambda c: "%dx%d_%dx%d" % c[:4])
def test_fpbipere_is_the_golden(et, case, zon, memory, via, esz):
    bc.golden_fpbipere(et, bc.Mem(memory, True), case, zon, esz, via)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("memory", MEMS)
@pytest.mark.parametrize("case", bc.ET_CASES, ids=lambda c: "%dx%d_%dx%d" % c[:4])
def test_etibihie_is_the_golden(et, case, memory, via, esz):
    bc.golden_etibihie(et, bc.Mem(memory, True), case, esz, via)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("memory", MEMS)
def test_boyd_window(et, memory, via, esz):
    bc.golden_boyd(et, bc.Mem(memory, True), esz, via)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("via", VIAS)
def test_horiz_field_is_the_golden(et, via, esz):
    bc.golden_horiz(et, esz, via)


@pytest.mark.parametrize("esz", [8, 4])
def test_fields_do_not_depend_on_each_other(et, esz):
    bc.field_independence(et, bc.Mem("device", True), esz)


@pytest.mark.parametrize("esz", [8, 4])
def test_fpbipere_600x500_matches_the_model(et, esz):
    bc.model_fpbipere(et, bc.Mem("device", True), 600, 500, 589, 489, 5, esz)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("memory", MEMS)
def test_fpbipere_packed_input_that_fills_kd1(et, memory, esz):
    """LDZON = .FALSE. with KD1 = KDLON * KDGL exactly: the last row of the re-laid field ends at the end of the array"""
    bc.model_fpbipere(et, bc.Mem(memory, True), 70, 67, 58, 64, 2, esz, zon=False, tail=0)


@pytest.mark.parametrize("esz", [8, 4])
@pytest.mark.parametrize("memory", MEMS)
def test_refusals_leave_the_array_untouched(et, memory, esz):
    bc.refusals(et, bc.Mem(memory, True), esz)
