"""Caller-placed arrays on the CPU functional emulator (tests/emu): the arrays of a call used in place (mem_space=EMI_MEM_DEVICE on numpy
arrays, the path device tensors take on a GPU), at element offsets 0 and 1 inside sentinel-filled buffers (tests/common.py::GuardedSpace).
Checked: nothing outside the defined elements is written (guard bands, the padding of the last NPROMA block, a surplus field), inputs
come back bit for bit, NaN in the padding and the surplus field of an input reaches no output, and the results match the oracle.  The
GPU tier (tests/test_gpu_placed_arrays.py) runs the same case functions on the HIP build, whose access code for caller rows differs.
This module is also what brings the in-place path within reach of the stand-alone CPU sanitizer recipe of tests/emu/README.md."""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests.common import assert_placed, placed_arrays_case, placed_call_mode2_case, placed_gpnorm_case
from tests.test_emu_parity import HOT_A, MR_LONG, MR_SHORT, R16_ROWS, R16S_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {8: 1e-12, 4: 2e-5}  # the emulator tier's bounds (tests/test_emu_parity.py)
EMI_MEM_DEVICE = 1
MEM = (lambda a: a, lambda a: np.asarray(a))  # the flat buffer is the numpy array itself
FLAGS = dict(scders=True, vorgp=True, divgp=True, uvder=True)


@pytest.fixture(scope="module")
def et():
    os.environ.setdefault("OMP_NUM_THREADS", "256")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    import ectrans_amd
    ectrans_amd._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
    ectrans_amd.setup_trans0(kmax_resol=4)
    yield ectrans_amd
    ectrans_amd.trans_end()
    ectrans_amd._L = None


H9 = [20 + 4 * i for i in range(9)]
ODD = [19, 21, 23, 25, 27, 29, 33, 35, 37]
CONV = {"EMI_FFT_MR": "0"}  # keep rows with a 23-smooth half-length off the direct mixed-radix kernels
ROWS = {
    "H9": (H9, {}), "ODD": (ODD, {}), "MR_SHORT": (MR_SHORT, {}), "MR_LONG": (MR_LONG, {}),
    "HOT_A": (HOT_A, dict(CONV, EMI_FFT_R16S="0")), "R16_ROWS": (R16_ROWS, CONV), "R16S_ROWS": (R16S_ROWS, CONV),
    "GM": ([10244, 5136], {}),
}
# (rows, precision, NPROMA): none = whole rows, all misaligned at lead 1; 37 / 1001 cut the rows (element path); an odd NPROMA above the
# longest row changes the parity of (block, field) from one to the next: aligned, misaligned and a few cut rows in one launch
CASES = [("H9", 8, None), ("H9", 4, 37), ("H9", 8, 53), ("ODD", 8, None), ("ODD", 8, 37), ("MR_SHORT", 8, None), ("MR_SHORT", 4, 647),
         ("HOT_A", 8, None), ("HOT_A", 8, 1001), ("R16_ROWS", 8, None), ("R16_ROWS", 8, 20001), ("R16S_ROWS", 8, None),
         ("R16S_ROWS", 8, 20001), ("MR_LONG", 4, None), ("MR_LONG", 4, 1001), ("GM", 8, None), ("GM", 8, 20001), ("GM", 4, None)]
RUNS = {}  # the result of a case at one lead: the run at lead 0 is the control of the fp64 run at lead 1


def placed(et, rows, precision, nproma, lead, monkeypatch, adjoint=False):
    """one case at one lead (a few seconds of emulated kernels each): checked against the oracle, and in fp64 at lead 1 against lead 0"""
    half, env = ROWS[rows]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nuv, nsc = (2, 7) if max(half) < 1000 else (1, 1)  # short rows: ragged chunks of 2, 4 and 8 fields per workgroup

    def run(ld):
        key = (rows, precision, nproma, adjoint, ld)
        if key not in RUNS:
            RUNS[key] = placed_arrays_case(et, Oracle, MEM, 15, half + half[::-1], nuv, nsc, FLAGS, nproma, precision, ld,
                                           mem_space=EMI_MEM_DEVICE, adjoint=adjoint)
        return RUNS[key]

    what = "%s nproma %s lead %d%s" % (rows, nproma, lead, " adjoints" if adjoint else "")
    assert_placed(run(lead), precision, TOL[precision], what=what, control=run(0) if lead and precision == 8 else None)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("rows,precision,nproma", CASES)
def test_placed_arrays_match_oracle_and_stay_inside(et, rows, precision, nproma, lead, monkeypatch):
    placed(et, rows, precision, nproma, lead, monkeypatch)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("rows,precision,nproma", [("H9", 8, 37), ("H9", 4, None), ("R16_ROWS", 8, None)])
def test_placed_arrays_adjoints(et, rows, precision, nproma, lead, monkeypatch):
    placed(et, rows, precision, nproma, lead, monkeypatch, adjoint=True)


@pytest.mark.parametrize("lead", [0, 1])
def test_placed_arrays_call_mode_2(et, lead):
    errs, viol = placed_call_mode2_case(et, Oracle, MEM, lead, mem_space=EMI_MEM_DEVICE)
    print("call mode 2, lead", lead, errs, viol)
    assert not viol, viol
    assert max(errs.values()) < TOL[8], errs


def test_placed_arrays_gpnorm(et):
    err, viol = placed_gpnorm_case(et, MEM, mem_space=EMI_MEM_DEVICE)
    print("GPNORM_TRANS on placed arrays against plain ones: %.2e" % err)
    assert not viol, viol
    assert err < 1e-14
