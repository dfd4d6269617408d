"""DIST_SPEC / GATH_SPEC with KVSET and DIST_GRID / GATH_GRID on sub-bands (NPRTRV > 1) on the CPU functional emulator: NPRTRW x NPRTRV
tasks over gloo, host arrays and device-resident arrays (tests/vsets_gs_common.py, tests/vsets_gs_worker.py).  2 x 3: GPU tier."""
import os
import subprocess

import pytest

from tests.vsets_gs_common import run_workers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nprw,nprv,prec", [(1, 2, 8), (2, 2, 8), (2, 2, 4)])
def test_global_fields_with_vsets(nprw, nprv, prec):
    """Layout from the inquiries, KSORT, NPROMA, a V-set without fields, chunks, host against device path, the round trip through the
    transforms against the oracle, and the refusals that every task must share."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    run_workers(nprw, nprv, "cpu", prec)
