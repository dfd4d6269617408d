"""DIST_* / GATH_* on device-resident fields, CPU tier: the device path of emi_dist_spec_m ... emi_egath_grid_m on the CPU functional
emulator (tests/emu), numpy arrays used in place (mem_space=EMI_MEM_DEVICE), against the host path of the same library byte for byte.
The cases are those of tests/devgs_common.py; tests/test_devgs_gpu.py runs them on the HIP build."""
import os
import subprocess

import numpy as np
import pytest

from tests.devgs_common import CASES, check_tasks, devgs_case, forget_handles, python_case, refusal_cases, run_workers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEM = (lambda a: a, lambda a: np.asarray(a))  # the flat buffer is the numpy array itself


@pytest.fixture(scope="module")
def et():
    os.environ.setdefault("OMP_NUM_THREADS", "256")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    import ectrans_amd
    ectrans_amd._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
    ectrans_amd.setup_trans0(kmax_resol=8)
    forget_handles()
    yield ectrans_amd
    forget_handles()
    ectrans_amd.trans_end()
    ectrans_amd._L = None


@pytest.mark.parametrize("glob_dev", [False, True], ids=["host_image", "device_image"])
@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("name,nfld,kproma,kinds", CASES)
def test_device_path_gives_the_host_path_bytes(et, name, nfld, kproma, kinds, precision, glob_dev):
    bad = devgs_case(et, name, nfld, kproma, precision, glob_dev, MEM, kinds)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("precision", [8, 4])
@pytest.mark.parametrize("name", ["o21", "lam"])
def test_python_keywords(et, name, precision):
    python_case(et, name, precision, to_dev=lambda a: np.ascontiguousarray(a))


def test_chunks_of_fields(et, monkeypatch):
    """a few fields per chunk (EMI_GATH_CHUNK): the global images of the chunks follow each other in the global array"""
    monkeypatch.setenv("EMI_GATH_CHUNK", str(3 * 506 * 8 + 8))
    bad = devgs_case(et, "o21", 5, 37, 8, False, MEM) + devgs_case(et, "o21", 5, 37, 8, True, MEM)
    assert not bad, "\n".join(bad)


def test_refusals(et):
    for what, rc, msg, text in refusal_cases(et):
        assert rc != 0 and text in msg, (what, rc, msg)


def test_tasks_give_the_one_task_bytes(tmp_path):
    """1, 2 and 3 tasks over gloo (tests/devgs_worker.py)"""
    check_tasks({n: run_workers(n, str(tmp_path)) for n in (1, 2, 3)})
