"""DIST_SPEC / GATH_SPEC with KVSET and DIST_GRID / GATH_GRID on sub-bands (NPRTRV > 1) on the HIP build: NPRTRW x NPRTRV tasks share
cuda:0, the exchange staged through gloo (tests/vsets_gs_common.py, tests/vsets_gs_worker.py).  2 x 3: sub-bands of unequal size and an
odd number of V-sets."""
import pytest

from tests.vsets_gs_common import run_workers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nprw,nprv,prec", [(1, 2, 8), (2, 2, 8), (2, 3, 8), (2, 2, 4)])
def test_global_fields_with_vsets_on_one_gpu(nprw, nprv, prec):
    """Layout from the inquiries, KSORT, NPROMA, a V-set without fields, chunks, host against device path (k_spec_fields, k_gridcopy,
    k_run_copy on placed device arrays), the round trip through the transforms against the oracle, and the refusals that every task
    must share."""
    run_workers(nprw, nprv, "cuda", prec)
