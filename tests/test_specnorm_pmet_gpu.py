"""SPECNORM with the metric PMET on the GPU: k_specnorm_met through the C-ABI and the Python mirror, with the cases and the derived
bound of the emulator tier (tests/specnorm_pmet_common.py, tests/test_specnorm_pmet_emu.py)."""
import numpy as np
import pytest

from tests import specnorm_pmet_common as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def et():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ectrans_amd
    ectrans_amd.lib()  # fails loudly if the HIP library is missing
    ectrans_amd.setup_trans0(kmax_resol=4, device=0)
    yield ectrans_amd
    ectrans_amd.trans_end()


@pytest.fixture(scope="module", params=[8, 4])
def handle(et, request):
    r = et.setup_trans(pc.NSMAX, len(pc.NLOEN), pc.NLOEN, precision=request.param)
    assert et.trans_inq(r, "nspec2") == pc.NSPEC2G
    yield r, request.param
    et.trans_release(r)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("memory", ["device", "host"])
@pytest.mark.parametrize("nf", pc.NFLDS)
def test_matches_the_model(et, handle, nf, memory):
    r, precision = handle
    err, err_sq = pc.model_case(et, r, nf, precision, to_dev=to_dev if memory == "device" else None)
    print("precision %d, %d fields, %s: norm %.2e (bound %.2e), squared %.2e (bound %.2e)" % (precision, nf, memory, err, pc.BOUND, err_sq, pc.BOUND_SQ))
    assert err <= pc.BOUND and err_sq <= pc.BOUND_SQ


def test_unit_metrics_isolate_every_n(et, handle):
    r, precision = handle
    worst = pc.unit_metric_case(et, r, precision, to_dev=to_dev)
    print("precision %d: worst error over the unit metrics %.2e (bound %.2e)" % (precision, worst, pc.BOUND))
    assert worst <= pc.BOUND


@pytest.mark.parametrize("nf", [1, 65])
def test_metric_of_ones_is_specnorm(et, handle, nf):
    r, precision = handle
    err = pc.ones_case(et, r, nf, precision, to_dev=to_dev)
    print("precision %d, %d fields: PMET = 1 against SPECNORM %.2e (bound %.2e)" % (precision, nf, err, 2 * pc.BOUND))
    assert err <= 2 * pc.BOUND


def test_bytes_across_field_counts_positions_and_memories(et, handle):
    r, precision = handle
    dev = pc.independence_case(et, r, precision, to_dev=to_dev)
    host = pc.independence_case(et, r, precision)
    assert dev.tobytes() == host.tobytes()


def test_tasks_give_the_one_task_bytes(tmp_path):
    """tests/specnorm_pmet_worker.py on 1, 2 and 3 tasks that share cuda:0 (host collectives over gloo): at most three processes at a
    time; every task checks itself against the model"""
    results = {n: pc.run_workers(n, str(tmp_path), where="cuda", timeout=300) for n in (1, 2, 3)}
    one = results[1][0]
    for n, parts in results.items():
        for p in parts:
            for k in ("norm_8", "norm_4"):
                assert p[k].tobytes() == one[k].tobytes(), (n, k)
