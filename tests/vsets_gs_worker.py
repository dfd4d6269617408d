"""One task of the tests of DIST_* / GATH_* with V-sets (tests/vsets_gs_common.py::run_workers for tests/test_vsets_gs_emu.py and
tests/test_vsets_gs_gpu.py): NPRTRW x NPRTRV tasks over gloo, EMI_TEST_DEVICE=cpu on the CPU functional emulator, cuda on the HIP build
with every task on cuda:0.  Octahedral T21 (nspec2g = 506: a partial element tile; spectral and grid fields, the transform round trip)
and T63 on the 96 x 192 full grid (whole tiles; spectral fields only).  EMI_TEST_CASES picks the cases (default: all of
vsets_gs_common.ALL_CASES)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch.distributed as dist  # noqa: E402
import faulthandler  # noqa: E402
faulthandler.dump_traceback_later(int(os.environ.get("EMI_TEST_WATCHDOG", "840")), exit=True)  # a deadlock between the tasks shows its stack

import ectrans_amd as et  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402
from tests.common import octahedral  # noqa: E402
from tests.vsets_gs_common import ALL_CASES, run_all  # noqa: E402


def main():
    rank, world, nprv = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["EMI_TEST_NPRTRV"])
    prec = int(os.environ.get("EMI_TEST_PRECISION", "8"))
    cases = [c for c in os.environ.get("EMI_TEST_CASES", "").split(",") if c] or list(ALL_CASES)
    nprw = world // nprv
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if os.environ.get("EMI_TEST_DEVICE", "cpu") == "cuda":
        import torch
        dev_mem = (lambda a: torch.from_numpy(a).to("cuda:0"), lambda t: t.cpu().numpy())
        et.setup_trans0(kmax_resol=2, kprtrw=nprw, kprtrv=nprv, myproc=rank + 1, device=0)
    else:
        dev_mem = (lambda a: a, lambda a: np.asarray(a))
        et._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
        et.setup_trans0(kmax_resol=2, kprtrw=nprw, kprtrv=nprv, myproc=rank + 1, device=None)
    nloen = octahedral(21)
    o21 = et.setup_trans(21, len(nloen), nloen, precision=prec)
    assert (et.trans_inq(o21, "nproc"), et.trans_inq(o21, "nprtrw"), et.trans_inq(o21, "nprtrv"), et.trans_inq(o21, "myproc")) == (world, nprw, nprv, rank + 1)
    bad = run_all(et, o21, dev_mem, nprv, cases, "o21", Oracle(21, nloen) if "transform" in cases else None)
    if prec == 8:
        f63 = et.setup_trans(63, 96, None, kdlon=192, precision=prec)
        bad += run_all(et, f63, dev_mem, nprv, [c for c in cases if c in ("layout", "ksort", "chunk")], "f63")
    for b in bad:
        print("VIOLATION rank %d: %s" % (rank, b), flush=True)
    et.trans_end()
    dist.barrier()
    dist.destroy_process_group()
    if bad:
        raise SystemExit(1)
    print("VSETS GS OK rank %d of %d" % (rank, world), flush=True)


if __name__ == "__main__":
    main()
