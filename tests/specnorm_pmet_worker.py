"""One task of the several-task tests of SPECNORM with PMET (launched by tests/specnorm_pmet_common.run_workers: argv = rank, tasks,
output directory, "cpu" | "cuda", NPRTRV).  T21 on the 32-row grid of tests/specnorm_pmet_common.py, tasks over gloo; "cpu" runs the
CPU functional emulator, "cuda" the real library with every task on cuda:0 and the fields in device memory.  The global fields are
the same on every task; each task passes its wavenumbers (and, with V-sets, the fields of its V-set) and saves the norms it got: the
launching test compares the files of 1, 2 and 3 tasks byte for byte, and the V-set run against the model."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch.distributed as dist  # noqa: E402

import ectrans_amd as et  # noqa: E402
from tests import specnorm_pmet_common as pc  # noqa: E402

NF = 7


def main():
    rank, world, outdir, where, nprv = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5])
    nprw = world // nprv
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    kw = dict(kmax_resol=2, kprtrw=nprw, myproc=rank + 1)
    if nprv > 1:
        kw["kprtrv"] = nprv
    if where == "cuda":
        import torch
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        et.setup_trans0(device=0, **kw)
    else:
        to = lambda a: np.ascontiguousarray(a)
        et._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
        et.setup_trans0(device=None, **kw)
    out = {}
    for precision in (8, 4):
        r = et.setup_trans(pc.NSMAX, len(pc.NLOEN), pc.NLOEN, precision=precision)
        spg, met = pc.fields(NF, precision, seed=41), pc.metric(precision)  # the same global fields on every task
        idx = pc.local_index(et.trans_inq(r, "myms"))
        assert len(idx) == et.trans_inq(r, "nspec2")
        want = np.sqrt(pc.model_sq(spg.astype(np.float64), met.astype(np.float64)))
        if nprv == 1:
            gots = {"": et.specnorm(r, to(spg[idx]), pmet=met)}
        else:
            # "mixed": both V-sets hold fields, unevenly (3 and 4) and interleaved, so the position of a field in its V-set differs from
            # its position in KVSET; "empty": every field in the last V-set, the others take part with no field
            gots = {}
            for tag, kv in (("_mixed", pc.KVSET_MIXED), ("_empty", [nprv] * NF)):
                kvset = np.array(kv, dtype=np.int32)
                assert len(kvset) == NF and kvset.max() <= nprv
                mine = np.flatnonzero(kvset == et.trans_inq(r, "mysetv"))
                loc = to(spg[idx][:, mine]) if len(mine) else np.zeros((len(idx), 0), dtype=pc.dt(precision))
                gots[tag] = et.specnorm(r, loc, kvset=kvset, pmet=met)
                own = et.specnorm(r, loc, pmet=met)  # without KVSET: the norms of this V-set's fields
                assert own.tobytes() == gots[tag][mine].tobytes()
        for tag, got in gots.items():
            err = pc.rel(got, want)
            print("rank %d of %d, NPRTRV %d%s, precision %d: error %.2e (bound %.2e)" % (rank, world, nprv, tag, precision, err, pc.BOUND), flush=True)
            assert got.shape == (NF,) and err <= pc.BOUND, (tag, err, pc.BOUND)
            out["norm%s_%d" % (tag, precision)] = got
        et.trans_release(r)
    np.savez(os.path.join(outdir, "pmet_%d_of_%d_v%d.npz" % (rank, world, nprv)), **out)
    et.trans_end()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("SPECNORM PMET OK rank %d of %d" % (rank, world), flush=True)


if __name__ == "__main__":
    main()
