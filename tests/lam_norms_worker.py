"""One task of the several-task test of the limited-area norms and gather / scatter routines (launched by tests/test_lam_norms_emu.py
and tests/test_lam_norms_gpu.py: argv = rank, tasks, output directory, "cpu" | "cuda").  60 x 50 points, truncation 19 x 16, W-sets
over gloo; "cpu" runs the CPU functional emulator, "cuda" the real library with every task on cuda:0 and the fields of the norms in
device memory.  The global inputs are the same on every task; each task works on its share and saves what it got, and the launching
test compares the files of 1, 2 and 3 tasks byte for byte."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch.distributed as dist  # noqa: E402

import ectrans_amd as et  # noqa: E402
from tests.lam_common import blocked, units  # noqa: E402
from tests.lam_norm_ref import bands, local_spec_index, pmet_size  # noqa: E402
from tests.lam_ref import LamRef  # noqa: E402

NDLON, NDGL, M, N, NF, NPROMA = 60, 50, 19, 16, 5, 77  # NPROMA cuts rows


def main():
    rank, world, outdir, where = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if where == "cuda":
        import torch
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        et.setup_trans0(kmax_resol=2, kprtrw=world, myproc=rank + 1, device=0)
    else:
        to = lambda a: np.ascontiguousarray(a)
        et._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
        et.setup_trans0(kmax_resol=2, kprtrw=world, myproc=rank + 1, device=None)
    exwn, eywn = units(NDLON, NDGL)
    r = et.esetup_trans(M, N, NDGL, kdlon=NDLON, pexwn=exwn, peywn=eywn)
    q = lambda n: et.etrans_inq(r, n)
    one = LamRef(NDLON, NDGL, M, N, exwn, eywn)
    rng = np.random.default_rng(41)  # the same global fields on every task
    spg = rng.uniform(-1.0, 1.0, (one.nspec2g, NF))  # every entry, those the inverse transform ignores included
    met = rng.uniform(0.5, 2.0, pmet_size(one.kntmp))
    gpg = rng.uniform(-1.0, 1.0, (NF, NDLON * NDGL)) + np.arange(NF)[:, None]
    # ---- this task's share
    idx = local_spec_index(one, q("myms"))
    rows = bands(NDGL, world)
    p0, p1 = rows[rank] * NDLON, rows[rank + 1] * NDLON
    assert len(idx) == q("nspec2") and p1 - p0 == q("ngptot")
    sp = np.ascontiguousarray(spg[idx])
    gp = blocked(gpg[:, p0:p1], NPROMA, np.float64)
    gp[gp == -777.0] = np.nan  # the padding of the last block is never read
    # ---- norms: the fields in device memory on the GPU tier
    norm = et.especnorm(r, to(sp))
    norm_met = et.especnorm(r, to(sp), met)
    ave, mn, mx = et.egpnorm_trans(r, to(gp), kproma=NPROMA)
    # ---- gathers: fields 0, 2, 4 to task 1, fields 1, 3 to the last task
    kto = np.array([1, world, 1, world, 1])
    mine = np.flatnonzero(kto == rank + 1)
    gs = et.egath_spec(r, sp, NF, kto)
    gg = et.egath_grid(r, gp, NF, kto)
    out = {}
    if len(mine):
        assert gs.shape == (one.nspec2g, len(mine)) and gg.shape == (len(mine), NDLON * NDGL)
        for k, f in enumerate(mine):
            out["gath_spec_%d" % f], out["gath_grid_%d" % f] = np.ascontiguousarray(gs[:, k]), gg[k]
    else:
        assert gs is None and gg is None
    # ---- distributions: the same fields from the tasks that hold them (the columns of other tasks' fields are not read), into
    # permuted slots
    ksort = np.array([3, 1, 5, 2, 4])
    ds = et.edist_spec(r, spg if len(mine) else None, NF, kto, ksort=ksort)
    dg = et.edist_grid(r, gpg if len(mine) else None, NF, kto, kproma=NPROMA, ksort=ksort)
    assert ds.shape == sp.shape and dg.shape == gp.shape
    for f in range(NF):  # field f in slot KSORT(f): this task's share, byte for byte
        assert ds[:, ksort[f] - 1].tobytes() == sp[:, f].tobytes(), f
        got, want = dg[:, ksort[f] - 1, :].reshape(-1)[:p1 - p0], gpg[f, p0:p1]
        assert got.tobytes() == want.tobytes(), f
    np.savez(os.path.join(outdir, "norms_%d_of_%d.npz" % (rank, world)), norm=norm, norm_met=norm_met, ave=ave, mn=mn, mx=mx,
             dist_spec=ds, dist_grid=dg, idx=idx, rows=np.array([p0, p1]), **out)
    et.trans_end()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("LAM NORMS OK rank %d of %d" % (rank, world), flush=True)


if __name__ == "__main__":
    main()
