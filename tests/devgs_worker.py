"""One task of the several-task test of DIST_* / GATH_* on device-resident fields (launched by tests/devgs_common.py::run_workers for
tests/test_devgs_emu.py and tests/test_devgs_gpu.py: argv = rank, tasks, output directory, "cpu" | "cuda").  Octahedral T21 and a
limited-area handle of 60 x 50 points, truncation 19 x 16, each in fp64 and in fp32; W-sets over gloo; "cpu" runs the CPU functional
emulator, "cuda" the real library with every task on cuda:0.  Five fields whose targets / sources alternate between task 1 and the last task: with three tasks
the middle one is source and target of nothing and passes no global array.  Each task compares the device path with the host path on
its own task count, byte for byte, checks the bytes it handed to the exchange, and saves what it got; the launching test compares the
files of 1, 2 and 3 tasks."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch.distributed as dist  # noqa: E402

import ectrans_amd as et  # noqa: E402
from tests.common import octahedral  # noqa: E402

NF, NPROMA, DEVICE = 5, 77, 1  # NPROMA cuts rows


def main():
    rank, world, outdir, where = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if where == "cuda":
        import torch
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        et.setup_trans0(kmax_resol=4, kprtrw=world, myproc=rank + 1, device=0)
    else:
        to = lambda a: np.ascontiguousarray(a)
        et._use_library_for_tests(os.path.join(ROOT, "tests", "emu", "libectrans_mi_emu.so"))
        et.setup_trans0(kmax_resol=4, kprtrw=world, myproc=rank + 1, device=None)
    back = lambda a: np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    nloen = octahedral(21)
    handles = {}
    for prec in (8, 4):  # fp32: blocks of the exchange that are no multiples of 8 bytes
        handles["o21_%d" % prec] = (et.setup_trans(21, len(nloen), nloen, precision=prec), "")
        handles["lam_%d" % prec] = (et.esetup_trans(19, 16, 50, kdlon=60, pexwn=1.0, peywn=1.0, precision=prec), "e")
    kto = np.array([1, world, 1, world, 1])
    mine = np.flatnonzero(kto == rank + 1)
    out = {}
    for h, (r, e) in handles.items():
        f = lambda n: getattr(et, e + n)
        ns2g, ngg, ng = et.trans_inq(r, "nspec2g"), et.trans_inq(r, "ngptotg"), et.trans_inq(r, "ngptot")
        rng = np.random.default_rng(41)  # the same global fields on every task
        dt = np.dtype(et.real_dtype(r))
        spg = rng.uniform(-1.0, 1.0, (ns2g, NF)).astype(dt)
        gpg = (rng.uniform(-1.0, 1.0, (NF, ngg)) + np.arange(NF)[:, None]).astype(dt)
        gl = lambda a: a if len(mine) else None  # a task that is the source of nothing passes no global array
        # ---- the host path: this task's share, the positions of its elements in a global field, the gathered images
        sp_h, gp_h = f("dist_spec")(r, gl(spg), NF, kto), f("dist_grid")(r, gl(gpg), NF, kto, kproma=NPROMA)
        pos_s = f("dist_spec")(r, gl(np.tile(np.arange(ns2g, dtype=dt)[:, None], (1, NF))), NF, kto)[:, 0].astype(np.int64)
        pos_g = f("dist_grid")(r, gl(np.tile(np.arange(ngg, dtype=dt), (NF, 1))), NF, kto, kproma=ng)[0, 0, :].astype(np.int64)
        gs_h, gg_h = f("gath_spec")(r, sp_h, NF, kto), f("gath_grid")(r, gp_h, NF, kto)
        gp_in = gp_h.copy()
        gp_in.reshape(-1, NF, NPROMA)[-1, :, ng - (gp_in.shape[0] - 1) * NPROMA:] = np.nan  # the padding of the last block is never read
        # ---- the device path: global images in host memory and in device memory
        for gsp, src in ((0, lambda a: a), (DEVICE, to)):
            sp_d = f("dist_spec")(r, None if gl(spg) is None else src(spg), NF, kto, mem_space=DEVICE, glob_space=gsp)
            gp_d = f("dist_grid")(r, None if gl(gpg) is None else src(gpg), NF, kto, kproma=NPROMA, mem_space=DEVICE, glob_space=gsp)
            assert back(sp_d).tobytes() == sp_h.tobytes() and back(gp_d).tobytes() == gp_h.tobytes(), (h, "dist", gsp)
            gs_d = f("gath_spec")(r, to(sp_h), NF, kto, mem_space=DEVICE, glob_space=gsp)
            gg_d = f("gath_grid")(r, to(gp_in), NF, kto, mem_space=DEVICE, glob_space=gsp)
            if len(mine):
                assert back(gs_d).tobytes() == gs_h.tobytes() and back(gg_d).tobytes() == gg_h.tobytes(), (h, "gath", gsp)
            else:
                assert gs_d is None and gg_d is None and gs_h is None
        # ---- a field leaves a task once, to its target: the bytes one GATH_GRID hands to the exchange
        et.set_profile(1)
        f("gath_grid")(r, to(gp_in), NF, kto, mem_space=DEVICE)
        sent = et.last_exchange()[2]
        et.set_profile(0)
        assert sent == sum(ng * dt.itemsize for t in kto if t != rank + 1), (h, sent, ng, rank)
        for k, fld in enumerate(mine):
            out["%s_gath_spec_%d" % (h, fld)], out["%s_gath_grid_%d" % (h, fld)] = np.ascontiguousarray(back(gs_d)[:, k]), back(gg_d)[k]
        out["%s_dist_spec" % h] = np.ascontiguousarray(back(sp_d).T)  # [field][local element]
        out["%s_dist_grid" % h] = np.ascontiguousarray(back(gp_d).transpose(1, 0, 2).reshape(NF, -1)[:, :ng])
        out["%s_pos_spec" % h], out["%s_pos_grid" % h] = pos_s, pos_g
    if world > 1:  # arguments that one task alone finds wrong (KSORT on task 1): every task fails, none is left waiting in the exchange
        try:
            et.edist_spec(r, gl(spg), NF, kto, ksort=[1, 2, 3, 4, 9 if rank == 0 else 5], mem_space=DEVICE)
        except et.TransError as x:
            assert ("KSORT(5) = 9 outside 1..5" if rank == 0 else "TASK 1 REFUSED ITS ARGUMENTS") in str(x), str(x)
        else:
            raise SystemExit("a bad KSORT on task 1 was not refused on task %d" % (rank + 1))
    np.savez(os.path.join(outdir, "devgs_%d_of_%d.npz" % (rank, world)), **out)
    et.trans_end()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print("DEVGS OK rank %d of %d" % (rank, world), flush=True)


if __name__ == "__main__":
    main()
