#!/usr/bin/env python3
"""Time DIST_GRID / GATH_GRID / DIST_SPEC / GATH_SPEC on device-resident fields (emi_*_m, one task) at O640 / NSMAX 639 with 32 fields
in fp64; writes profiles/devgs_rate.txt.

Line 1: each of the four routines with the global image in device memory and in host memory.  Line 2: what a caller pays without the
device path for the same result: the local array copied between device and host plus the host routine.  Line 3: a device-to-device
hipMemcpy of the bytes of the local array, in the same run, as the bandwidth yardstick.  Every figure is the time per call, median
(minimum) over windows of 20 calls (line 2: of one call) after a warm-up, a host clock around a window that ends in a device
synchronise.  Nothing is asserted on the numbers; the results
of the timed calls are compared with the host routine's bytes.  Run on the GPU:
    python tools/devgs_rate.py [--calls 10] [--nfld 32] [--nsmax 639] [--out profiles/devgs_rate.txt]

--nprtrw W --nprtrv V (several tasks): the tool starts itself W x V times over gloo, all tasks on cuda:0, and times GATH_SPEC and GATH_GRID
of device-resident fields to a device image on task 1 (emi_gath_spec_v with the fields dealt round-robin to the V-sets; emi_gath_spec_m with
V = 1).  Tasks that share one GPU over gloo measure the packing and the bookkeeping of the routines, not a device interconnect.  The
gathered fields are compared with the bytes they were distributed from.  --lib PATH times another build of the library (an A/B run
against an older commit; with V = 1 only entry points that it has are called).  Prints one line per routine; --out appends them.
    python tools/devgs_rate.py --nprtrw 2 --nprtrv 2 --nsmax 159 [--lib other/libectrans_mi.so] [--out profiles/devgs_rate_vsets.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ectrans_amd as et  # noqa: E402

HOST, DEVICE = 0, 1


def timed(fn, calls, warm=2, inner=20):
    """ms per call: median (minimum) over `calls` windows of `inner` calls each, a host clock around a window that ends in a device
    synchronise (every call of the library waits for its stream itself)"""
    ms = []
    for i in range(warm + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(1e3 * (time.perf_counter() - t0) / inner)
    return statistics.median(ms), min(ms)


def several_tasks(a):
    """launch W x V copies of this tool (RANK in the environment marks a task) and pass on what task 1 printed"""
    import socket
    import subprocess
    world = a.nprtrw * a.nprtrv
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(s.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=dict(env, RANK=str(rank)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for rank in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=a.timeout)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for rank, (p, out) in enumerate(zip(procs, outs)):
        if p.returncode != 0:
            raise SystemExit("task %d failed:\n%s" % (rank + 1, out))
    text = "".join(l + "\n" for l in outs[0].splitlines() if l.startswith("devgs_rate"))
    print(text, end="")
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


def one_task_of_several(a):
    """GATH_SPEC and GATH_GRID of nfld device-resident fields to a device image on task 1, W x V tasks on cuda:0 over gloo"""
    import torch.distributed as dist
    rank, world, nf, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), a.nfld, a.nsmax
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if a.lib:  # another build of the library, for an A/B run
        et._L = et._bind(C.CDLL(os.path.abspath(a.lib)))
        et._EMULATOR[0] = False
    et.setup_trans0(kmax_resol=1, kprtrw=a.nprtrw, kprtrv=a.nprtrv, myproc=rank + 1, device=0)
    nloen = np.array([20 + 4 * i for i in range(n + 1)] + [20 + 4 * i for i in reversed(range(n + 1))], dtype=np.int32)
    r = et.setup_trans(n, len(nloen), nloen)
    L = et.lib()
    ns2g, ngg, ns2, ng = (et.trans_inq(r, k) for k in ("nspec2g", "ngptotg", "nspec2", "ngptot"))
    one = np.ones(nf, dtype=np.int32)
    kv = (np.arange(nf, dtype=np.int32) % a.nprtrv) + 1
    nfl = int((kv == et.trans_inq(r, "mysetv")).sum())
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    rng = np.random.default_rng(1)  # the same global fields on every task
    spg, gpg = rng.uniform(-1.0, 1.0, (nf, ns2g)), rng.uniform(-1.0, 1.0, (nf, ngg))
    dev = lambda x: torch.from_numpy(x).to("cuda:0")
    first = rank == 0
    sp_d, gp_d = torch.zeros((ns2, nfl), dtype=torch.float64, device="cuda:0"), torch.zeros((1, nf, ng), dtype=torch.float64, device="cuda:0")
    in_s, in_g = (dev(spg), dev(gpg)) if first else (None, None)
    out_s, out_g = (torch.zeros_like(in_s), torch.zeros_like(in_g)) if first else (None, None)
    if a.nprtrv > 1:
        dist_spec = lambda: L.emi_dist_spec_v(r, DEVICE, dp(in_s), nf, ip(one), ip(kv), None, DEVICE, dp(sp_d))
        gath_spec = lambda: L.emi_gath_spec_v(r, DEVICE, dp(out_s), nf, ip(one), ip(kv), DEVICE, dp(sp_d))
    else:
        dist_spec = lambda: L.emi_dist_spec_m(r, DEVICE, dp(in_s), nf, ip(one), None, DEVICE, dp(sp_d))
        gath_spec = lambda: L.emi_gath_spec_m(r, DEVICE, dp(out_s), nf, ip(one), DEVICE, dp(sp_d))
    dist_grid = lambda: L.emi_dist_grid_m(r, DEVICE, dp(in_g), nf, ip(one), None, ng, DEVICE, dp(gp_d))
    gath_grid = lambda: L.emi_gath_grid_m(r, DEVICE, dp(out_g), nf, ip(one), ng, DEVICE, dp(gp_d))

    def ok(fn):
        if fn() != 0:
            raise SystemExit(L.emi_last_error().decode())

    ok(dist_spec), ok(dist_grid)
    what = "%d x %d tasks%s" % (a.nprtrw, a.nprtrv, (", library " + a.lib) if a.lib else "")
    for name, fn, out, ref, mb in (("GATH_SPEC", gath_spec, out_s, spg, spg.nbytes / 1e6), ("GATH_GRID", gath_grid, out_g, gpg, gpg.nbytes / 1e6)):
        dist.barrier()
        med, mn = timed(lambda: ok(fn), a.calls, inner=5)
        if first:
            assert out.cpu().numpy().tobytes() == ref.tobytes(), name
            print("devgs_rate %s, %s, O%d, %d fields, fp64, device image on task 1: %8.3f ms per call (minimum %8.3f), %7.2f GB/s of the %.1f MB of the fields"
                  % (name, what, n + 1, nf, med, mn, mb / med, mb), flush=True)
    et.trans_end()
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--nfld", type=int, default=32)
    ap.add_argument("--nsmax", type=int, default=639)
    ap.add_argument("--out", default=None)
    ap.add_argument("--nprtrw", type=int, default=1)
    ap.add_argument("--nprtrv", type=int, default=1)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--timeout", type=int, default=500)
    a = ap.parse_args()
    if a.nprtrw * a.nprtrv > 1:
        return one_task_of_several(a) if "RANK" in os.environ else several_tasks(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "devgs_rate.txt")
    nf, n = a.nfld, a.nsmax
    nloen = np.array([20 + 4 * i for i in range(n + 1)] + [20 + 4 * i for i in reversed(range(n + 1))], dtype=np.int32)
    et.setup_trans0(kmax_resol=1, device=0)
    r = et.setup_trans(n, len(nloen), nloen)
    L = et.lib()
    ns2, ng = et.trans_inq(r, "nspec2g"), et.trans_inq(r, "ngptotg")
    one = np.ones(nf, dtype=np.int32)
    ip = one.ctypes.data_as(C.POINTER(C.c_int))
    rng = np.random.default_rng(1)
    dev = lambda x: torch.from_numpy(x).to("cuda:0")
    hp, dp = (lambda x: C.c_void_p(x.ctypes.data)), (lambda x: C.c_void_p(x.data_ptr()))
    lines = ["DIST_* / GATH_* on device-resident fields: O%d, NSMAX %d, %d fields, fp64, one task; %s" % (n + 1, n, nf, torch.cuda.get_device_name(0)),
             "ms per call: median (minimum) of %d windows of 20 calls (part 2: of single calls) after 2 warm-up windows, host clock around a window that ends in a device synchronise; one box, one day" % a.calls,
             "command: python tools/devgs_rate.py --calls %d --nfld %d --nsmax %d" % (a.calls, nf, n), ""]
    l1, l2, l3 = [], [], []
    for kind, nglob, extra in (("GRID", ng, (ng,)), ("SPEC", ns2, ())):
        k = kind.lower()
        glob_h = rng.uniform(-1.0, 1.0, (nf, nglob))
        loc_shape = (1, nf, ng) if kind == "GRID" else (ns2, nf)
        loc_h = np.zeros(loc_shape)
        assert getattr(L, "emi_dist_" + k)(r, hp(glob_h), nf, ip, None, *extra, hp(loc_h)) == 0  # the host routine: the reference bytes
        glob_d, loc_d, out_d, out_h, pin = dev(glob_h), dev(loc_h), torch.zeros((nf, nglob), dtype=torch.float64, device="cuda:0"), np.zeros((nf, nglob)), np.zeros(loc_shape)
        mb = loc_h.nbytes / 1e6
        for gname, gsp, gin, gout, gp in (("device image", DEVICE, glob_d, out_d, dp), ("host image", HOST, glob_h, out_h, hp)):
            loc_d.zero_()
            med, mn = timed(lambda: getattr(L, "emi_dist_%s_m" % k)(r, gsp, gp(gin), nf, ip, None, *extra, DEVICE, dp(loc_d)), a.calls)
            assert loc_d.cpu().numpy().tobytes() == loc_h.tobytes()
            l1.append("  DIST_%s, %-12s %8.3f ms (%8.3f)  %7.1f GB/s of the %.1f MB of the fields" % (kind, gname, med, mn, loc_h.nbytes / (med * 1e-3) / 1e9, mb))
            med, mn = timed(lambda: getattr(L, "emi_gath_%s_m" % k)(r, gsp, gp(gout), nf, ip, *extra, DEVICE, dp(loc_d)), a.calls)
            assert (gout.cpu().numpy() if gsp == DEVICE else gout).tobytes() == glob_h.tobytes()
            l1.append("  GATH_%s, %-12s %8.3f ms (%8.3f)  %7.1f GB/s" % (kind, gname, med, mn, loc_h.nbytes / (med * 1e-3) / 1e9))

        def today_gath():
            h = loc_d.cpu().numpy()
            getattr(L, "emi_gath_" + k)(r, hp(out_h), nf, ip, *extra, hp(h))

        def today_dist():
            getattr(L, "emi_dist_" + k)(r, hp(glob_h), nf, ip, None, *extra, hp(pin))
            loc_d.copy_(torch.from_numpy(pin))

        for nm, fn in (("GATH_" + kind, today_gath), ("DIST_" + kind, today_dist)):
            med, mn = timed(fn, max(3, a.calls // 3), warm=1, inner=1)
            l2.append("  %s: the local array between device and host + the host routine %9.3f ms (%9.3f)" % (nm, med, mn))
        cp = torch.empty_like(loc_d)
        med, mn = timed(lambda: cp.copy_(loc_d), a.calls)
        l3.append("  hipMemcpy device to device of the %s fields (%.1f MB) %8.3f ms (%8.3f)  %7.1f GB/s" % (kind, mb, med, mn, loc_h.nbytes / (med * 1e-3) / 1e9))
        del glob_d, loc_d, out_d, cp
    lines += ["1. the device path (local array in device memory, used in place)"] + l1 + ["", "2. the same result without it"] + l2 + ["", "3. yardstick"] + l3
    et.trans_end()
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
