#!/usr/bin/env python3
"""Time DIST_GRID / GATH_GRID / DIST_SPEC / GATH_SPEC on device-resident fields (emi_*_m, one task) at O640 / NSMAX 639 with 32 fields
in fp64; writes profiles/devgs_rate.txt.

Line 1: each of the four routines with the global image in device memory and in host memory.  Line 2: what a caller pays without the
device path for the same result: the local array copied between device and host plus the host routine.  Line 3: a device-to-device
hipMemcpy of the bytes of the local array, in the same run, as the bandwidth yardstick.  Every figure is the time per call, median
(minimum) over windows of 20 calls (line 2: of one call) after a warm-up, a host clock around a window that ends in a device
synchronise.  Nothing is asserted on the numbers; the results
of the timed calls are compared with the host routine's bytes.  Run on the GPU:
    python tools/devgs_rate.py [--calls 10] [--nfld 32] [--nsmax 639] [--out profiles/devgs_rate.txt]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--nfld", type=int, default=32)
    ap.add_argument("--nsmax", type=int, default=639)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "devgs_rate.txt"))
    a = ap.parse_args()
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
