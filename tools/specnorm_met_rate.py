#!/usr/bin/env python3
"""Time SPECNORM with the metric PMET (k_specnorm_met) and, in the same run, the unchanged unweighted SPECNORM (k_specnorm) on
device-resident spectra of TCo1279 with 137 fields, fp64, beside a torch.sum over the same tensor as the read-rate yardstick; writes
profiles/specnorm_met.txt.

The timed region is synchronised and runs from the call's start to the returned norms (allocation of the result, upload of PMET,
kernel, copy back, the sum over m on the host); the kernels alone are timed in further calls by the library's events around the
launch (emi_set_profile(1), emi_specnorm_last_ms).  Median of the calls after a warm-up.  GB/s = bytes of the spectral array / median
time, quoted against the HBM figures of the MI355X (8.0 TB/s peak, about 6.3 TB/s achievable by a streaming copy).  Run on the GPU:
    python tools/specnorm_met_rate.py [--calls 20] [--nfld 137] [--nsmax 1279] [--out profiles/specnorm_met.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ectrans_amd as et  # noqa: E402

HBM_PEAK, HBM_STREAM = 8000.0, 6300.0  # GB/s


def median_ms(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--nfld", type=int, default=137)
    ap.add_argument("--nsmax", type=int, default=1279)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specnorm_met.txt"))
    a = ap.parse_args()
    N = a.nsmax
    half = [20 + 4 * i for i in range(N + 1)]  # the octahedral grid TCo<N>
    nloen = np.array(half + half[::-1], dtype=np.int32)
    et.setup_trans0(kmax_resol=2, device=0)
    r = et.setup_trans(N, len(nloen), nloen, precision=8)
    ns2 = et.trans_inq(r, "nspec2")
    g = torch.Generator(device="cuda:0").manual_seed(1)
    sp = torch.rand((ns2, a.nfld), dtype=torch.float64, device="cuda:0", generator=g) - 0.5
    met = np.random.default_rng(2).uniform(0.5, 2.0, N + 1)
    nbytes = sp.numel() * sp.element_size()
    t_met = median_ms(lambda: et.specnorm(r, sp, pmet=met), a.calls)
    t_old = median_ms(lambda: et.specnorm(r, sp), a.calls)
    t_all = median_ms(lambda: torch.sum(sp).item(), a.calls)
    # the kernels alone: events on the null stream around the launch (emi_set_profile(1), emi_specnorm_last_ms)
    et.set_profile(1)

    def kernel_ms(fn):
        out = []
        for _ in range(a.calls + 3):
            fn()
            out.append(et.specnorm_last_ms())
        return statistics.median(out[3:]), min(out[3:])
    k_met = kernel_ms(lambda: et.specnorm(r, sp, pmet=met))
    k_old = kernel_ms(lambda: et.specnorm(r, sp))
    et.set_profile(0)
    ones = et.specnorm(r, sp, pmet=np.ones(N + 1))
    dev = float(np.max(np.abs(ones / et.specnorm(r, sp) - 1.0)))
    gbs = lambda t: nbytes / (t[0] * 1e-3) / 1e9
    pct = lambda t: "%4.1f %% of the HBM peak, %4.1f %% of a streaming copy" % (100 * gbs(t) / HBM_PEAK, 100 * gbs(t) / HBM_STREAM)
    lines = ["SPECNORM on device-resident spectra, TCo%d (NSMAX %d, %d rows), %d fields, fp64; %s" % (N, N, len(nloen), a.nfld, torch.cuda.get_device_name(0)),
             "median (minimum) of %d synchronised calls after 3 warm-up calls; GB/s = bytes of the spectral array / median time" % a.calls,
             "HBM of the MI355X: %.1f TB/s peak, about %.1f TB/s achieved by a streaming copy" % (HBM_PEAK / 1e3, HBM_STREAM / 1e3), "",
             "nspec2 = %d, %.1f MB read per call" % (ns2, nbytes / 1e6),
             "  SPECNORM with PMET (k_specnorm_met)  %8.3f ms (%8.3f)  %7.1f GB/s  %s" % (t_met[0], t_met[1], gbs(t_met), pct(t_met)),
             "  SPECNORM (k_specnorm, unchanged)     %8.3f ms (%8.3f)  %7.1f GB/s  %s" % (t_old[0], t_old[1], gbs(t_old), pct(t_old)),
             "  torch.sum, whole tensor              %8.3f ms (%8.3f)  %7.1f GB/s  %s   (the yardstick)" % (t_all[0], t_all[1], gbs(t_all), pct(t_all)),
             "  the weighted call takes %.2f of the unweighted call's time and reaches %.0f %% of the yardstick's rate" % (
                 t_met[0] / t_old[0], 100.0 * t_all[0] / t_met[0]),
             "the kernels alone (events around the launch):",
             "  k_specnorm_met                       %8.3f ms (%8.3f)  %7.1f GB/s  %s" % (k_met[0], k_met[1], gbs(k_met), pct(k_met)),
             "  k_specnorm                           %8.3f ms (%8.3f)  %7.1f GB/s  %s" % (k_old[0], k_old[1], gbs(k_old), pct(k_old)),
             "  PMET = 1 against the unweighted norms: largest relative difference %.2e" % dev, ""]
    et.trans_release(r)
    et.trans_end()
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
