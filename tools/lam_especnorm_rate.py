#!/usr/bin/env python3
"""Time ESPECNORM on device-resident spectra of the 1536 x 1440 limited-area handle (truncation 767 x 719) with 137 fields, fp64 and
fp32, beside a torch.sum over the same tensor as the read-rate yardstick; writes profiles/lam_especnorm.txt.

The timed region of ESPECNORM is synchronised and runs from the call's start to the returned norms (allocation of the result, upload
of PMET where there is one, kernel, copy back).  Median of the calls after a warm-up.  Run on the GPU:
    python tools/lam_especnorm_rate.py [--calls 20] [--nfld 137] [--out profiles/lam_especnorm.txt]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lam_especnorm.txt"))
    a = ap.parse_args()
    ndlon, ndgl, M, N = 1536, 1440, 767, 719
    et.setup_trans0(kmax_resol=2, device=0)
    lines = ["ESPECNORM on device-resident spectra, %d x %d points, truncation %d x %d, %d fields; %s" %
             (ndlon, ndgl, M, N, a.nfld, torch.cuda.get_device_name(0)),
             "median (minimum) of %d synchronised calls after 3 warm-up calls; GB/s = bytes of the spectral array / median time" % a.calls, ""]
    for prec, dt in ((8, torch.float64), (4, torch.float32)):
        r = et.esetup_trans(M, N, ndgl, kdlon=ndlon, precision=prec)
        ns2 = et.etrans_inq(r, "nspec2")
        g = torch.Generator(device="cuda:0").manual_seed(1)
        sp = torch.rand((ns2, a.nfld), dtype=dt, device="cuda:0", generator=g) - 0.5
        met = np.random.default_rng(2).uniform(0.5, 2.0, ns2 // 4 + 1).astype("float64" if prec == 8 else "float32")
        nbytes = sp.numel() * sp.element_size()
        t_norm = median_ms(lambda: et.especnorm(r, sp), a.calls)
        t_met = median_ms(lambda: et.especnorm(r, sp, met), a.calls)
        t_sum = median_ms(lambda: torch.sum(sp, dim=0, dtype=torch.float64).cpu(), a.calls)
        t_all = median_ms(lambda: torch.sum(sp).item(), a.calls)
        gbs = lambda t: nbytes / (t[0] * 1e-3) / 1e9
        lines += ["fp%d: nspec2 = %d, %.1f MB read per call" % (8 * prec, ns2, nbytes / 1e6),
                  "  ESPECNORM                 %8.3f ms (%8.3f)  %7.1f GB/s" % (t_norm[0], t_norm[1], gbs(t_norm)),
                  "  ESPECNORM with PMET       %8.3f ms (%8.3f)  %7.1f GB/s" % (t_met[0], t_met[1], gbs(t_met)),
                  "  torch.sum, whole tensor   %8.3f ms (%8.3f)  %7.1f GB/s   (the yardstick)" % (t_all[0], t_all[1], gbs(t_all)),
                  "  torch.sum per field, f64  %8.3f ms (%8.3f)  %7.1f GB/s" % (t_sum[0], t_sum[1], gbs(t_sum)),
                  "  ESPECNORM reaches %.0f %% of the yardstick's rate" % (100.0 * t_all[0] / t_norm[0]), ""]
        et.trans_release(r)
    et.trans_end()
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
