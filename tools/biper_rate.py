#!/usr/bin/env python3
"""Time FPBIPERE(LDZON=.TRUE.) on device-resident fields of a 1536 x 1440 domain (C+I 1525 x 1429) with 64 fields, fp64 and fp32;
writes profiles/biper_rate.txt.

The call is timed with events on the null stream, the stream it runs on: median of the calls after a warm-up.  One further call
with the library's event timers on gives the share of each kernel.  "Must touch" counts every element a kernel has to read or write
once: the four values per line and the extension written by the two spline passes, and per smoothing half-pass the band with its
one-point halo read, the band written to the band buffer, and the band read and written again by the copy back.  For comparison the
same fields as a host array through the same call, which stages the whole array to the device and back (the library's own staging),
and the difference of the two.  Run on the GPU:
    python tools/biper_rate.py [--calls 20] [--nfld 64] [--out profiles/biper_rate.txt]"""
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

X, Y, UX, UY = 1536, 1440, 1525, 1429


def must_touch(nf):
    """elements per kernel: spline x, spline y, smoothing, band copy"""
    ex, ey = X - UX, Y - UY
    sx = (4 + ex) * UY * nf
    sy = (4 + ey) * X * nf
    sm = cp = 0
    for l in range(1, (max(ex, ey) + 1) // 2 + 1):
        for nx, ny in ((ex - 2 * l + 2, Y), (X, ey - 2 * l + 2)):
            if nx > 0 and ny > 0:
                sm += ((nx + 2) * (ny + 2) + nx * ny) * nf
                cp += 2 * nx * ny * nf
    return [sx, sy, sm, cp]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--nfld", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "biper_rate.txt"))
    a = ap.parse_args()
    nf = a.nfld
    et.setup_trans0(kmax_resol=1, device=0)
    lines = ["FPBIPERE(LDZON=.TRUE.) on device-resident fields: %d x %d points, C+I %d x %d, %d fields; %s" % (X, Y, UX, UY, nf, torch.cuda.get_device_name(0)),
             "median (minimum) of %d calls after 3 warm-up calls, timed with events on the null stream; one box, one day" % a.calls,
             "command: python tools/biper_rate.py --calls %d --nfld %d" % (a.calls, nf), ""]
    names = ["k_biper_spline_x", "k_biper_spline_y", "k_biper_smooth", "k_biper_copy"]
    for esz, dt in ((8, torch.float64), (4, torch.float32)):
        ci = torch.rand((nf, UY, UX), dtype=dt, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1)) * 2 - 1
        f = torch.full((nf, Y, X), float("nan"), dtype=dt, device="cuda:0")
        f[:, :UY, :UX] = ci
        f = f.reshape(nf, X * Y)
        ms = []
        for i in range(3 + a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            et.fpbipere(f, UX, UY, X, Y, ldzon=True)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        assert bool(torch.isfinite(f).all())
        med, mn = statistics.median(ms), min(ms)
        et.set_profile(1)
        et.fpbipere(f, UX, UY, X, Y, ldzon=True)
        kms = et.biper_last_ms()
        et.set_profile(0)
        touch = [e * esz for e in must_touch(nf)]
        tot = sum(touch)
        lines += ["fp%d: the fields hold %.1f MB; the call must touch %.1f MB (%.2f %% of them)" % (8 * esz, nf * X * Y * esz / 1e6, tot / 1e6, 100.0 * tot / (nf * X * Y * esz)),
                  "  FPBIPERE, device arrays   %8.3f ms (%8.3f)  %7.1f GB/s of the bytes it must touch" % (med, mn, tot / (med * 1e-3) / 1e9)]
        ksum = sum(kms)
        for n, k, b in zip(names, kms, touch):
            lines.append("    %-18s %8.3f ms  %5.1f %% of the kernels' time  %7.1f MB  %7.1f GB/s" % (n, k, 100.0 * k / ksum if ksum else 0.0, b / 1e6, b / (k * 1e-3) / 1e9 if k else 0.0))
        lines.append("    kernels together   %8.3f ms (events around every launch; the rest of the call is allocation of the band buffer, launches and the final wait)" % ksum)
        h = f.cpu().numpy()
        hs = []
        for i in range(1 + 3):
            t0 = time.perf_counter()
            et.fpbipere(h, UX, UY, X, Y, ldzon=True)
            if i >= 1:
                hs.append(1e3 * (time.perf_counter() - t0))
        hmed = statistics.median(hs)
        assert np.array_equal(h, f.cpu().numpy())
        lines += ["  FPBIPERE, host array      %8.3f ms  (median of 3 after 1 warm-up: the whole array to the device and back, %.1f GB/s over both ways)" %
                  (hmed, 2 * nf * X * Y * esz / (hmed * 1e-3) / 1e9),
                  "  staging alone             %8.3f ms  (host call - device call): %.0f x the device-resident call" % (hmed - med, (hmed - med) / med), ""]
        del f, ci
    et.trans_end()
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
