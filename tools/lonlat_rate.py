"""Rate of INV_TRANS(LDLATLON) beside the Gaussian inverse of the same build (no threshold; the output is kept in
profiles/lonlat_inv.txt).

T1279 onto the 0.1 degree grid (1801 x 3600), 137 scalar fields in fp64, device-resident arrays: the per-phase device times of one
call (emi_last_phase_ms: spectral pack, Legendre, FFT), the same fields through the Gaussian octahedral O1280 inverse, the Legendre
flop counts of both from emi_work_model and the achieved fraction of the fp64 matrix peak.  The dense lat-lon panels do more flops
per row and the row counts differ, so the fractions compare, not the times.

    python tools/lonlat_rate.py [--nsmax 1279] [--nlat 1801] [--nlon 3600] [--fields 137] [--steps 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F64_MFMA_TFLOPS = 78.6  # as bench.py: 256 CU x 4 SIMD x 32 FLOP / clk / SIMD at 2.4 GHz


def measure(et, torch, r, nf, steps, **kw):
    ns2, ng = et.trans_inq(r, "nspec2"), et.trans_inq(r, "ngptot")
    rng = np.random.default_rng(1)
    sp = torch.from_numpy(rng.uniform(-0.5, 0.5, (ns2, nf))).to("cuda:0")
    sp[1:2 * (et.trans_inq(r, "nsmax") + 1):2] = 0.0
    gp = torch.zeros((1, nf, ng), dtype=torch.float64, device="cuda:0")
    et.inv_trans(r, pspscalar=sp, pgp=gp, **kw)  # warm-up: work buffers, tile maps
    torch.cuda.synchronize()
    et.set_profile(1)
    ms = []
    for _ in range(steps):
        et.inv_trans(r, pspscalar=sp, pgp=gp, **kw)
        torch.cuda.synchronize()
        ms.append(et.last_phase_ms())
    et.set_profile(0)
    assert bool(torch.isfinite(gp).all())
    ms = np.median(np.array(ms), axis=0)
    flops = et.work_model(r, nf)["legendre_flops"]
    del sp, gp
    torch.cuda.empty_cache()
    return ng, ms, flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsmax", type=int, default=1279)
    ap.add_argument("--nlat", type=int, default=1801)
    ap.add_argument("--nlon", type=int, default=3600)
    ap.add_argument("--fields", type=int, default=137)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import ectrans_amd as et
    assert torch.cuda.is_available(), "needs a GPU"
    et.setup_trans0(kmax_resol=2, device=0)
    shifted = a.nlat % 2 == 0
    rows = []
    r = et.setup_trans(a.nsmax, a.nlat if shifted else a.nlat - 1, kdlon=a.nlon, ldll=True, ldshiftll=shifted)
    rows.append(("lat-lon %d x %d" % (a.nlat, a.nlon),) + measure(et, torch, r, a.fields, a.steps, ldlatlon=True))
    et.trans_release(r)
    h = a.nsmax + 1
    nloen = np.array([20 + 4 * i for i in range(h)] + [20 + 4 * i for i in reversed(range(h))], dtype=np.int32)
    r = et.setup_trans(a.nsmax, 2 * h, nloen)
    rows.append(("Gaussian O%d" % h,) + measure(et, torch, r, a.fields, a.steps))
    et.trans_release(r)
    et.trans_end()
    print("INV_TRANS of %d scalar fields, T%d, fp64, device-resident arrays; median of %d calls (ms)" % (a.fields, a.nsmax, a.steps))
    print("%-24s %12s %9s %9s %9s %16s %12s %14s" % ("grid", "points", "pack", "legendre", "fft", "legendre GFLOP", "TFLOP/s", "of fp64 peak"))
    for name, ng, ms, fl in rows:
        tf = fl / (ms[1] * 1e-3) / 1e12
        print("%-24s %12d %9.3f %9.3f %9.3f %16.1f %12.2f %13.1f%%" % (name, ng, ms[0], ms[1], ms[2], fl / 1e9, tf, 100.0 * tf / PEAK_F64_MFMA_TFLOPS))


if __name__ == "__main__":
    main()
