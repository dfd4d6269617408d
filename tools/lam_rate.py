"""Rates of the limited-area transforms EINV_TRANS / EDIR_TRANS (no threshold; the output is kept in profiles/lam_rate.txt).

A 1536 x 1440 grid with linear truncation 767 x 719; 90 levels x 10 scalar fields, vorticity and divergence on 90 levels and one
surface field, in fp64 on device-resident arrays.  Per direction: the device time of the three phases of one call
(emi_last_phase_ms: spectral pack -- empty on a limited-area handle, the y-direction kernel reads and writes the caller's arrays --,
y-direction FFT in the Legendre slot, x-direction FFT), the algorithmic bytes of each phase from the shapes alone (every array read or
written once: the caller's spectral arrays, the Fourier buffer FB[(row, m)][field], the caller's grid arrays), the resulting GB/s and
the ratio of the y-phase to the x-phase.  The x-phase runs the FFT kernels of the spherical path, whose rates on Gaussian grids are
known, so the ratio places the new y-direction kernels beside them.

    python tools/lam_rate.py [--ndlon 1536] [--ndgl 1440] [--levels 90] [--fields 10] [--steps 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndlon", type=int, default=1536)
    ap.add_argument("--ndgl", type=int, default=1440)
    ap.add_argument("--levels", type=int, default=90)
    ap.add_argument("--fields", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("not measured (no GPU)")
        return
    import ectrans_amd as et
    M, N = a.ndlon // 2 - 1, a.ndgl // 2 - 1
    nuv, nsc = a.levels, a.levels * a.fields + 1
    et.setup_trans0(kmax_resol=2, device=0)
    r = et.esetup_trans(M, N, a.ndgl, kdlon=a.ndlon, pexwn=2 * np.pi / (a.ndlon * 1300.0), peywn=2 * np.pi / (a.ndgl * 1300.0))
    ns2, ng = et.etrans_inq(r, "nspec2"), et.etrans_inq(r, "ngptot")
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float64, device=dev, generator=gen) - 0.5
    vor, div, sc = rnd(ns2, nuv), rnd(ns2, nuv), rnd(ns2, nsc)
    mu, mv = rnd(nuv), rnd(nuv)
    gp = torch.zeros((1, 2 * nuv + nsc, ng), dtype=torch.float64, device=dev)
    vor2, div2, sc2, mu2, mv2 = torch.zeros_like(vor), torch.zeros_like(div), torch.zeros_like(sc), torch.zeros_like(mu), torch.zeros_like(mv)

    def inv():
        et.einv_trans(r, pspvor=vor, pspdiv=div, pspscalar=sc, pmeanu=mu, pmeanv=mv, pgp=gp)

    def dirt():
        et.edir_trans(r, pspvor=vor2, pspdiv=div2, pspscalar=sc2, pmeanu=mu2, pmeanv=mv2, pgp=gp)

    rows = []
    nfb = 2 * nuv + nsc  # fields in the Fourier buffer, either direction
    fb = a.ndgl * (M + 1) * nfb * 16.0
    grid = ng * nfb * 8.0
    # spectral side: u and v each read vorticity and divergence (inverse); vorticity and divergence are written once each (direct)
    spec = {"inverse": ns2 * (4 * nuv + nsc) * 8.0, "direct": ns2 * (2 * nuv + nsc) * 8.0}
    for name, fn in (("inverse", inv), ("direct", dirt)):
        fn()  # warm-up: work buffers
        torch.cuda.synchronize()
        et.set_profile(1)
        ms = []
        for _ in range(a.steps):
            fn()
            torch.cuda.synchronize()
            ms.append(et.last_phase_ms())
        et.set_profile(0)
        rows.append((name, np.median(np.array(ms), axis=0), spec[name] + fb, fb + grid))
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(sc2).all())
    et.trans_release(r)
    et.trans_end()
    print("EINV_TRANS / EDIR_TRANS, %d x %d points, truncation %d x %d, %d wind levels + %d scalar fields, fp64, device-resident arrays; "
          "median of %d calls" % (a.ndlon, a.ndgl, M, N, nuv, nsc, a.steps))
    print("nspec2 = %d, ngptot = %d, %d fields in the Fourier buffer (%d (row, m) rows)" % (ns2, ng, nfb, a.ndgl * (M + 1)))
    print("%-10s %10s %10s %10s %14s %14s %10s %10s %8s" % ("direction", "pack ms", "y ms", "x ms", "y bytes (GB)", "x bytes (GB)", "y GB/s", "x GB/s", "y / x"))
    for name, ms, by, bx in rows:
        print("%-10s %10.3f %10.3f %10.3f %14.2f %14.2f %10.1f %10.1f %8.2f" % (name, ms[0], ms[1], ms[2], by / 1e9, bx / 1e9, by / ms[1] / 1e6, bx / ms[2] / 1e6,
                                                                               ms[1] / ms[2]))


if __name__ == "__main__":
    main()
