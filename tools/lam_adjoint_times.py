"""Times of the limited-area adjoints beside the forward routines of the same direction (no threshold; the output is kept in
profiles/lam_adjoints.txt).

1536 x 1440 points, truncation 767 x 719, 8 wind and 16 scalar fields, no derivative flags, device-resident arrays, fp64 and fp32.
EINV_TRANSAD runs the passes of EDIR_TRANS (grid -> spectral) and EDIR_TRANSAD those of EINV_TRANS, so each adjoint is timed against
that forward routine, alternating with it in the same process: per call the device time of the phases (emi_last_phase_ms with the
phase timers on: spectral pack -- empty on a limited-area handle --, y-direction kernel in the Legendre slot, x-direction FFT) and the
host time from the call to the end of a device synchronise; medians over the calls.

    python tools/lam_adjoint_times.py [--steps 20] [--out profiles/lam_adjoints.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NDLON, NDGL, NUV, NSC = 1536, 1440, 8, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("not measured (no GPU)")
        return 1
    import ectrans_amd as et
    M, N = NDLON // 2 - 1, NDGL // 2 - 1
    et.setup_trans0(kmax_resol=2, device=0)
    lines = ["EINV_TRANSAD against EDIR_TRANS, EDIR_TRANSAD against EINV_TRANS: %d x %d points, truncation %d x %d, %d wind + %d scalar fields, no flags,"
             % (NDLON, NDGL, M, N, NUV, NSC),
             "device-resident arrays, phase timers on; each pair alternates in one process, medians of %d calls (ms)" % a.steps,
             "%-6s %-14s %10s %10s %10s %12s %10s" % ("", "routine", "pack", "y kernel", "x FFT", "call + sync", "/ forward")]
    for prec, dt in ((8, torch.float64), (4, torch.float32)):
        r = et.esetup_trans(M, N, NDGL, kdlon=NDLON, pexwn=2 * np.pi / (NDLON * 1300.0), peywn=2 * np.pi / (NDGL * 1300.0), precision=prec)
        ns2, ng = et.etrans_inq(r, "nspec2"), et.etrans_inq(r, "ngptot")
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        rnd = lambda *s: torch.rand(*s, dtype=dt, device="cuda:0", generator=gen) - 0.5
        sp_in = dict(pspvor=rnd(ns2, NUV), pspdiv=rnd(ns2, NUV), pspscalar=rnd(ns2, NSC), pmeanu=rnd(NUV), pmeanv=rnd(NUV))
        sp_out = {k: torch.zeros_like(v) for k, v in sp_in.items()}
        g_in, g_out = rnd(1, 2 * NUV + NSC, ng), torch.zeros((1, 2 * NUV + NSC, ng), dtype=dt, device="cuda:0")
        pairs = (("EDIR_TRANS", lambda: et.edir_trans(r, pgp=g_in, **sp_out), "EINV_TRANSAD", lambda: et.einv_transad(r, pgp=g_in, **sp_out)),
                 ("EINV_TRANS", lambda: et.einv_trans(r, pgp=g_out, **sp_in), "EDIR_TRANSAD", lambda: et.edir_transad(r, pgp=g_out, **sp_in)))
        for fname, fwd, aname, adj in pairs:
            for fn in (fwd, adj):  # warm-up: work buffers, code objects
                fn()
            torch.cuda.synchronize()
            et.set_profile(1)
            rec = {fname: [], aname: []}
            for _ in range(a.steps):
                for name, fn in ((fname, fwd), (aname, adj)):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    rec[name].append(et.last_phase_ms() + [1e3 * (time.perf_counter() - t0)])
            et.set_profile(0)
            med = {k: np.median(np.array(v), axis=0) for k, v in rec.items()}
            for name in (fname, aname):
                m = med[name]
                lines.append("%-6s %-14s %10.3f %10.3f %10.3f %12.3f %10.2f" % ("fp64" if prec == 8 else "fp32", name, m[0], m[1], m[2], m[3],
                                                                          (m[1] + m[2]) / (med[fname][1] + med[fname][2])))
        assert all(bool(torch.isfinite(v).all()) for v in sp_out.values()) and bool(torch.isfinite(g_out).all())
        et.trans_release(r)
    et.trans_end()
    lines.append("/ forward: the sum of the y-kernel and x-FFT device times over that of the forward routine of the same direction")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
