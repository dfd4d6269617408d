"""SPECNORM with the metric PMET on the sphere (k_specnorm_met): the model and the cases shared by the emulator tier
(tests/test_specnorm_pmet_emu.py) and the GPU tier (tests/test_specnorm_pmet_gpu.py).

Handle: T21 on a reduced grid of 32 rows, so K = NSMAX - m + 1 runs through 22 .. 1: every remainder of the kernel's split of n into
four quarters and every K < 4 occurs.

Model (spnormd_mod.F90:36-53): PNORM(f)^2 = sum over m of c_m sum over n = m .. NSMAX of PMET(n) (re^2 + im^2), c_0 = 1 with the real
parts only, c_m = 2.  Each term c w (re^2 + im^2) is formed in double as the library forms it and the terms are added with math.fsum.

Bound (derived, not tuned; u = 2^-53).  All terms are non-negative.  A sum of K such terms added in any order in double is within
(K - 1) u of the exact sum, relative; the library adds NSPEC2G / 2 terms (per m, then over m), the model's math.fsum is correctly
rounded (u), and a fused multiply-add in a term moves it by at most 2 u.  The squared norm is therefore within (NSPEC2G + 6) u of the
model's, and the norm within half of that plus the rounding of the root, which the + 6 covers."""
import math
import os
import socket
import subprocess
import sys

import numpy as np

NSMAX = 21
NLOEN = np.array([20 + 4 * i for i in range(16)] + [20 + 4 * i for i in reversed(range(16))], dtype=np.int32)
NSPEC2G = (NSMAX + 1) * (NSMAX + 2)
NFLDS = [1, 63, 64, 65, 130]  # the edges of the kernel's tile of 64 fields
KVSET_MIXED = [1, 2, 2, 1, 2, 1, 2]  # the seven fields of the several-task worker on two V-sets: 3 and 4 fields, interleaved
U53 = 2.0 ** -53
BOUND_SQ = (NSPEC2G + 6) * U53  # relative, of the squared norm
BOUND = 0.5 * BOUND_SQ          # relative, of the norm
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dt(precision):
    return np.float64 if precision == 8 else np.float32


def nasm0():
    """0-based position of Re(m, n = m) in the global spectral dimension, m = 0 .. NSMAX"""
    return np.concatenate([[0], np.cumsum([2 * (NSMAX - m + 1) for m in range(NSMAX)])]).astype(np.int64)


def local_index(myms):
    """the rows of the global spectral array that a task with the zonal wavenumbers myms holds, in its order"""
    pos = nasm0()
    return np.concatenate([np.arange(pos[m], pos[m] + 2 * (NSMAX - m + 1)) for m in myms])


def model_sq(spg, met):
    """squared norms of the global fields spg (NSPEC2G, nf) under the metric met (>= NSMAX + 1 elements), float64 inputs"""
    pos = nasm0()
    out = np.zeros(spg.shape[1])
    for f in range(spg.shape[1]):
        terms = []
        for m in range(NSMAX + 1):
            blk = spg[pos[m]:pos[m] + 2 * (NSMAX - m + 1), f]
            re, im = blk[0::2], (blk[1::2] if m > 0 else np.zeros(NSMAX - m + 1))
            terms.extend((1.0 if m == 0 else 2.0) * (met[m:NSMAX + 1] * (re * re + im * im)))
        out[f] = math.fsum(terms)
    return out


def fields(nf, precision, seed=5, nan_imag0=True):
    """random global fields rounded to the precision; the imaginary parts of m = 0 hold NaN: they carry no weight"""
    rng = np.random.default_rng(seed + nf)
    sp = rng.uniform(-1.0, 1.0, (NSPEC2G, nf)).astype(dt(precision))
    if nan_imag0:
        sp[1:2 * (NSMAX + 1):2] = np.nan
    return sp


def metric(precision, seed=9, extra=0):
    return np.random.default_rng(seed).uniform(0.5, 2.0, NSMAX + 1 + extra).astype(dt(precision))


def rel(got, want):
    e = float(np.max(np.abs(got - want) / want))
    return e if np.isfinite(e) else np.inf


def model_case(et, r, nf, precision, to_dev=None, mem_space=None):
    """(a): norms and per-wavenumber sums of one call against the model; returns (error of the norms, of the squared per-m sums)"""
    to_dev = to_dev or (lambda a: a)
    sp, met = fields(nf, precision), metric(precision, extra=3)  # (a longer PMET: only NSMAX + 1 elements are read)
    met[NSMAX + 1:] = np.nan
    d = to_dev(sp)
    got = et.specnorm(r, d, pmet=met, mem_space=mem_space)
    want = np.sqrt(model_sq(sp.astype(np.float64), met.astype(np.float64)))
    sums = et.specnorm_met_partial(r, d, met, mem_space=mem_space)
    assert sums.shape == (NSMAX + 1, nf)
    acc = np.zeros(nf)  # the norm is the root of the per-m sums added for m = 0 .. NSMAX in ascending order
    for m in range(NSMAX + 1):
        acc = acc + sums[m]
    assert np.sqrt(acc).tobytes() == got.tobytes()
    return rel(got, want), rel(acc, want * want)


def unit_metric_case(et, r, precision, to_dev=None):
    """(b): PMET = e_n isolates the coefficients of total wavenumber n, for every n: an index off by one in n or in m shows"""
    to_dev = to_dev or (lambda a: a)
    sp = fields(3, precision, seed=13)
    d, sp64, worst = to_dev(sp), sp.astype(np.float64), 0.0
    for n in range(NSMAX + 1):
        met = np.zeros(NSMAX + 1, dtype=dt(precision))
        met[n] = 1.0
        got = et.specnorm(r, d, pmet=met)
        worst = max(worst, rel(got, np.sqrt(model_sq(sp64, met.astype(np.float64)))))
    return worst


def ones_case(et, r, nf, precision, to_dev=None):
    """(c): PMET = 1 against SPECNORM without a metric (another kernel, another summation order: twice the bound)"""
    to_dev = to_dev or (lambda a: a)
    d = to_dev(fields(nf, precision, seed=21, nan_imag0=False))
    return rel(et.specnorm(r, d, pmet=np.ones(NSMAX + 1)), et.specnorm(r, d))


def independence_case(et, r, precision, to_dev=None, mem_space=None):
    """(d): the norm of a field passed alone is byte-identical to its norm as field 1, 64, 65 and 130 of a 130-field call, and to its
    norm in calls of the other field counts"""
    to_dev = to_dev or (lambda a: a)
    sp, met = fields(130, precision, seed=17), metric(precision)
    many = et.specnorm(r, to_dev(sp), pmet=met, mem_space=mem_space)
    assert np.all(np.isfinite(many))
    for f in (0, 63, 64, 129):
        alone = et.specnorm(r, to_dev(np.ascontiguousarray(sp[:, f:f + 1])), pmet=met, mem_space=mem_space)
        assert alone.tobytes() == many[f:f + 1].tobytes(), (f, alone, many[f])
    for nf in (63, 64, 65):
        part = et.specnorm(r, to_dev(np.ascontiguousarray(sp[:, 130 - nf:])), pmet=met, mem_space=mem_space)
        assert part.tobytes() == many[130 - nf:].tobytes(), nf
    return many


# ---- several tasks (tests/specnorm_pmet_worker.py) --------------------------------------------------------------------------------------
def run_workers(nproc, outdir, where="cpu", nprv=1, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1")
    if where == "cpu":
        env["OMP_NUM_THREADS"] = "64"  # the emulator runs a workgroup's lanes as threads; the GPU tier leaves the setting alone
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(s.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "specnorm_pmet_worker.py"), str(rank), str(nproc), outdir, where,
                               str(nprv)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(nproc)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("SPECNORM PMET OK rank %d of %d" % (rank, nproc)) in out, out
    return [np.load(os.path.join(outdir, "pmet_%d_of_%d_v%d.npz" % (rank, nproc, nprv))) for rank in range(nproc)]
