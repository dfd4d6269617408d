"""The cases of ESPECNORM and EGPNORM_TRANS shared by the emulator tier (tests/test_lam_norms_emu.py) and the GPU tier
(tests/test_lam_norms_gpu.py), against the model of tests/lam_norm_ref.py.  to_dev: numpy -> the array type handed to the library
(torch device tensors on the GPU tier); mem_space as in the Python mirror.

Bounds (derived, not tuned; u = 2^-53).  One term is w (((a^2 + b^2) + c^2) + d^2), computed with the same IEEE operations in the
library and in the model (a fused multiply-add in the library moves a term by at most 2 u).  A sum of K non-negative terms added in
any order in double is within (K - 1) u of the exact sum of the terms, relative; the model's sums (math.fsum) are correctly rounded, u.
So the library is within (K + 2) u of the model.  The tests assert nsq 2^-52 = 8 K u with nsq = 4 K the number of squares in the sum:
nsq = NSPEC2G for a norm (the square root halves the error and adds u) and nsq = 4 (KNTMP(m) + 1) for one wavenumber's sum.
The average of a grid field: a row sum of NDLON points is within NDLON u sum|v| of the exact one, the weight, the division and the sum
over the NDGL rows add (NDGL + 2) u of the result: less than NGPTOTG 2^-52 mean|v| in all, absolute."""
import os
import socket
import subprocess
import sys

import numpy as np

from tests import lam_norm_ref as nr
from tests.lam_common import blocked
from tests.lam_ref import LamRef

HANDLES = [(24, 20, 7, 6), (128, 96, 0, 31), (128, 96, 42, 0), (60, 50, 19, 16)]  # (NDLON, NDGL, KMSMAX, KSMAX)
NFLDS = [1, 63, 64, 65, 130]  # the edges of the kernel's tile of 64 fields
U52 = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dt(precision):
    return np.float64 if precision == 8 else np.float32


def especnorm_case(et, r, ref, nf, precision, with_met, to_dev=None, mem_space=None, seed=5):
    """ESPECNORM and the per-wavenumber sums of one call against the model: returns (error of the norms, bound, worst ratio of a
    per-m error to its bound); all relative."""
    to_dev = to_dev or (lambda a: a)
    dt = _dt(precision)
    rng = np.random.default_rng(seed + nf)
    sp = rng.uniform(-1.0, 1.0, (ref.nspec2, nf)).astype(dt)  # every entry: those the inverse transform ignores enter too
    met = rng.uniform(0.5, 2.0, nr.pmet_size(ref.kntmp)).astype(dt) if with_met else None
    if with_met:
        met[0] = np.nan  # element 0 is never read
    sp64, met64 = sp.astype(np.float64), None if met is None else met.astype(np.float64)
    d = to_dev(sp)
    got = et.especnorm(r, d, met, mem_space=mem_space)
    want = nr.spec_norm(ref, sp64, met64)
    err = float(np.max(np.abs(got - want) / want))
    sums = et.especnorm_partial(r, d, met, mem_space=mem_space)
    wsum = nr.spec_sums(ref, sp64, met64)
    assert sums.shape == wsum.shape == (ref.M + 1, nf)
    worst = 0.0
    for k, m in enumerate(ref.myms):
        e = float(np.max(np.abs(sums[k] - wsum[k]) / wsum[k]))
        worst = max(worst, e / (4 * (int(ref.kntmp[m]) + 1) * U52))
    # the norm is the root of the per-m sums added for m = 0 .. KMSMAX in ascending order
    acc = np.zeros(nf)
    for k in range(sums.shape[0]):
        acc = acc + sums[k]
    assert np.sqrt(acc).tobytes() == got.tobytes()
    return (err if np.isfinite(err) else np.inf), ref.nspec2g * U52, (worst if np.isfinite(worst) else np.inf)


def independence_case(et, r, ref, precision, to_dev=None, mem_space=None):
    """the norm of a field passed alone is byte-identical to its norm as field 1, 64 and 65 of a 130-field call, with and without PMET"""
    to_dev = to_dev or (lambda a: a)
    dt = _dt(precision)
    rng = np.random.default_rng(17)
    sp = rng.uniform(-1.0, 1.0, (ref.nspec2, 130)).astype(dt)
    met = rng.uniform(0.5, 2.0, nr.pmet_size(ref.kntmp)).astype(dt)
    for pm in (None, met):
        many = et.especnorm(r, to_dev(sp), pm, mem_space=mem_space)
        for f in (0, 63, 64):
            alone = et.especnorm(r, to_dev(np.ascontiguousarray(sp[:, f:f + 1])), pm, mem_space=mem_space)
            assert alone.tobytes() == many[f:f + 1].tobytes(), (f, alone, many[f])


def placement_case(et, r, ref, precision, to_dev=None, to_host=None, mem_space=None):
    """an input that sits on an odd element inside a larger NaN-filled buffer gives the same bytes as the same input in an array of its
    own, and the buffer is unchanged afterwards"""
    to_dev = to_dev or (lambda a: a)
    to_host = to_host or (lambda a: a)
    dt = _dt(precision)
    nf = 65
    rng = np.random.default_rng(29)
    sp = rng.uniform(-1.0, 1.0, (ref.nspec2, nf)).astype(dt)
    met = rng.uniform(0.5, 2.0, nr.pmet_size(ref.kntmp)).astype(dt)
    buf = np.full(sp.size + 11, np.nan, dtype=dt)
    buf[3:3 + sp.size] = sp.reshape(-1)
    dbuf = to_dev(buf)
    placed = dbuf[3:3 + sp.size].reshape(ref.nspec2, nf)
    for pm in (None, met):
        a = et.especnorm(r, to_dev(sp), pm, mem_space=mem_space)
        b = et.especnorm(r, placed, pm, mem_space=mem_space)
        assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes()
    assert np.asarray(to_host(dbuf)).tobytes() == buf.tobytes()


def egpnorm_cases(et, precision, to_dev=None, mem_space=None):
    """EGPNORM_TRANS on 251 rows of 300 points with NPROMA = 1000 (blocks cut rows): NaN in the padding of the last block, a surplus
    field holding NaN (gp_nfld = kfields + 1), LDAVE_ONLY.  Returns (error of the averages, bound), absolute."""
    to_dev = to_dev or (lambda a: a)
    dt = _dt(precision)
    ndlon, ndgl, nproma, nf = 300, 251, 1000, 3
    r = et.esetup_trans(99, 83, ndgl, kdlon=ndlon, pexwn=1.0, peywn=1.0, precision=precision)
    try:
        rng = np.random.default_rng(23)
        g = (rng.uniform(-1.0, 1.0, (nf, ndlon * ndgl)) + np.array([0.0, 3.0, -0.25])[:, None]).astype(dt)
        g64 = g.astype(np.float64)
        full = np.concatenate([g, np.full((1, g.shape[1]), np.nan, dtype=dt)])  # the surplus field
        arr = blocked(full, nproma, dt)
        arr[arr == -777.0] = np.nan  # the padding of the last block
        assert np.isnan(arr[-1, 0, -1]) and arr.shape[0] * nproma > ndlon * ndgl
        ave, mn, mx = et.egpnorm_trans(r, to_dev(arr), kfields=nf, kproma=nproma, mem_space=mem_space)
        wave, wmn, wmx = nr.gp_norms(g64, ndgl, ndlon, precision)
        assert np.array_equal(mn, wmn) and np.array_equal(mx, wmx), (mn, wmn, mx, wmx)
        err = float(np.max(np.abs(ave - wave)))
        bound = ndlon * ndgl * U52 * float(np.mean(np.abs(g64)))
        # LDAVE_ONLY: the caller's extrema come back (one task), the averages are the same bytes
        ave2, mn2, mx2 = et.egpnorm_trans(r, to_dev(arr), kfields=nf, kproma=nproma, ldave_only=True, pmin=[-7.0, -8.0, -9.0],
                                          pmax=[7.0, 8.0, 9.0], mem_space=mem_space)
        assert ave2.tobytes() == ave.tobytes() and list(mn2) == [-7.0, -8.0, -9.0] and list(mx2) == [7.0, 8.0, 9.0]
        return (err if np.isfinite(err) else np.inf), bound
    finally:
        et.trans_release(r)


def setup(et, handle, precision):
    ndlon, ndgl, M, N = handle
    return et.esetup_trans(M, N, ndgl, kdlon=ndlon, pexwn=1.0, peywn=1.0, precision=precision), LamRef(ndlon, ndgl, M, N, 1.0, 1.0)


# ---- several tasks (tests/lam_norms_worker.py) ------------------------------------------------------------------------------------------
def run_workers(nproc, outdir, where="cpu", timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1")
    if where == "cpu":
        env["OMP_NUM_THREADS"] = "64"  # the emulator runs a workgroup's lanes as threads; the GPU tier leaves the setting alone
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(s.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "lam_norms_worker.py"), str(rank), str(nproc), outdir, where],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(nproc)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("LAM NORMS OK rank %d of %d" % (rank, nproc)) in out, out
    return [np.load(os.path.join(outdir, "norms_%d_of_%d.npz" % (rank, nproc))) for rank in range(nproc)]


def check_decomposition_invariance(results):
    """results: {tasks: the workers' files}.  Norms, averages and extrema byte-identical across the task counts and the tasks; the
    gathered fields on task 1 and on the last task byte-identical to the one-task arrays; the distributed shares, assembled through
    each task's positions, byte-identical to the one-task share."""
    one = results[1][0]
    for nproc, parts in results.items():
        for p in parts:
            for k in ("norm", "norm_met", "ave", "mn", "mx"):
                assert p[k].tobytes() == one[k].tobytes(), (nproc, k)
        for f in range(5):  # fields 0, 2, 4 on task 1, fields 1, 3 on the last task
            holder = parts[0] if f % 2 == 0 else parts[-1]
            for k in ("gath_spec_%d" % f, "gath_grid_%d" % f):
                assert holder[k].tobytes() == one[k].tobytes(), (nproc, k)
                assert all(k not in q.files for q in parts if q is not holder)
        spec, grid = np.zeros_like(one["dist_spec"]), np.zeros((5, one["rows"][1]))
        for p in parts:
            spec[p["idx"]] = p["dist_spec"]
            n = p["rows"][1] - p["rows"][0]
            grid[:, p["rows"][0]:p["rows"][1]] = np.transpose(p["dist_grid"], (1, 0, 2)).reshape(5, -1)[:, :n]
        one_grid = np.transpose(one["dist_grid"], (1, 0, 2)).reshape(5, -1)[:, :one["rows"][1]]
        assert spec.tobytes() == one["dist_spec"].tobytes() and grid.tobytes() == np.ascontiguousarray(one_grid).tobytes(), nproc
