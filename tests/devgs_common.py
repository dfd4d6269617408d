"""Shared cases of the DIST_* / GATH_* routines on device-resident fields (emi_dist_spec_m ... emi_egath_grid_m): run by
tests/test_devgs_emu.py on the CPU functional emulator (numpy arrays in place: mem_space=EMI_MEM_DEVICE) and by tests/test_devgs_gpu.py
on the HIP build (torch device tensors).  The yardstick is the host path of the same library (emi_dist_spec ... emi_egath_grid), which
other tests hold to the reference's layouts; the routines only copy, so every comparison is on bytes.  Every array of a device-path call
is placed as a caller places it (tests/common.py::GuardedSpace): inside a larger buffer, on an odd element, sentinels around it."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np

from tests.common import GuardedSpace, guard_for, octahedral

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE, AUTO = 0, 1, 2
# (handle, fields, NPROMA; None = NGPTOT, kinds: s spectral, g grid): every field count on the handle with a partial element tile, the
# largest array (70 x 4160 reals) on the handle with whole tiles, 1 / 33 / 70 fields of either kind and NPROMA 37 / 64 / NGPTOT.  Grid
# fields in their dozens go to the small handles: the emulator runs every 256-point workgroup as 256 threads, milliseconds each.
CASES = [("o21", 1, None, "sg"), ("o21", 5, 37, "sg"), ("o21", 33, 64, "sg"), ("o21", 70, 37, "s"), ("f63", 5, 64, "s"), ("f63", 70, None, "s"),
         ("ll", 5, None, "sg"), ("ll", 33, 37, "sg"), ("ll", 70, 64, "g"), ("lam", 1, 64, "sg"), ("lam", 5, 37, "g"), ("lam", 33, None, "s"),
         ("lam", 70, 37, "s")]
# the GPU tier has no such limit: every handle x field count x NPROMA, both kinds
FULL_CASES = [(h, nf, kp, "sg") for h in ("o21", "f63", "ll", "lam") for nf in (1, 5, 33, 70) for kp in (None, 37, 64)]
_HANDLES = {}


def handle(et, name, precision):
    """(kresol, "" | "e") of a named handle, set up once per library and precision"""
    key = (id(et.lib()), name, precision)
    if key not in _HANDLES:
        if name == "o21":  # nspec2 = 506: a partial tile of elements
            nloen = octahedral(21)
            r = et.setup_trans(21, len(nloen), nloen, precision=precision)
        elif name == "f63":  # full grid, nspec2 = 4160: whole tiles of elements
            r = et.setup_trans(63, 96, None, kdlon=192, precision=precision)
        elif name == "ll":  # 24 x 13 points pole to pole
            r = et.setup_trans(10, 12, kdlon=24, ldll=True, precision=precision)
        else:  # limited area, 60 x 50 points, truncation 19 x 16
            r = et.esetup_trans(19, 16, 50, kdlon=60, pexwn=1.0, peywn=1.0, precision=precision)
        _HANDLES[key] = (r, "e" if name == "lam" else "")
    return _HANDLES[key]


def forget_handles():
    _HANDLES.clear()


def _ptr(a):
    return None if a is None else C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def call(et, name, *args):
    """a C-ABI routine by name; (return code, message)"""
    rc = getattr(et.lib(), name)(*args)
    return rc, (et.lib().emi_last_error().decode() if rc else "")


def ok(et, name, *args):
    rc, msg = call(et, name, *args)
    assert rc == 0, "%s: %s" % (name, msg)


def permutation(nfld, seed=5):
    """KSORT: a permutation of 1 .. nfld that is not the identity (nfld > 1)"""
    p = np.random.default_rng(seed).permutation(nfld)
    if nfld > 1 and (p == np.arange(nfld)).all():
        p = np.roll(p, 1)
    return (p + 1).astype(np.int32)


def devgs_case(et, name, nfld, kproma, precision, glob_dev, dev_mem, kinds="sg", lead=1):
    """All four directions on one handle with one task: the device path on placed arrays against the host path on the same data.
    dev_mem = (to_flat, back) of the memory the local arrays live in (GuardedSpace); the global image lives there too (glob_dev) or in
    host memory.  Returns the violations (strings)."""
    r, e = handle(et, name, precision)
    dt = np.dtype(et.real_dtype(r))
    q = lambda n: et.trans_inq(r, n)
    ns2, ns2g, ng, ngg = q("nspec2"), q("nspec2g"), q("ngptot"), q("ngptotg")
    assert (ns2, ng) == (ns2g, ngg)
    nproma = kproma or ng
    nblk = (ng - 1) // nproma + 1
    rng = np.random.default_rng(1000 * nfld + nproma)
    specg = rng.uniform(-1.0, 1.0, (nfld, ns2g)).astype(dt)
    gpg = (rng.uniform(-1.0, 1.0, (nfld, ngg)) + np.arange(nfld)[:, None]).astype(dt)
    one = np.ones(nfld, dtype=np.int32)
    ksort = permutation(nfld)
    # ---- the host path: the references.  Arrays that are written start as NaN, so that what a routine leaves alone (the padding of the
    # last NPROMA block) compares equal between the two paths only if neither writes it
    spec_ref, gp_ref = np.full((ns2, nfld), np.nan, dtype=dt), np.full((nblk, nfld, nproma), np.nan, dtype=dt)
    specg_ref, gpg_ref = np.full((nfld, ns2g), np.nan, dtype=dt), np.full((nfld, ngg), np.nan, dtype=dt)
    if "s" in kinds:
        ok(et, "emi_%sdist_spec" % e, r, _ptr(specg), nfld, _ip(one), _ip(ksort), _ptr(spec_ref))
        ok(et, "emi_%sgath_spec" % e, r, _ptr(specg_ref), nfld, _ip(one), _ptr(spec_ref))
        assert not np.isnan(spec_ref).any() and not np.isnan(specg_ref).any()
    if "g" in kinds:
        ok(et, "emi_%sdist_grid" % e, r, _ptr(gpg), nfld, _ip(one), _ip(ksort), nproma, _ptr(gp_ref))
        ok(et, "emi_%sgath_grid" % e, r, _ptr(gpg_ref), nfld, _ip(one), nproma, _ptr(gp_ref))
        assert not np.isnan(gpg_ref).any() and int(np.isnan(gp_ref).sum()) == nfld * (nblk * nproma - ng)
    # ---- the device path on placed arrays
    guard = guard_for(max(nproma, 64))
    host_mem = (lambda a: a, lambda a: np.asarray(a))
    bad = []
    gsp = DEVICE if glob_dev else HOST

    def spaces():
        loc = GuardedSpace(lead, guard, *dev_mem)
        return loc, (loc if glob_dev else GuardedSpace(lead, guard, *host_mem))

    def same(space, view, ref, what):
        if np.ascontiguousarray(space.back(view)).tobytes() != ref.tobytes():
            bad.append("%s: differs from the host path" % what)

    def finish(what, *sp):
        for s in set(sp):
            bad.extend("%s: %s" % (what, v) for v in s.check())

    # DIST_SPEC / DIST_GRID: global image in, local array (NaN before the call) out
    for kind, glob, ref, extra in (("spec", specg, spec_ref, ()), ("grid", gpg, gp_ref, (nproma,))):
        if kind[0] not in kinds:
            continue
        what = "%sDIST_%s %s nfld %d nproma %d %s" % (e.upper(), kind.upper(), name, nfld, nproma, "device image" if glob_dev else "host image")
        sl, sg = spaces()
        g = sg.put(glob, "in")
        loc = sl.put(np.full(ref.shape, np.nan, dtype=dt), "out")
        ok(et, "emi_%sdist_%s_m" % (e, kind), r, gsp, _ptr(g), nfld, _ip(one), _ip(ksort), *extra, DEVICE, _ptr(loc))
        same(sl, loc, ref, what)
        finish(what, sl, sg)
    # GATH_SPEC / GATH_GRID: local array (NaN in the padding) in, global image (NaN before the call) out
    for kind, locref, ref, extra in (("spec", spec_ref, specg_ref, ()), ("grid", gp_ref, gpg_ref, (nproma,))):
        if kind[0] not in kinds:
            continue
        what = "%sGATH_%s %s nfld %d nproma %d %s" % (e.upper(), kind.upper(), name, nfld, nproma, "device image" if glob_dev else "host image")
        sl, sg = spaces()
        loc = sl.put(locref, "in")
        g = sg.put(np.full(ref.shape, np.nan, dtype=dt), "out")
        ok(et, "emi_%sgath_%s_m" % (e, kind), r, gsp, _ptr(g), nfld, _ip(one), *extra, DEVICE, _ptr(loc))
        same(sg, g, ref, what)
        finish(what, sl, sg)
    return bad


def python_case(et, name, precision, to_dev, is_dev=None):
    """the keywords of the Python mirror: mem_space=EMI_MEM_DEVICE gives what the calls without them give, in the memory asked for.
    to_dev(numpy) -> an array in device memory; is_dev(x): x lives there (None on the emulator, where both memories are numpy arrays)"""
    r, e = handle(et, name, precision)
    dt = np.dtype(et.real_dtype(r))
    nf, nproma = 5, 37
    ns2g, ngg = et.trans_inq(r, "nspec2g"), et.trans_inq(r, "ngptotg")
    rng = np.random.default_rng(3)
    spg, gpg = rng.uniform(-1, 1, (ns2g, nf)).astype(dt), rng.uniform(-1, 1, (nf, ngg)).astype(dt)
    f = lambda n: getattr(et, e + n)
    back = lambda a: np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    sp0, gp0 = f("dist_spec")(r, spg, nf), f("dist_grid")(r, gpg, nf, kproma=nproma)
    for gs, src in ((None, lambda a: a), (DEVICE, lambda a: a), (None, to_dev), (HOST, to_dev)):
        sp = f("dist_spec")(r, src(spg), nf, mem_space=DEVICE, glob_space=gs)
        gp = f("dist_grid")(r, src(gpg), nf, kproma=nproma, mem_space=DEVICE, glob_space=gs)
        assert is_dev is None or (is_dev(sp) and is_dev(gp))
        assert back(sp).tobytes() == sp0.tobytes() and back(gp).tobytes() == gp0.tobytes(), gs
    sg0, gg0 = f("gath_spec")(r, sp0, nf), f("gath_grid")(r, gp0, nf)
    assert sg0.tobytes() == spg.tobytes() and gg0.tobytes() == gpg.tobytes()
    for gs in (None, HOST, DEVICE):
        sg = f("gath_spec")(r, to_dev(sp0), nf, mem_space=DEVICE, glob_space=gs)
        gg = f("gath_grid")(r, to_dev(gp0), nf, mem_space=DEVICE, glob_space=gs)
        assert is_dev is None or (is_dev(sg) == (gs == DEVICE) and is_dev(gg) == (gs == DEVICE))
        assert tuple(sg.shape) == sg0.shape
        assert back(sg).tobytes() == sg0.tobytes() and back(gg).tobytes() == gg0.tobytes(), gs


def refusal_cases(et, precision=8):
    """a device global array beside a host local array; the wrong kind of handle; KSORT out of range: [(what, return code, message, expected text)]"""
    out = []
    for name in ("o21", "lam"):
        r, e = handle(et, name, precision)
        other = "" if e else "e"
        dt = np.dtype(et.real_dtype(r))
        nf, ns2, ng = 2, et.trans_inq(r, "nspec2"), et.trans_inq(r, "ngptot")
        one, bad_sort = np.ones(nf, dtype=np.int32), np.array([1, 3], dtype=np.int32)
        sg, sp = np.zeros((nf, ns2), dtype=dt), np.zeros((ns2, nf), dtype=dt)
        gg, gp = np.zeros((nf, ng), dtype=dt), np.zeros((1, nf, ng), dtype=dt)
        E = e.upper()
        wrong = "is a limited-area handle" if e else "is not a limited-area handle"
        for what, text, nm, args in (
                ("device image, host field", "%sGATH_SPEC: THE GLOBAL ARRAY IS IN DEVICE MEMORY AND THE LOCAL ARRAY IN HOST MEMORY" % E, "emi_%sgath_spec_m" % e,
                 (r, DEVICE, _ptr(sg), nf, _ip(one), HOST, _ptr(sp))),
                ("device image, host field", "%sDIST_GRID: THE GLOBAL ARRAY IS IN DEVICE MEMORY AND THE LOCAL ARRAY IN HOST MEMORY" % E, "emi_%sdist_grid_m" % e,
                 (r, DEVICE, _ptr(gg), nf, _ip(one), None, 0, HOST, _ptr(gp))),
                ("wrong handle", wrong, "emi_%sdist_spec_m" % other, (r, HOST, _ptr(sg), nf, _ip(one), None, DEVICE, _ptr(sp))),
                ("wrong handle", wrong, "emi_%sgath_grid_m" % other, (r, HOST, _ptr(gg), nf, _ip(one), 0, DEVICE, _ptr(gp))),
                ("KSORT", "%sDIST_SPEC: KSORT(2) = 3 outside 1..2" % E, "emi_%sdist_spec_m" % e, (r, HOST, _ptr(sg), nf, _ip(one), _ip(bad_sort), DEVICE, _ptr(sp))),
                ("KSORT", "%sDIST_GRID: KSORT(2) = 3 outside 1..2" % E, "emi_%sdist_grid_m" % e, (r, HOST, _ptr(gg), nf, _ip(one), _ip(bad_sort), 0, DEVICE, _ptr(gp))),
                ("memory space", "memory space 7", "emi_%sgath_grid_m" % e, (r, 7, _ptr(gg), nf, _ip(one), 0, DEVICE, _ptr(gp)))):
            rc, msg = call(et, nm, *args)
            out.append(("%s %s %s" % (name, nm, what), rc, msg, text))
        # nothing was written by a refused call
        assert not sg.any() and not sp.any() and not gg.any() and not gp.any()
    return out


# ---- several tasks ----------------------------------------------------------------------------------------------------------------------
def run_workers(nproc, outdir, where="cpu", timeout=600):
    """tests/devgs_worker.py on nproc tasks over gloo; the files the tasks wrote"""
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1")
    if where == "cpu":
        env["OMP_NUM_THREADS"] = "256"  # the emulator runs a workgroup's lanes as threads; the GPU tier leaves the setting alone
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(s.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "devgs_worker.py"), str(rank), str(nproc), outdir, where],
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
        assert p.returncode == 0 and ("DEVGS OK rank %d of %d" % (rank, nproc)) in out, out
    return [np.load(os.path.join(outdir, "devgs_%d_of_%d.npz" % (rank, nproc))) for rank in range(nproc)]


def check_tasks(results, nf=5):
    """results: {tasks: the workers' files}.  The gathered images on task 1 and on the last task are byte-identical to one task's; the
    distributed shares, assembled through each task's positions, are byte-identical to the one-task share.  (Each worker has already
    compared the device path with the host path on its own task count, and the bytes of the exchange with the count of the issue.)"""
    one = results[1][0]
    for nproc, parts in results.items():
        for h in ("o21_8", "lam_8", "o21_4", "lam_4"):
            for f in range(nf):  # fields 0, 2, 4 on task 1, fields 1, 3 on the last task
                holder = parts[0] if f % 2 == 0 else parts[-1]
                for k in ("gath_spec", "gath_grid"):
                    key = "%s_%s_%d" % (h, k, f)
                    assert holder[key].tobytes() == one[key].tobytes(), (nproc, key)
            if nproc == 3:
                assert not [k for k in parts[1].files if "gath" in k], "the middle task is the target of nothing"
            for k in ("spec", "grid"):
                whole = np.full_like(one["%s_dist_%s" % (h, k)], np.nan)
                for p in parts:
                    whole[:, p["%s_pos_%s" % (h, k)]] = p["%s_dist_%s" % (h, k)]
                assert whole.tobytes() == one["%s_dist_%s" % (h, k)].tobytes(), (nproc, h, k)
