"""Shared cases of DIST_* / GATH_* with V-sets (NPRTRV > 1): run by tests/vsets_gs_worker.py on NPRTRW x NPRTRV tasks over gloo, which
tests/test_vsets_gs_emu.py launches on the CPU functional emulator and tests/test_vsets_gs_gpu.py on the HIP build (all tasks on cuda:0).
The routines only copy, so every layout check is on bytes: element i of global field f holds (f + 1) * 8192 + i, exact in fp32, and each
task works out the piece it must hold from the inquiries alone (myms, nasm0, nspec2, nfrstlat, ngptot, mysetv).  Arrays are placed as a
caller places them (tests/common.py::GuardedSpace: an odd element, sentinels around).  The C-ABI is called directly where the Python
mirror has no keyword (KSORT, a sentinel-filled PSPECG on a task that is no target); the transform case goes through the mirror."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np

from tests.common import GuardedSpace, guard_for, octahedral, random_spectrum, rel_err
from tests.specnorm_pmet_common import KVSET_MIXED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE = 0, 1
NSPEC, NGRID = 7, 5  # global spectral / grid fields
SENT = -4321.0       # a global array that no field of the call lands in
PATHS = (("host", HOST, HOST), ("device, host image", HOST, DEVICE), ("device, device image", DEVICE, DEVICE))
ALL_CASES = ("layout", "ksort", "kproma", "empty", "chunk", "transform", "refuse")
TOL = {8: 1e-12, 4: 3e-5}  # the bound tests/vsets_worker.py applies to its own pieces (its `tol[0]`)


def kvset_for(nprv):
    """KVSET_MIXED; with three V-sets set 3 takes two of the fields"""
    kv = list(KVSET_MIXED)
    if nprv == 3:
        kv[2], kv[6] = 3, 3
    assert set(kv) == set(range(1, nprv + 1))
    return np.array(kv, dtype=np.int32)


def spread(nfld, ntasks, sources):
    """sources: fields come from tasks 2 .. NPROC in turn (task 1 is the source of nothing); targets: they go to tasks 1 .. NPROC - 1,
    starting at 2 (the last task is the target of nothing).  Two tasks: everything from task 2, everything to task 1."""
    if ntasks == 2:
        return np.full(nfld, 2 if sources else 1, dtype=np.int32)
    return np.array([2 + j % (ntasks - 1) if sources else 1 + (j + 1) % (ntasks - 1) for j in range(nfld)], dtype=np.int32)


def _ptr(a):
    return None if a is None else C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


class Tasks:
    """one task's view of a handle: its numbers, the pieces it must hold, and the four routines on placed arrays"""

    def __init__(self, et, r, dev_mem, nprv):
        self.et, self.r, self.dev_mem, self.nprv = et, r, dev_mem, nprv
        self.host_mem = (lambda a: a, lambda a: np.asarray(a))
        q = lambda n: et.trans_inq(r, n)
        self.dt = np.dtype(et.real_dtype(r))
        self.nt, self.me, self.myv = q("nproc"), q("myproc"), q("mysetv")
        self.ns2, self.ns2g, self.ng, self.ngg = q("nspec2"), q("nspec2g"), q("ngptot"), q("ngptotg")
        n, nasm0, nloen = q("nsmax"), q("nasm0"), np.asarray(q("nloen"))
        iasm0g = np.concatenate([[0], np.cumsum([2 * (n - m + 1) for m in range(n + 1)])])
        self.pos_s = np.full(self.ns2, -1, dtype=np.int64)  # global position of every local coefficient
        for m in q("myms"):
            self.pos_s[nasm0[m] - 1:nasm0[m] - 1 + 2 * (n - m + 1)] = np.arange(iasm0g[m], iasm0g[m + 1])
        assert (self.pos_s >= 0).all() and iasm0g[-1] == self.ns2g
        lat0, lat1 = q("nfrstlat") - 1, q("nlstlat")
        assert self.ng == int(nloen[lat0:lat1].sum()) and self.ngg == int(nloen.sum())
        self.pos_g = int(nloen[:lat0].sum()) + np.arange(self.ng, dtype=np.int64)  # latitude order = task order
        self.bad = []

    # ---- values ----
    def code(self, f, n):
        return ((f + 1) * 8192 + np.arange(n)).astype(self.dt)

    def local_fields(self, kvset, nfld):
        return list(range(nfld)) if kvset is None else [f for f in range(nfld) if kvset[f] == self.myv]

    def want_spec(self, fields, slots=None):
        """PSPEC (nspec2, nfl) holding `fields` (global numbers) in the slots given"""
        out = np.full((self.ns2, len(fields)), np.nan, dtype=self.dt)
        for k, f in enumerate(fields):
            out[:, k if slots is None else slots[k]] = self.code(f, self.ns2g)[self.pos_s]
        return out

    def want_grid(self, fields, nproma, fill, slots=None):
        nblk = (self.ng - 1) // nproma + 1
        flat = np.full((len(fields), nblk * nproma), fill, dtype=self.dt)
        for k, f in enumerate(fields):
            flat[k if slots is None else slots[k], :self.ng] = self.code(f, self.ngg)[self.pos_g]
        return np.ascontiguousarray(flat.reshape(len(fields), nblk, nproma).transpose(1, 0, 2))

    # ---- calls ----
    def _spaces(self, gsp, lsp, nproma):
        guard = guard_for(max(nproma, 64))
        return GuardedSpace(1, guard, *(self.dev_mem if gsp == DEVICE else self.host_mem)), GuardedSpace(1, guard, *(self.dev_mem if lsp == DEVICE else self.host_mem))

    def call(self, name, *args):
        rc = getattr(self.et.lib(), name)(*args)
        return rc, (self.et.lib().emi_last_error().decode() if rc else "")

    def move(self, kind, gath, path, glob, loc, nfld, ktask, kvset=None, ksort=None, kproma=None, what=""):
        """one routine on placed arrays.  glob: numpy [n][nglob] or None (this task passes no global array); loc: numpy local array or
        None.  Returns (return code, message, global array after the call, local array after the call)."""
        _, gsp, lsp = path
        nproma = kproma or self.ng
        sg, sl = self._spaces(gsp, lsp, nproma)
        g = None if glob is None else sg.put(glob, "out" if gath else "in")
        l = None if loc is None else sl.put(loc, "in" if gath else "out")
        kt = np.ascontiguousarray(ktask, dtype=np.int32)
        kv = None if kvset is None else np.ascontiguousarray(kvset, dtype=np.int32)
        ks = None if ksort is None else np.ascontiguousarray(ksort, dtype=np.int32)
        if kind == "spec":
            args = (self.r, gsp, _ptr(g), nfld, _ip(kt), _ip(kv)) + (() if gath else (_ip(ks),)) + (lsp, _ptr(l))
            rc, msg = self.call("emi_%s_spec_v" % ("gath" if gath else "dist"), *args)
        else:
            args = (self.r, gsp, _ptr(g), nfld, _ip(kt)) + (() if gath else (_ip(ks),)) + (nproma, lsp, _ptr(l))
            rc, msg = self.call("emi_%s_grid_m" % ("gath" if gath else "dist"), *args)
        for s in {id(sg): sg, id(sl): sl}.values():  # the guards stay intact and the inputs stay unchanged
            self.bad.extend("%s %s: %s" % (what, path[0], v) for v in s.check())
        return rc, msg, None if g is None else np.ascontiguousarray(sg.back(g)), None if l is None else np.ascontiguousarray(sl.back(l))

    def same(self, got, want, what):
        if got is None or want is None:
            if not (got is None and want is None):
                self.bad.append("%s: an array is missing" % what)
        elif got.shape != want.shape or got.tobytes() != want.tobytes():
            w = np.flatnonzero(got.reshape(-1) != want.reshape(-1)) if got.shape == want.shape else []
            self.bad.append("%s: differs (shape %s / %s, first flat indices %s)" % (what, got.shape, want.shape, list(w[:6])))

    def glob_of(self, fields, nglob):
        return np.stack([self.code(f, nglob) for f in fields]) if fields else None

    def round_trip(self, path, kvset, kfrom_s, kto_s, kfrom_g, kto_g, kproma, what, kinds="sg", pad_dist=-777.0):
        """DIST_* from the sources, each task checks its piece; GATH_* of those pieces to the targets, each target checks the fields;
        a task that is the target of none passes a sentinel-filled global array that must stay as it is.  Returns what the task got:
        [local spectral, gathered spectral, local grid, gathered grid]."""
        out = []
        for kind in ("spec", "grid"):
            if kind[0] not in kinds:
                continue
            spec = kind == "spec"
            nfld, kfrom, kto, kv = (len(kfrom_s), kfrom_s, kto_s, kvset) if spec else (len(kfrom_g), kfrom_g, kto_g, None)
            nglob = self.ns2g if spec else self.ngg
            kp = None if spec else kproma
            fl = self.local_fields(kv, nfld)
            mine = [f for f in range(nfld) if kfrom[f] == self.me]
            if spec:
                loc0 = np.full((self.ns2, len(fl)), np.nan, dtype=self.dt) if fl else None
                want = self.want_spec(fl) if fl else None
            else:
                loc0 = np.full(((self.ng - 1) // (kp or self.ng) + 1, nfld, kp or self.ng), pad_dist, dtype=self.dt)
                want = self.want_grid(fl, kp or self.ng, pad_dist)
            w = "%s DIST_%s" % (what, kind.upper())
            rc, msg, _, loc = self.move(kind, False, path, self.glob_of(mine, nglob), loc0, nfld, kfrom, kv, None, kp, w)
            assert rc == 0, (w, path[0], msg)
            self.same(loc, want, "%s %s" % (w, path[0]))
            out.append(loc)
            # back, to another spread of tasks; the padding of the last NPROMA block is NaN: it is never read
            tgt = [f for f in range(nfld) if kto[f] == self.me]
            src = want if spec else self.want_grid(fl, kp or self.ng, np.nan)
            g0 = np.full((max(len(tgt), 1), nglob), SENT, dtype=self.dt)
            w = "%s GATH_%s" % (what, kind.upper())
            rc, msg, g, _ = self.move(kind, True, path, g0, src, nfld, kto, kv, None, kp, w)
            assert rc == 0, (w, path[0], msg)
            self.same(g, self.glob_of(tgt, nglob) if tgt else g0, "%s %s" % (w, path[0]))
            out.append(g)
        return out


def run_all(et, r, dev_mem, nprv, cases, name, oracle=None):
    """every case of `cases` on handle r (name "o21": spectral and grid; "f63": spectral only).  Returns the violations."""
    T = Tasks(et, r, dev_mem, nprv)
    nt, me = T.nt, T.me
    kinds = "sg" if name == "o21" else "s"
    kv = kvset_for(nprv)
    kfrom_s, kto_s, kfrom_g, kto_g = spread(NSPEC, nt, True), spread(NSPEC, nt, False), spread(NGRID, nt, True), spread(NGRID, nt, False)
    # the spread the cases rely on: a task that is the source of nothing, one that is the source of a field of a V-set it is not in, one that
    # is the source of two fields; targets elsewhere
    vset_of = lambda task: (task - 1) % nprv + 1
    assert 1 not in kfrom_s and any(vset_of(kfrom_s[f]) != kv[f] for f in range(NSPEC)) and max(np.bincount(kfrom_s)) >= 2
    assert nt not in kto_s and (kfrom_s != kto_s).any()
    esz = T.dt.itemsize

    if "layout" in cases:  # 1 and 6: every path gives the expected bytes, hence the same bytes
        for path in PATHS:
            for kp in ((37,) if kinds == "sg" else (None,)):
                T.round_trip(path, kv, kfrom_s, kto_s, kfrom_g, kto_g, kp, "%s layout" % name, kinds)
    if "ksort" in cases:  # 2: a reversal of the local fields
        for path in PATHS[:2]:
            fl = T.local_fields(kv, NSPEC)
            mine = [f for f in range(NSPEC) if kfrom_s[f] == me]
            ks = np.arange(len(fl), 0, -1, dtype=np.int32)
            loc0 = np.full((T.ns2, len(fl)), np.nan, dtype=T.dt) if fl else None
            rc, msg, _, loc = T.move("spec", False, path, T.glob_of(mine, T.ns2g), loc0, NSPEC, kfrom_s, kv, ks if fl else None, None, "%s KSORT" % name)
            assert rc == 0, msg
            T.same(loc, T.want_spec(fl, list(ks - 1)) if fl else None, "%s DIST_SPEC KSORT %s" % (name, path[0]))
            if "g" in kinds:
                mine = [f for f in range(NGRID) if kfrom_g[f] == me]
                ks = np.arange(NGRID, 0, -1, dtype=np.int32)
                loc0 = np.full(((T.ng - 1) // 37 + 1, NGRID, 37), -777.0, dtype=T.dt)
                rc, msg, _, loc = T.move("grid", False, path, T.glob_of(mine, T.ngg), loc0, NGRID, kfrom_g, None, ks, 37, "%s KSORT" % name)
                assert rc == 0, msg
                T.same(loc, T.want_grid(list(range(NGRID)), 37, -777.0, list(ks - 1)), "%s DIST_GRID KSORT %s" % (name, path[0]))
    if "kproma" in cases and "g" in kinds:  # 3: 37 cuts the sub-band and its latitudes; 64; NGPTOT itself
        # a last block with padding: NGPTOT is no multiple of 37 -- but for task 5 of 2 x 3, whose sub-band has 444 = 12 x 37 points and
        # whose padded block is that of 64
        assert T.ng > 64 and (T.ng % 37 != 0 or (T.ng % 64 != 0 and (T.nt, T.me) == (6, 5))), T.ng
        for path in PATHS[:2]:
            for kp in (37, 64, T.ng):
                T.round_trip(path, kv, kfrom_s, kto_s, kfrom_g, kto_g, kp, "%s NPROMA %d" % (name, kp), "g")
    if "empty" in cases:  # 4: every field in the last V-set (the others pass no PSPEC and still take part); no field at all
        last = np.full(NSPEC, nprv, dtype=np.int32)
        for path in PATHS[:2]:
            T.round_trip(path, last, kfrom_s, kto_s, kfrom_g, kto_g, None, "%s last V-set only" % name, "s")
            for gath in (False, True):
                rc, msg, _, _ = T.move("spec", gath, path, None, None, 0, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), None, None, "no field")
                assert rc == 0, msg
                if "g" in kinds:
                    rc, msg, _, _ = T.move("grid", gath, path, None, None, 0, np.zeros(0, dtype=np.int32), None, None, None, "no field")
                    assert rc == 0, msg
    if "chunk" in cases:  # 5: two fields per chunk: the boundary after field 2 falls between two fields of V-set 2
        assert kv[1] == kv[2] or nprv == 3
        for path in PATHS[:2]:
            whole = T.round_trip(path, kv, kfrom_s, kto_s, kfrom_g, kto_g, 37 if "g" in kinds else None, "%s unchunked" % name, kinds)
            parts = []
            for kind, nglob in (("s", T.ns2g), ("g", T.ngg)):
                if kind in kinds:
                    os.environ["EMI_GATH_CHUNK"] = str(2 * nglob * esz + 8)
                    parts += T.round_trip(path, kv, kfrom_s, kto_s, kfrom_g, kto_g, 37, "%s chunked" % name, kind)
            os.environ["EMI_GATH_CHUNK"] = ""
            for a, b in zip(whole, parts):
                T.same(b, a, "%s chunked against unchunked %s" % (name, path[0]))
    if "transform" in cases and oracle is not None:  # 7
        transform_case(et, r, T, kv, oracle, dev_mem)
    if "refuse" in cases:  # 8
        refusals(T, kv, kfrom_s, kto_s, name)
        T.round_trip(PATHS[1], kv, kfrom_s, kto_s, kfrom_g, kto_g, None, "%s after the refusals" % name, "s")  # no task was left behind
    return T.bad


def transform_case(et, r, T, kv, oracle, dev_mem):
    """DIST_SPEC(KVSET) -> INV_TRANS(KVSETSC) -> GATH_GRID to task 1, against the oracle's inverse; DIST_GRID of the oracle's grid fields
    from task 1 -> DIR_TRANS -> GATH_SPEC(KVSET) to task 1, against the oracle's direct transform of them (the inputs of
    tests/vsets_worker.py, whose bound this is).  Host arrays and device-resident arrays, through the Python mirror."""
    o, n, prec = oracle, et.trans_inq(r, "nsmax"), T.dt.itemsize
    rng = np.random.default_rng(11)  # the same global fields on every task
    sc = random_spectrum(rng, o.nasm0, n, o.nspec2, NSPEC, False).astype(T.dt)
    gref = o.inv_trans(spsc=sc.astype(np.float64))
    gin = gref.astype(T.dt)
    sref = o.dir_trans(gin.astype(np.float64), nsc=NSPEC)[2]
    kfrom = spread(NSPEC, T.nt, True)
    fl = T.local_fields(kv, NSPEC)
    npr = 37
    nb = (T.ng - 1) // npr + 1
    back = lambda a: np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float64)
    for mem in ({}, {"mem_space": DEVICE}):
        to = (lambda a: dev_mem[0](np.ascontiguousarray(a).reshape(-1)).reshape(a.shape)) if mem else (lambda a: a)
        loc = et.dist_spec(r, sc if (kfrom == T.me).any() else None, NSPEC, kfrom, kvset=kv, **mem)
        assert tuple(loc.shape) == (T.ns2, len(fl))
        gp = to(np.zeros((nb, NSPEC, npr), dtype=T.dt))
        et.inv_trans(r, pspscalar=loc if fl else None, pgp=gp, kproma=npr, kvsetsc=kv)
        gg = et.gath_grid(r, gp, NSPEC, kto=1, **mem)
        gp2 = et.dist_grid(r, gin if T.me == 1 else None, NSPEC, kfrom=1, kproma=npr, **mem)
        s2 = to(np.zeros((T.ns2, len(fl)), dtype=T.dt)) if fl else None
        et.dir_trans(r, pspscalar=s2, pgp=gp2, kproma=npr, kvsetsc=kv)
        sg = et.gath_spec(r, s2, NSPEC, kto=1, kvset=kv, **mem)
        if T.me == 1:
            e_inv, e_dir = rel_err(back(gg), gref, axis=1), rel_err(back(sg), sref)
            print("transform %s: e_inv %.2e e_dir %.2e (bound %.0e)" % ("device" if mem else "host", e_inv, e_dir, TOL[prec]), flush=True)
            assert e_inv < TOL[prec] and e_dir < TOL[prec], (e_inv, e_dir)
        else:
            assert gg is None and sg is None


def refusals(T, kv, kfrom_s, kto_s, name):
    """argument errors, found on the host side before anything moves: every task of the call fails, with the reference's text where
    there is one, and none is left waiting in the exchange (the worker ends within its timeout)"""
    fl = T.local_fields(kv, NSPEC)
    loc = T.want_spec(fl) if fl else None
    g0 = np.full((NSPEC, T.ns2g), SENT, dtype=T.dt)
    over = kv.copy()
    over[3] = T.nprv + 1
    other = kv.copy()  # task 1 names other V-sets than the rest: fields 0 and 1 swapped
    if T.me == 1:
        other[0], other[1] = kv[1], kv[0]
    fl_o = T.local_fields(other, NSPEC)
    loc_o = T.want_spec(fl_o) if fl_o else None

    def refused(rc, msg, text, what):
        if rc == 0 or text not in msg:
            T.bad.append("%s %s: return code %d, message %r, expected %r" % (name, what, rc, msg, text))

    for path in PATHS[:2]:
        for gath, who, kt in ((True, "GATH_SPEC", kto_s), (False, "DIST_SPEC", kfrom_s)):
            l = loc if gath or loc is None else np.full_like(loc, np.nan)
            rc, msg, _, _ = T.move("spec", gath, path, g0, l, NSPEC, kt, None, None, None, "refusal")
            refused(rc, msg, "%s:KVSET MISSING, NPRTRV > 1" % who, "%s without KVSET, %s" % (who, path[0]))
            rc, msg, _, _ = T.move("spec", gath, path, g0, l, NSPEC, kt, over, None, None, "refusal")
            refused(rc, msg, "%s:KVSET CONTAINS VALUES OUTSIDE RANGE" % who, "%s with V-set NPRTRV + 1, %s" % (who, path[0]))
            lo = loc_o if gath or loc_o is None else np.full_like(loc_o, np.nan)
            rc, msg, _, _ = T.move("spec", gath, path, g0, lo, NSPEC, kt, other, None, None, "refusal")
            refused(rc, msg, "%s: KVSET DIFFERS BETWEEN TASKS" % who, "%s with another KVSET on task 1, %s" % (who, path[0]))
        # the first target passes no global array: it says so, the others name it
        t0 = int(kto_s[0])
        rc, msg, _, _ = T.move("spec", True, path, None if T.me == t0 else g0, loc, NSPEC, kto_s, kv, None, None, "refusal")
        refused(rc, msg, "passes no global array" if T.me == t0 else "TASK %d REFUSED ITS ARGUMENTS" % t0, "GATH_SPEC without PSPECG on task %d, %s" % (t0, path[0]))
    # the entry points without KVSET answer the same
    for nm, args in (("emi_gath_spec", (T.r, _ptr(g0), NSPEC, _ip(kto_s), _ptr(g0))), ("emi_dist_spec", (T.r, _ptr(g0), NSPEC, _ip(kfrom_s), None, _ptr(g0))),
                     ("emi_gath_spec_m", (T.r, HOST, _ptr(g0), NSPEC, _ip(kto_s), HOST, _ptr(g0)))):
        rc, msg = T.call(nm, *args)
        refused(rc, msg, "_SPEC:KVSET MISSING, NPRTRV > 1", nm)
    assert (g0 == SENT).all()  # nothing was written by a refused call


# ---- launching ---------------------------------------------------------------------------------------------------------------------------
def run_workers(nprw, nprv, where="cpu", precision=8, cases=None, timeout=600):
    """tests/vsets_gs_worker.py on nprw x nprv tasks over gloo, every launch under its own timeout; the tasks' output"""
    world = nprw * nprv
    assert world <= 6
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", WORLD_SIZE=str(world), EMI_TEST_NPRTRV=str(nprv), EMI_TEST_DEVICE=where,
               EMI_TEST_PRECISION=str(precision), EMI_GATH_CHUNK="")
    if cases:
        env["EMI_TEST_CASES"] = ",".join(cases)
    if where == "cpu":
        env["OMP_NUM_THREADS"] = "256"  # the emulator runs a workgroup's lanes as threads; the GPU tier leaves the setting alone
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        env["MASTER_PORT"] = str(s.getsockname()[1])
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "vsets_gs_worker.py")], env=dict(env, RANK=str(rank)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("VSETS GS OK rank %d of %d" % (rank, world)) in out, out
    return outs
