"""The limited-area part of the transi-style C layer, shared by the emulator tier (tests/test_transi_lam_emu.py) and the GPU tier
(tests/test_transi_lam_gpu.py).  The Python test writes the global inputs of one domain as raw doubles, tests/transi/transi_test_lam.c
reads them, calls transi and writes what it got, and the test compares that
  - byte for byte with the same calls through the Python mirror on the same library (transi adds no arithmetic),
  - with the NumPy models of tests/lam_ref.py / tests/lam_ad_ref.py / tests/lam_norm_ref.py at the tolerances of their own tests,
  - on the 54 x 48 domain with the reference's known-answer pair (tests/golden/antwrp1300) at its 1e-10 absolute."""
import os
import subprocess

import numpy as np

from tests import lam_norm_ref as nr
from tests.lam_ad_ref import LamAdRef
from tests.lam_common import blocked, unblocked, units

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "antwrp1300")
# (nx, ny, dx, dy, trunc_x, trunc_y, nproma): the reference test's shape with dx /= dy; the golden pair's domain; a column of 22 rows,
# which is not 2 3 5 7-smooth (the convolution path in y).  NPROMA never divides the point count: the last block is ragged.
DOMAINS = {
    "ref_20x18": (20, 18, 2500.0, 1300.0, 9, 8, 77),
    "antwrp_54x48": (54, 48, 1300.0, 1300.0, 26, 23, 100),
    "conv_24x22": (24, 22, 1300.0, 2000.0, 11, 10, 50),
}
NUV, NSC = 2, 3
MASKS = (0, 7, 1, 6)  # bit 0: lscalarders, bit 1: luvder_EW, bit 2: lvordivgp
AD_MASKS = (0, 7)
EPSILON = 1e-10       # absolute, the golden pair
U52 = 2.0 ** -52      # the norms: tests/lam_norms_common.py


def flags_of(mask):
    return dict(scders=bool(mask & 1), uvder=bool(mask & 2), vorgp=bool(mask & 4), divgp=bool(mask & 4))


def nfld_of(mask):
    return 2 * NUV + NSC + (2 * NSC if mask & 1 else 0) + (2 * NUV if mask & 2 else 0) + (2 * NUV if mask & 4 else 0)


def make_inputs(name):
    """the global inputs of a domain (one task: global == local), as {file stem: float64 array}, and the model"""
    nx, ny, dx, dy, mx, my, nproma = DOMAINS[name]
    exwn, eywn = units(nx, ny, dx, dy)
    ref = LamAdRef(nx, ny, mx, my, exwn, eywn)
    rng = np.random.default_rng(11)
    inp = dict(vor=ref.random_spec(rng, NUV, wind=True), div=ref.random_spec(rng, NUV, wind=True), sc=ref.random_spec(rng, NSC),
               mu=rng.uniform(-3, 3, NUV), mv=rng.uniform(-3, 3, NUV))
    if name == "antwrp_54x48":
        inp["sc"][:, 0] = np.load(os.path.join(GOLD, "antwrp1300-s1t@sp.npy"))
    inp["gp"] = ref.inv_trans(inp["vor"], inp["div"], inp["sc"], inp["mu"], inp["mv"]).reshape(-1, ref.ngptot)  # u, v, scalars
    if name == "antwrp_54x48":
        inp["gp"][2 * NUV] = np.load(os.path.join(GOLD, "antwrp1300-s1t@sp2gp.npy")).ravel()
    for mask in AD_MASKS:
        inp["gpad_%d" % mask] = rng.uniform(-1.0, 1.0, (nfld_of(mask), ref.ngptot))
    met = rng.uniform(0.5, 2.0, nr.pmet_size(ref.kntmp))
    met[0] = np.nan  # element 0 is never read
    inp["rmet"] = met
    return ref, {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in inp.items()}


def run_program(exe, name, outdir, inp, memory="host", launcher=(), env=None, marker_count=1):
    nx, ny, dx, dy, mx, my, nproma = DOMAINS[name]
    os.makedirs(outdir, exist_ok=True)
    for k, v in inp.items():
        v.tofile(os.path.join(outdir, k + ".f64"))
    cmd = list(launcher) + [exe, outdir, str(nx), str(ny), repr(dx), repr(dy), str(mx), str(my), str(NUV), str(NSC), str(nproma), memory]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and p.stdout.count("TRANSI LAM OK") == marker_count and "TRANSI LAM REFUSALS OK" in p.stdout, p.stdout + p.stderr
    for text in ("trans_setup: ERROR: nmsmax < 0", "readfp is not available on a limited-area handle", "rgw is a quantity of the Gaussian grid",
                 "trans_invtrans: ERROR: Array RMEANU was not allocated", "trans_dirtrans: ERROR: Array RMEANV was not allocated",
                 "mvalue is a quantity of a limited-area handle"):
        assert text in p.stderr, (text, p.stderr)
    return read_outputs(outdir, inp)


def read_outputs(outdir, inp):
    ld = lambda fn, dt=np.float64: np.fromfile(os.path.join(outdir, fn), dtype=dt)
    out = {"sizes": ld("sizes.i32", np.int32)}
    ns2g, ngg = int(out["sizes"][1]), int(out["sizes"][5])
    for k in ("nvalue", "mvalue", "nmyms", "nloen"):
        out[k] = ld(k + ".i32", np.int32)
    for mask in MASKS:
        out["inv_%d" % mask] = ld("inv_%d.f64" % mask).reshape(nfld_of(mask), ngg)
    if os.path.exists(os.path.join(outdir, "invg_7.f64")):
        out["invg_7"] = ld("invg_7.f64").reshape(nfld_of(7), ngg)
    for stem in ["dir"] + ["invad_%d" % m for m in AD_MASKS]:
        fn = lambda w: "%s_%s.f64" % (stem, w)
        out[stem] = dict(vor=ld(fn("vor")).reshape(ns2g, NUV), div=ld(fn("div")).reshape(ns2g, NUV), sc=ld(fn("sc")).reshape(ns2g, NSC),
                         mu=ld(fn("mu")), mv=ld(fn("mv")))
    out["dirad"] = ld("dirad.f64").reshape(nfld_of(0), ngg)
    out["norm"], out["norm_met"] = ld("norm.f64"), ld("norm_met.f64")
    return out


def mirror(et, name, inp):
    """the same calls through the Python mirror, one task, host arrays, the same NPROMA blocks: outputs in the layout of read_outputs"""
    nx, ny, dx, dy, mx, my, nproma = DOMAINS[name]
    exwn, eywn = units(nx, ny, dx, dy)
    r = et.esetup_trans(mx, my, ny, kdlon=nx, pexwn=exwn, peywn=eywn)
    try:
        q = lambda n: et.etrans_inq(r, n)
        npt, ns2 = q("ngptot"), q("nspec2")
        nb = (npt - 1) // nproma + 1
        out = {"sizes": np.array([q(n) for n in ("nspec2", "nspec2g", "nspec2mx", "nump", "ngptot", "ngptotg", "ngptotmx", "nproc", "myproc", "ndgux")] +
                                 [ns2 // 2, 1], dtype=np.int32)}
        myms, kntmp = q("myms"), q("kntmp")
        out["nmyms"] = np.asarray(myms, dtype=np.int32)
        out["nvalue"] = np.array([n for m in myms for n in range(kntmp[m] + 1) for _ in range(4)], dtype=np.int32)
        out["mvalue"] = np.array([m for m in myms for n in range(kntmp[m] + 1) for _ in range(4)], dtype=np.int32)
        out["nloen"] = np.full(ny, nx, dtype=np.int32)
        spec = dict(pspvor=inp["vor"], pspdiv=inp["div"], pspscalar=inp["sc"], pmeanu=inp["mu"], pmeanv=inp["mv"])
        nanpad = lambda f: np.where(blocked(f, nproma, np.float64) == -777.0, np.nan, blocked(f, nproma, np.float64))
        for mask in MASKS:
            pgp = np.full((nb, nfld_of(mask), nproma), np.nan)
            et.einv_trans(r, pgp=pgp, kproma=nproma, **spec, **{"ld" + k: v for k, v in flags_of(mask).items()})
            out["inv_%d" % mask] = unblocked(pgp, npt)
        nspec = lambda: dict(pspvor=np.full((ns2, NUV), np.nan), pspdiv=np.full((ns2, NUV), np.nan), pspscalar=np.full((ns2, NSC), np.nan),
                             pmeanu=np.full(NUV, -777.0), pmeanv=np.full(NUV, -777.0))
        short = lambda o: dict(vor=o["pspvor"], div=o["pspdiv"], sc=o["pspscalar"], mu=o["pmeanu"], mv=o["pmeanv"])
        o = nspec()
        et.edir_trans(r, pgp=nanpad(inp["gp"]), kproma=nproma, **o)
        out["dir"] = short(o)
        for mask in AD_MASKS:
            o = nspec()
            et.einv_transad(r, pgp=nanpad(inp["gpad_%d" % mask]), kproma=nproma, **o, **{"ld" + k: v for k, v in flags_of(mask).items()})
            out["invad_%d" % mask] = short(o)
        pgp = np.full((nb, nfld_of(0), nproma), np.nan)
        et.edir_transad(r, pgp=pgp, kproma=nproma, **spec)
        out["dirad"] = unblocked(pgp, npt)
        out["norm"], out["norm_met"] = et.especnorm(r, inp["sc"]), et.especnorm(r, inp["sc"], inp["rmet"])
        return out
    finally:
        et.trans_release(r)


def same_bytes(a, b, what=""):
    """every entry of two output sets, byte for byte (invg_7, which the mirror has no call for, against inv_7)"""
    for k, v in a.items():
        w = b["inv_7"] if k == "invg_7" and k not in b else b[k]
        if isinstance(v, dict):
            for kk in v:
                assert np.asarray(v[kk]).tobytes() == np.asarray(w[kk]).tobytes(), (what, k, kk)
        else:
            assert np.ascontiguousarray(v).tobytes() == np.ascontiguousarray(w).tobytes(), (what, k)


def against_models(name, ref, inp, out, tol):
    """(c), (d), (f): the program's outputs against the models; tol: of each field's maximum"""
    npt = ref.ngptot
    errs = {}

    def cmp(label, got, want, scale=None):
        for f in range(want.shape[0]):
            e = float(np.abs(got[f] - want[f]).max() / (scale or max(np.abs(want[f]).max(), 1e-300)))
            errs[label] = max(errs.get(label, 0.0), e if np.isfinite(e) else np.inf)

    for mask in MASKS:
        want = ref.inv_trans(inp["vor"], inp["div"], inp["sc"], inp["mu"], inp["mv"], **flags_of(mask)).reshape(-1, npt)
        cmp("inv %d" % mask, out["inv_%d" % mask], want)
    rv, rd, rs, rmu, rmv = ref.dir_trans(inp["gp"].reshape(-1, ref.ndgl, ref.ndlon), nuv=NUV, nsc=NSC)
    d = out["dir"]
    cmp("dir vor", d["vor"].T, rv.T), cmp("dir div", d["div"].T, rd.T), cmp("dir sc", d["sc"].T, rs.T)
    cmp("dir mean", np.stack([d["mu"], d["mv"]]), np.stack([rmu, rmv]), scale=float(np.abs(inp["gp"][:2 * NUV]).max()))
    for k in ("vor", "div", "sc"):
        assert np.array_equal(ref.clean(d[k]), d[k]), "structural zeros of " + k
    for mask in AD_MASKS:
        rv, rd, rs, rmu, rmv = ref.inv_transad(inp["gpad_%d" % mask].reshape(-1, ref.ndgl, ref.ndlon), nuv=NUV, nsc=NSC, **flags_of(mask))
        a = out["invad_%d" % mask]
        cmp("invad %d vor" % mask, a["vor"].T, rv.T), cmp("invad %d div" % mask, a["div"].T, rd.T), cmp("invad %d sc" % mask, a["sc"].T, rs.T)
        cmp("invad %d mean" % mask, np.stack([a["mu"], a["mv"]]), np.stack([rmu, rmv]), scale=ref.wind_max)
    want = ref.dir_transad(inp["vor"], inp["div"], inp["sc"], inp["mu"], inp["mv"]).reshape(-1, npt)
    cmp("dirad", out["dirad"], want)
    print(name, {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < tol, errs
    # the norms: the bounds of tests/lam_norms_common.py
    for k, met in (("norm", None), ("norm_met", inp["rmet"])):
        want = nr.spec_norm(ref, inp["sc"], met)
        e = float(np.max(np.abs(out[k] - want) / want))
        assert e <= ref.nspec2g * U52, (k, e)
    if name == "antwrp_54x48":  # (d) the reference's known-answer pair, both ways
        sp, gp = np.load(os.path.join(GOLD, "antwrp1300-s1t@sp.npy")), np.load(os.path.join(GOLD, "antwrp1300-s1t@sp2gp.npy")).ravel()
        e_inv, e_dir = np.abs(out["inv_0"][2 * NUV] - gp).max(), np.abs(out["dir"]["sc"][:, 0] - sp).max()
        print("golden pair through transi: inverse %.2e direct %.2e" % (e_inv, e_dir))
        assert e_inv < EPSILON and e_dir < EPSILON
