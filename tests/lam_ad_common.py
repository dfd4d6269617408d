"""One EINV_TRANSAD + EDIR_TRANSAD case through the Python mirror, compared element by element with the NumPy model of
tests/lam_ad_ref.py: shared by the emulator tier (tests/test_lam_ad_emu.py) and the GPU tier (tests/test_lam_ad_gpu.py)."""
import itertools
import math

import numpy as np

from tests.lam_ad_ref import LamAdRef
from tests.lam_common import blocked, unblocked, units

ALL = dict(scders=True, vorgp=True, divgp=True, uvder=True)
NONE = dict(scders=False, vorgp=False, divgp=False, uvder=False)
FLAG_COMBOS = [dict(zip(("scders", "vorgp", "divgp", "uvder"), c)) for c in itertools.product((False, True), repeat=4)]
TOL = {8: 1e-11, 4: 3e-5}  # of each output field's maximum: the bounds of tests/test_lam_gpu.py

FBK = 16  # fields per workgroup of the y-direction kernels on a short column (build_fft_plans: at most 16)
# (ndlon, ndgl, M, N, keywords of lam_ad_case)
CASES = {
    "ref_size": (20, 18, 9, 8, {}),                                     # the size of the reference's adjoint tests
    "prime_y": (36, 23, 11, 10, {}),                                    # NDGL = 23: Bluestein in y
    "prime_x": (37, 24, 12, 11, {}),                                    # NDLON = 37: Bluestein in x
    "m_zero": (128, 96, 0, 31, {}),
    "n_zero": (128, 96, 42, 0, {}),
    "atoms_meet_chunks": (20, 18, 9, 8, dict(nuv=3, nsc=2 * FBK + 1)),   # 4-field wind atoms, 2-field scalar atoms, chunks of 16
    "atoms_of_three": (20, 18, 9, 8, dict(nuv=3, nsc=2 * FBK + 1, flags=dict(scders=True, vorgp=False, divgp=True, uvder=True))),
    "no_flags_odd_counts": (20, 18, 9, 8, dict(nuv=3, nsc=2 * FBK + 1, flags=NONE)),
    "call_mode_2": (36, 23, 11, 10, dict(split=True, nproma=100)),      # PGPUV / PGP2 / PGP3A / PGP3B; NPROMA cuts rows, padded
    "call_mode_2_no_flags": (37, 24, 12, 11, dict(split=True, nproma=77, flags=NONE)),
    "nproma_padded": (20, 18, 9, 8, dict(nproma=77)),
    "in_place": (36, 23, 11, 10, dict(mem_space=1)),                     # EMI_MEM_DEVICE: arrays used in place
    "in_place_call_mode_2": (20, 18, 9, 8, dict(mem_space=1, split=True, nproma=64)),
    "scalars_only": (20, 18, 9, 8, dict(nuv=0)),
    "wind_only": (20, 18, 9, 8, dict(nsc=0)),
}


def flag_id(f):
    return "".join(k[0] if v else "-" for k, v in f.items())


def grid_groups(nuv, nsc, flags):
    """[(name, count)] of the grid fields of EINV_TRANS / EINV_TRANSAD in their order in PGP"""
    vorgp, divgp = flags["vorgp"], flags["divgp"] or flags["vorgp"]
    return ([("vor", nuv)] if vorgp and nuv else []) + ([("div", nuv)] if divgp and nuv else []) + ([("u", nuv), ("v", nuv)] if nuv else []) + \
        ([("sc", nsc)] if nsc else []) + ([("nsd", nsc)] if flags["scders"] and nsc else []) + \
        ([("uew", nuv), ("vew", nuv)] if flags["uvder"] and nuv else []) + ([("scew", nsc)] if flags["scders"] and nsc else [])


def pack_grid(grp, nuv, nsc, flags, split, nproma, dt, pad):
    """{name: (count, ngptot)} -> the grid keywords of the call (numpy, padding of the last NPROMA block = pad).  split: PGPUV, PGP2
    (scalar 0), PGP3A (scalars 1..4 as 2 variables x 2 levels), PGP3B (scalar 5)."""
    def blk(fields):
        a = blocked(fields, nproma, dt)
        a[a == -777.0] = pad
        return a
    names = [nm for nm, _ in grid_groups(nuv, nsc, flags)]
    if not split:
        return dict(pgp=blk(np.concatenate([grp[nm] for nm in names])))
    nb = (grp[names[0]].shape[1] - 1) // nproma + 1
    out = {}
    uvn = [nm for nm in names if nm in ("vor", "div", "u", "v", "uew", "vew")]
    if uvn:
        out["pgpuv"] = blk(np.concatenate([grp[nm] for nm in uvn])).reshape(nb, len(uvn), nuv, nproma)
    ders = [nm for nm in names if nm in ("sc", "nsd", "scew")]
    out["pgp2"] = blk(np.concatenate([grp[nm][0:1] for nm in ders]))
    out["pgp3a"] = blk(np.concatenate([grp[nm][1:5] for nm in ders])).reshape(nb, 2 * len(ders), 2, nproma)
    out["pgp3b"] = blk(np.concatenate([grp[nm][5:6] for nm in ders])).reshape(nb, len(ders), 1, nproma)
    return out


def unpack_grid(arrs, nuv, nsc, flags, split, npt):
    """the inverse of pack_grid, on host arrays -> {name: (count, ngptot)}"""
    names = grid_groups(nuv, nsc, flags)
    grp = {}
    if not split:
        g, pos = unblocked(arrs["pgp"], npt), 0
        for nm, cnt in names:
            grp[nm] = g[pos:pos + cnt]
            pos += cnt
        return grp
    flat = lambda a: unblocked(a.reshape(a.shape[0], -1, a.shape[-1]), npt)
    uvn = [nm for nm, _ in names if nm in ("vor", "div", "u", "v", "uew", "vew")]
    if uvn:
        g = flat(arrs["pgpuv"])
        for k, nm in enumerate(uvn):
            grp[nm] = g[k * nuv:(k + 1) * nuv]
    ders = [nm for nm, _ in names if nm in ("sc", "nsd", "scew")]
    g2, g3a, g3b = flat(arrs["pgp2"]), flat(arrs["pgp3a"]), flat(arrs["pgp3b"])
    for k, nm in enumerate(ders):
        grp[nm] = np.concatenate([g2[k:k + 1], g3a[4 * k:4 * k + 4], g3b[k:k + 1]])
    return grp


def pack_spec(vor, div, sc, mu, mv, split, dt):
    """the spectral keywords of a call (numpy); split: PSPSC2, PSPSC3A (nvar, nspec2, nlev), PSPSC3B in place of PSPSCALAR"""
    C = lambda a: np.ascontiguousarray(a, dtype=dt)
    out = dict(pspvor=C(vor), pspdiv=C(div), pmeanu=C(mu), pmeanv=C(mv)) if vor is not None else {}
    if sc is None:
        return out
    if not split:
        out["pspscalar"] = C(sc)
    else:
        out.update(pspsc2=C(sc[:, 0:1]), pspsc3a=C(np.stack([sc[:, 1:3], sc[:, 3:5]])), pspsc3b=C(sc[None, :, 5:6]))
    return out


def unpack_spec(arrs, split):
    """-> vor, div, sc, mu, mv as float64 host arrays (None where absent)"""
    H = lambda k: np.asarray(arrs[k], dtype=np.float64) if k in arrs else None
    if split:
        s3a = H("pspsc3a")
        sc = np.concatenate([H("pspsc2"), s3a[0], s3a[1], H("pspsc3b")[0]], axis=1)
    else:
        sc = H("pspscalar")
    return H("pspvor"), H("pspdiv"), sc, H("pmeanu"), H("pmeanv")


def lam_ad_case(et, ndlon, ndgl, M, N, nuv=2, nsc=3, flags=ALL, split=False, nproma=None, precision=8, mem_space=None, seed=17,
                to_dev=None, to_host=None, kresol=None, which=("inv", "dir")):
    """Both adjoints against the model.  Returns errs: label -> the largest error of its fields relative to each field's maximum in
    the model (the means: relative to the largest coefficient of the wind); NaN in an output counts as infinite.  Asserts: inputs
    bit-identical after the call, outputs (pre-filled with NaN) fully defined, exact zeros in the structural entries, the padding of
    the last NPROMA block not written.
    EINV_TRANSAD: white grid fields, U(-1, 1) in every point, NaN in the NPROMA padding.  EDIR_TRANSAD: U(-0.5, 0.5) in every spectral
    entry that enters, NaN in the entries that EDIR_TRANS writes as structural zeros."""
    dt = np.float64 if precision == 8 else np.float32
    to_dev = to_dev or (lambda a: a)
    to_host = to_host or (lambda a: a)
    exwn, eywn = units(ndlon, ndgl)
    ref = LamAdRef(ndlon, ndgl, M, N, exwn, eywn)
    r = kresol if kresol is not None else et.esetup_trans(M, N, ndgl, kdlon=ndlon, pexwn=exwn, peywn=eywn, precision=precision)
    try:
        assert et.etrans_inq(r, "nspec2") == ref.nspec2 and et.etrans_inq(r, "ngptot") == ref.ngptot
        npt = ref.ngptot
        nproma = nproma or npt
        if split:
            nsc = 6
        rng = np.random.default_rng(seed)
        rnd = lambda a: a.astype(dt).astype(np.float64)
        dev = lambda kw: {k: to_dev(v) for k, v in kw.items()}
        host = lambda kw: {k: np.asarray(to_host(v)) for k, v in kw.items()}
        nanspec = lambda *sh: np.full(sh, np.nan)
        lflags = {"ld" + k: v for k, v in flags.items()}
        errs = {}

        def cmp(label, got, want, scale=None):
            for f in range(want.shape[0]):
                e = float(np.abs(got[f] - want[f]).max() / (scale or max(np.abs(want[f]).max(), 1e-300)))
                errs[label] = max(errs.get(label, 0.0), e if np.isfinite(e) else np.inf)

        same = lambda a, b: all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
        if "inv" in which:
            names = grid_groups(nuv, nsc, flags)
            grp = {nm: rnd(rng.uniform(-1.0, 1.0, (cnt, npt))) for nm, cnt in names}
            g_h = pack_grid(grp, nuv, nsc, flags, split, nproma, dt, np.nan)
            g_d = dev(g_h)
            sp_d = dev(pack_spec(nanspec(ref.nspec2, nuv) if nuv else None, nanspec(ref.nspec2, nuv), nanspec(ref.nspec2, nsc) if nsc else None,
                                 nanspec(nuv), nanspec(nuv), split, dt))
            et.einv_transad(r, kproma=nproma, mem_space=mem_space, **g_d, **sp_d, **lflags)
            assert same(host(g_d), g_h), "EINV_TRANSAD changed its input"
            vor, div, sc, mu, mv = unpack_spec(host(sp_d), split)
            gin = np.concatenate([grp[nm] for nm, _ in names]).reshape(-1, ndgl, ndlon)
            rv, rd, rs, rmu, rmv = ref.inv_transad(gin, nuv=nuv, nsc=nsc, **flags)
            if nsc:
                cmp("invad sc", sc.T, rs.T)
                assert np.array_equal(ref.clean(sc), sc), "structural zeros of sc"
            if nuv:
                cmp("invad vor", vor.T, rv.T)
                cmp("invad div", div.T, rd.T)
                cmp("invad mean", np.stack([mu, mv]), np.stack([rmu, rmv]), scale=ref.wind_max)
                assert np.array_equal(ref.clean(vor), vor) and np.array_equal(ref.clean(div), div), "structural zeros of vor, div"
        if "dir" in which:
            def spec(nf):  # NaN where EDIR_TRANS writes structural zeros
                sp = rnd(rng.uniform(-0.5, 0.5, (ref.nspec2, nf)))
                return np.where(ref.clean(np.ones((ref.nspec2, nf))) == 0.0, np.nan, sp)
            vor, div = (spec(nuv), spec(nuv)) if nuv else (None, None)
            sc = spec(nsc) if nsc else None
            mu, mv = rnd(rng.uniform(-3, 3, nuv)), rnd(rng.uniform(-3, 3, nuv))
            sp_h = pack_spec(vor, div, sc, mu, mv, split, dt)
            sp_d = dev(sp_h)
            names = grid_groups(nuv, nsc, NONE)
            g_d = dev(pack_grid({nm: np.full((cnt, npt), np.nan) for nm, cnt in names}, nuv, nsc, NONE, split, nproma, dt, np.nan))
            et.edir_transad(r, kproma=nproma, mem_space=mem_space, **sp_d, **g_d)
            assert same(host(sp_d), sp_h), "EDIR_TRANSAD changed its input"
            g_o = host(g_d)
            got = unpack_grid(g_o, nuv, nsc, NONE, split, npt)
            z = lambda a: None if a is None else np.nan_to_num(a, nan=0.0)
            want = ref.dir_transad(z(vor), z(div), z(sc), mu, mv).reshape(-1, npt)
            pos = 0
            for nm, cnt in names:
                cmp("dirad " + nm, got[nm], want[pos:pos + cnt])
                pos += cnt
            nb = (npt - 1) // nproma + 1
            if nb * nproma > npt:
                assert all(np.all(np.isnan(a[-1, ..., npt - (nb - 1) * nproma:])) for a in g_o.values()), "NPROMA padding written"
        return errs
    finally:
        if kresol is None:
            et.trans_release(r)


def fdot(*pairs):
    """sum over the pairs (x, y) of <x, y>, accumulated with math.fsum in double"""
    return math.fsum(float(p) for x, y in pairs for p in (np.asarray(x, dtype=np.float64).ravel() * np.asarray(y, dtype=np.float64).ravel()))


def dot_identities(et, ndlon, ndgl, M, N, nuv=2, nsc=3, flags=ALL, precision=8, seed=23, to_dev=None, to_host=None):
    """<y, EINV_TRANS x> against <EINV_TRANSAD y, x>, and the same for the direct pair, the means among the spectral entries, through the
    library alone.  Returns the two relative differences |l - r| / max(|l|, |r|)."""
    dt = np.float64 if precision == 8 else np.float32
    to_dev = to_dev or (lambda a: a)
    to_host = to_host or (lambda a: a)
    exwn, eywn = units(ndlon, ndgl)
    ref = LamAdRef(ndlon, ndgl, M, N, exwn, eywn)
    r = et.esetup_trans(M, N, ndgl, kdlon=ndlon, pexwn=exwn, peywn=eywn, precision=precision)
    try:
        npt, ns2 = ref.ngptot, ref.nspec2
        rng = np.random.default_rng(seed)
        C = lambda a: to_dev(np.ascontiguousarray(a, dtype=dt))
        H = lambda a: np.asarray(to_host(a), dtype=np.float64)
        Z = lambda *sh: to_dev(np.zeros(sh, dtype=dt))
        lflags = {"ld" + k: v for k, v in flags.items()}
        nf = sum(c for _, c in grid_groups(nuv, nsc, flags))
        out = []
        # ---- the inverse pair
        x = dict(pspvor=C(ref.random_spec(rng, nuv, wind=True)), pspdiv=C(ref.random_spec(rng, nuv, wind=True)), pspscalar=C(ref.random_spec(rng, nsc)),
                 pmeanu=C(rng.uniform(-3, 3, nuv)), pmeanv=C(rng.uniform(-3, 3, nuv)))
        y = C(rng.uniform(-1, 1, (1, nf, npt)))
        ax = Z(1, nf, npt)
        et.einv_trans(r, pgp=ax, **x, **lflags)
        aty = dict(pspvor=Z(ns2, nuv), pspdiv=Z(ns2, nuv), pspscalar=Z(ns2, nsc), pmeanu=Z(nuv), pmeanv=Z(nuv))
        et.einv_transad(r, pgp=y, **aty, **lflags)
        lhs, rhs = fdot((H(y), H(ax))), fdot(*[(H(aty[k]), H(x[k])) for k in x])
        out.append(abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
        # ---- the direct pair
        g = C(rng.uniform(-1, 1, (1, 2 * nuv + nsc, npt)))
        bg = dict(pspvor=Z(ns2, nuv), pspdiv=Z(ns2, nuv), pspscalar=Z(ns2, nsc), pmeanu=Z(nuv), pmeanv=Z(nuv))
        et.edir_trans(r, pgp=g, **bg)
        s = dict(pspvor=C(rng.uniform(-0.5, 0.5, (ns2, nuv))), pspdiv=C(rng.uniform(-0.5, 0.5, (ns2, nuv))), pspscalar=C(rng.uniform(-0.5, 0.5, (ns2, nsc))),
                 pmeanu=C(rng.uniform(-3, 3, nuv)), pmeanv=C(rng.uniform(-3, 3, nuv)))
        bts = Z(1, 2 * nuv + nsc, npt)
        et.edir_transad(r, pgp=bts, **s)
        lhs, rhs = fdot(*[(H(s[k]), H(bg[k])) for k in s]), fdot((H(bts), H(g)))
        out.append(abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
        return out
    finally:
        et.trans_release(r)
