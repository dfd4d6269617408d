"""One EINV_TRANS + EDIR_TRANS case through the Python mirror, compared with the NumPy model of tests/lam_ref.py: shared by the
emulator tier (tests/test_lam_emu.py) and the GPU tier (tests/test_lam_gpu.py)."""
import numpy as np

from tests.lam_ref import LamRef

DX = 1300.0  # grid spacing of the golden pair (m); the wavenumber units follow ectrans4py: 2 pi / (n dx)


def units(ndlon, ndgl, dx=DX, dy=DX):
    return 2.0 * np.pi / (ndlon * dx), 2.0 * np.pi / (ndgl * dy)


def blocked(fields, nproma, dtype):
    """(nf, ngptot) -> PGP(nproma, nf, ngpblks) as the (ngpblks, nf, nproma) array of the Python mirror, padding = -777"""
    nf, npt = fields.shape
    nb = (npt - 1) // nproma + 1
    out = np.full((nb, nf, nproma), -777.0, dtype=dtype)
    for f in range(nf):
        flat = np.full(nb * nproma, -777.0, dtype=dtype)
        flat[:npt] = fields[f]
        out[:, f, :] = flat.reshape(nb, nproma)
    return out


def unblocked(arr, npt):
    """(ngpblks, nf, nproma) -> (nf, ngptot)"""
    nb, nf, nproma = arr.shape
    return np.ascontiguousarray(np.transpose(arr, (1, 0, 2)).reshape(nf, nb * nproma)[:, :npt])


def lam_case(et, ndlon, ndgl, M, N, nuv=2, nsc=3, split=False, nproma=None, precision=8, mem_space=None, seed=3, flags=True,
             to_dev=None, to_host=None, kresol=None):
    """Runs both directions; returns (errs, outputs): errs maps a label to the largest error of its fields relative to each field's
    maximum in the model.  split: PGPUV / PGP2 / PGP3A / PGP3B and PSPSC2 / PSPSC3A / PSPSC3B (nsc is then 1 + 2 x 2 + 1 = 6) in place
    of PGP and PSPSCALAR.  to_dev / to_host: numpy <-> the array type handed to the library (torch device tensors on the GPU tier)."""
    dt = np.float64 if precision == 8 else np.float32
    to_dev = to_dev or (lambda a: a)
    to_host = to_host or (lambda a: a)
    exwn, eywn = units(ndlon, ndgl)
    ref = LamRef(ndlon, ndgl, M, N, exwn, eywn)
    r = kresol if kresol is not None else et.esetup_trans(M, N, ndgl, kdlon=ndlon, pexwn=exwn, peywn=eywn, precision=precision)
    assert et.etrans_inq(r, "nspec2") == ref.nspec2 and et.etrans_inq(r, "ngptot") == ref.ngptot
    npt = ref.ngptot
    nproma = nproma or npt
    rng = np.random.default_rng(seed)
    if split:
        nsc = 6
    rnd = lambda a: a.astype(dt).astype(np.float64)  # inputs rounded to the library precision
    vor, div, sc = rnd(ref.random_spec(rng, nuv, wind=True)), rnd(ref.random_spec(rng, nuv, wind=True)), rnd(ref.random_spec(rng, nsc))
    mu, mv = rnd(rng.uniform(-3, 3, nuv)), rnd(rng.uniform(-3, 3, nuv))
    kw = dict(scders=flags, vorgp=flags, divgp=flags, uvder=flags)
    g = ref.inv_trans(vor if nuv else None, div if nuv else None, sc, mu, mv, **kw).reshape(-1, npt)
    # the model's fields by group, in INV_TRANS order
    grp, pos = {}, 0
    names = ([("vor", nuv), ("div", nuv)] if flags and nuv else []) + ([("u", nuv), ("v", nuv)] if nuv else []) + [("sc", nsc)] + \
        ([("nsd", nsc)] if flags else []) + ([("uew", nuv), ("vew", nuv)] if flags and nuv else []) + ([("scew", nsc)] if flags else [])
    for nm, cnt in names:
        grp[nm] = g[pos:pos + cnt]
        pos += cnt
    assert pos == g.shape[0]
    lflags = dict(ldscders=flags, ldvorgp=flags, lddivgp=flags, lduvder=flags)
    C = lambda a: to_dev(np.ascontiguousarray(a, dtype=dt))
    sp_in = dict(pspvor=C(vor), pspdiv=C(div), pmeanu=C(mu), pmeanv=C(mv)) if nuv else {}
    dmul = 3 if flags else 1
    nb = (npt - 1) // nproma + 1
    Z = lambda *shape: to_dev(np.full(shape, -777.0, dtype=dt))
    errs = {}

    def cmp(label, got, want):
        for f in range(want.shape[0]):  # NaN in the output counts as infinite
            e = float(np.abs(got[f] - want[f]).max() / max(np.abs(want[f]).max(), 1e-300))
            errs[label] = max(errs.get(label, 0.0), e if np.isfinite(e) else np.inf)

    if not split:
        sp_in["pspscalar"] = C(sc)
        pgp = Z(nb, g.shape[0], nproma)
        et.einv_trans(r, pgp=pgp, kproma=nproma, mem_space=mem_space, **sp_in, **lflags)
        got = unblocked(to_host(pgp), npt)
        pos = 0
        for nm, cnt in names:
            cmp("inv " + nm, got[pos:pos + cnt], grp[nm])
            pos += cnt
        if nb * nproma > npt:  # the padding of the last block is not written
            assert np.all(to_host(pgp)[-1, :, npt - (nb - 1) * nproma:] == -777.0)
        gin_h = blocked(np.concatenate(([grp["u"], grp["v"]] if nuv else []) + [grp["sc"]]), nproma, dt)
        gin_h[gin_h == -777.0] = np.nan  # a Fortran caller leaves the padding of the last block uninitialised: it must not be read
        dir_in = dict(pgp=to_dev(gin_h))
        sp_out = dict(pspscalar=Z(ref.nspec2, nsc))
    else:
        # scalars in the order PSPSC2 (1), PSPSC3A (2 variables x 2 levels, variable outer), PSPSC3B (1 x 1)
        sp_in["pspsc2"] = C(sc[:, 0:1])
        sp_in["pspsc3a"] = C(np.stack([sc[:, 1:3], sc[:, 3:5]]))  # (nvar, nspec2, nlev)
        sp_in["pspsc3b"] = C(sc[None, :, 5:6])
        nvar_uv = (2 + (4 if flags else 0)) if nuv else 0
        out = dict(pgp2=Z(nb, 1 * dmul, nproma), pgp3a=Z(nb, 2 * dmul, 2, nproma), pgp3b=Z(nb, 1 * dmul, 1, nproma))
        if nuv:
            out["pgpuv"] = Z(nb, nvar_uv, nuv, nproma)
        et.einv_trans(r, kproma=nproma, mem_space=mem_space, **sp_in, **out, **lflags)
        flat = lambda a: np.transpose(a.reshape(nb, -1, nproma), (1, 0, 2)).reshape(-1, nb * nproma)[:, :npt]
        if nuv:
            uvn = (["vor", "div"] if flags else []) + ["u", "v"] + (["uew", "vew"] if flags else [])
            guv = flat(to_host(out["pgpuv"]))
            for k, nm in enumerate(uvn):
                cmp("inv " + nm, guv[k * nuv:(k + 1) * nuv], grp[nm])
        ders = ["sc", "nsd", "scew"] if flags else ["sc"]
        g2, g3a, g3b = flat(to_host(out["pgp2"])), flat(to_host(out["pgp3a"])), flat(to_host(out["pgp3b"]))
        for k, nm in enumerate(ders):
            cmp("inv2 " + nm, g2[k:k + 1], grp[nm][0:1])
            cmp("inv3a " + nm, g3a[4 * k:4 * k + 4], grp[nm][1:5])
            cmp("inv3b " + nm, g3b[k:k + 1], grp[nm][5:6])
        z0 = lambda a: np.where(a == -777.0, np.nan, a).astype(dt)  # (NaN padding, as above)
        dir_in = dict(pgp2=to_dev(z0(blocked(grp["sc"][0:1], nproma, dt))),
                      pgp3a=to_dev(z0(blocked(grp["sc"][1:5], nproma, dt).reshape(nb, 2, 2, nproma))),
                      pgp3b=to_dev(z0(blocked(grp["sc"][5:6], nproma, dt).reshape(nb, 1, 1, nproma))))
        if nuv:
            dir_in["pgpuv"] = to_dev(z0(blocked(np.concatenate([grp["u"], grp["v"]]), nproma, dt).reshape(nb, 2, nuv, nproma)))
        sp_out = dict(pspsc2=Z(ref.nspec2, 1), pspsc3a=Z(2, ref.nspec2, 2), pspsc3b=Z(1, ref.nspec2, 1))
    # ---- direct transform of the model's own grid fields (rounded to the library precision), against the model
    gu = rnd(np.concatenate(([grp["u"], grp["v"]] if nuv else []) + [grp["sc"]])).reshape(-1, ndgl, ndlon)
    rv, rd, rs, rmu, rmv = ref.dir_trans(gu, nuv=nuv, nsc=nsc)
    if nuv:
        sp_out.update(pspvor=Z(ref.nspec2, nuv), pspdiv=Z(ref.nspec2, nuv), pmeanu=Z(nuv), pmeanv=Z(nuv))
    et.edir_trans(r, kproma=nproma, mem_space=mem_space, **dir_in, **sp_out)
    if split:
        s2, s3a, s3b = to_host(sp_out["pspsc2"]), to_host(sp_out["pspsc3a"]), to_host(sp_out["pspsc3b"])
        got_sc = np.concatenate([s2, s3a[0], s3a[1], s3b[0]], axis=1)
    else:
        got_sc = to_host(sp_out["pspscalar"])
    outs = {"sc": np.asarray(got_sc, dtype=np.float64)}
    cmp("dir sc", outs["sc"].T, rs.T)
    if nuv:
        outs["vor"], outs["div"] = np.asarray(to_host(sp_out["pspvor"]), dtype=np.float64), np.asarray(to_host(sp_out["pspdiv"]), dtype=np.float64)
        cmp("dir vor", outs["vor"].T, rv.T)
        cmp("dir div", outs["div"].T, rd.T)
        scale = max(np.abs(gu[:2 * nuv]).max(), 1e-300)
        e = float(np.max(np.abs(np.concatenate([to_host(sp_out["pmeanu"]) - rmu, to_host(sp_out["pmeanv"]) - rmv]))) / scale)
        errs["dir mean"] = e if np.isfinite(e) else np.inf
    # the entries that do not enter the inverse transform are written as exact zeros
    for nm, a in outs.items():
        assert np.array_equal(ref.clean(a), a), "structural zeros of " + nm
    if kresol is None:
        et.trans_release(r)
    return errs, outs


def fp32_lam_direct(ref, g):
    """The float32 yardstick of EDIR_TRANS for one scalar grid field g (ndgl, ndlon): LamRef.analyse restated in single precision --
    scipy's single-precision real-to-complex FFT of every row, its complex FFT of every column, the split into (a, b), all in
    float32 / complex64 on float32 data.  Reference arithmetic only, nothing of the library.  Returns (nspec2, 1) in float64."""
    import scipy.fft
    L, N, M = ref.ndgl, ref.N, ref.M
    g32 = np.asarray(g, dtype=np.float32)
    X = scipy.fft.rfft(g32, axis=1)[:, :M + 1] / np.float32(ref.ndlon)
    Z = scipy.fft.fft(X, axis=0) / np.float32(L)  # Z[k, m]
    assert X.dtype == np.complex64 and Z.dtype == np.complex64
    Zp = Z[:N + 1, :].T
    Zm = np.conj(Z[(-np.arange(N + 1)) % L, :].T)
    a, b = np.complex64(0.5) * (Zp + Zm), np.complex64(-0.5j) * (Zp - Zm)
    assert a.dtype == np.complex64
    a, b = ref.mask(a[None].astype(np.complex128)), ref.mask(b[None].astype(np.complex128))
    a[:, :, 0], b[:, :, 0] = a[:, :, 0].real, b[:, :, 0].real
    b[:, 0, :] = 0.0
    return ref.pack(a, b)


def lam_white_case(et, ndlon, ndgl, M, N, nuv=2, nsc=3, split=False, nproma=None, precision=8, mem_space=None, seed=31, to_dev=None,
                   to_host=None, kresol=None):
    """EDIR_TRANS of FULL-BANDWIDTH grid fields against LamRef.dir_trans: U(-1,1) white noise in every point of the (nf, ndgl, ndlon)
    fields (rounded to the library precision before the model sees it) -- energy above KMSMAX in every row and outside the ellipse, which
    the transform must discard; the fields of lam_case hold none there.  Winds (vorticity, divergence, PMEANU / PMEANV), scalars, the
    structural zeros; the single-array and (split) the split-array call forms; the padding of the last NPROMA block is NaN.
    Returns (errs, yard): errs as lam_case; yard (precision=4 only) = {"lib", "cpu"}: the error of the library and of the float32
    yardstick fp32_lam_direct on scalar field 0, both against the float64 model, relative to the field's largest coefficient."""
    dt = np.float64 if precision == 8 else np.float32
    to_dev = to_dev or (lambda a: a)
    to_host = to_host or (lambda a: a)
    exwn, eywn = units(ndlon, ndgl)
    ref = LamRef(ndlon, ndgl, M, N, exwn, eywn)
    r = kresol if kresol is not None else et.esetup_trans(M, N, ndgl, kdlon=ndlon, pexwn=exwn, peywn=eywn, precision=precision)
    try:
        assert et.etrans_inq(r, "nspec2") == ref.nspec2 and et.etrans_inq(r, "ngptot") == ref.ngptot
        npt = ref.ngptot
        nproma = nproma or npt
        nb = (npt - 1) // nproma + 1
        if split:
            nsc = 6
        rng = np.random.default_rng(seed)
        g = rng.uniform(-1.0, 1.0, (2 * nuv + nsc, npt)).astype(dt).astype(np.float64)
        rv, rd, rs, rmu, rmv = ref.dir_trans(g.reshape(-1, ndgl, ndlon), nuv=nuv, nsc=nsc)
        pad = lambda a: np.where(a == -777.0, np.nan, a).astype(dt)
        Z = lambda *shape: to_dev(np.full(shape, -777.0, dtype=dt))
        gsc = g[2 * nuv:]
        if not split:
            dir_in = dict(pgp=to_dev(pad(blocked(g, nproma, dt))))
            sp_out = dict(pspscalar=Z(ref.nspec2, nsc))
        else:
            dir_in = dict(pgp2=to_dev(pad(blocked(gsc[0:1], nproma, dt))),
                          pgp3a=to_dev(pad(blocked(gsc[1:5], nproma, dt).reshape(nb, 2, 2, nproma))),
                          pgp3b=to_dev(pad(blocked(gsc[5:6], nproma, dt).reshape(nb, 1, 1, nproma))))
            if nuv:
                dir_in["pgpuv"] = to_dev(pad(blocked(g[:2 * nuv], nproma, dt).reshape(nb, 2, nuv, nproma)))
            sp_out = dict(pspsc2=Z(ref.nspec2, 1), pspsc3a=Z(2, ref.nspec2, 2), pspsc3b=Z(1, ref.nspec2, 1))
        if nuv:
            sp_out.update(pspvor=Z(ref.nspec2, nuv), pspdiv=Z(ref.nspec2, nuv), pmeanu=Z(nuv), pmeanv=Z(nuv))
        et.edir_trans(r, kproma=nproma, mem_space=mem_space, **dir_in, **sp_out)
        H = lambda a: np.asarray(to_host(a), dtype=np.float64)
        if split:
            s3a = H(sp_out["pspsc3a"])
            got_sc = np.concatenate([H(sp_out["pspsc2"]), s3a[0], s3a[1], H(sp_out["pspsc3b"])[0]], axis=1)
        else:
            got_sc = H(sp_out["pspscalar"])
        errs = {}

        def cmp(label, got, want):
            for f in range(want.shape[1]):  # NaN in the output counts as infinite
                e = np.abs(got[:, f] - want[:, f]).max() / max(np.abs(want[:, f]).max(), 1e-300)
                errs[label] = max(errs.get(label, 0.0), float(e) if np.isfinite(e) else np.inf)

        outs = {"sc": got_sc}
        cmp("dir sc", got_sc, rs)
        if nuv:
            outs["vor"], outs["div"] = H(sp_out["pspvor"]), H(sp_out["pspdiv"])
            cmp("dir vor", outs["vor"], rv)
            cmp("dir div", outs["div"], rd)
            e = np.max(np.abs(np.concatenate([H(sp_out["pmeanu"]) - rmu, H(sp_out["pmeanv"]) - rmv]))) / np.abs(g[:2 * nuv]).max()
            errs["dir mean"] = float(e) if np.isfinite(e) else np.inf
        for nm, a in outs.items():  # the entries that do not enter the inverse transform are written as exact zeros
            assert np.array_equal(ref.clean(a), a), "structural zeros of " + nm
        yard = None
        if precision == 4:
            want = rs[:, :1]
            y = fp32_lam_direct(ref, gsc[0].reshape(ndgl, ndlon))
            scale = np.abs(want).max()
            yard = {"lib": float(np.abs(got_sc[:, :1] - want).max() / scale), "cpu": float(np.abs(y - want).max() / scale)}
        return errs, yard
    finally:
        if kresol is None:
            et.trans_release(r)
