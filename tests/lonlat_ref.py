"""Direct summation of the truncated spherical-harmonic series at arbitrary latitudes (numpy only): the yardstick of the lat-lon
inverse transform (INV_TRANS with LDLATLON), which the frozen oracle does not have.  tests/test_lonlat_emu.py pins it to the oracle
on full Gaussian grids before anything is compared with it.

Normalisation of ecTrans: P_0^0 = 1, 1/2 int P^2 dmu = 1, no Condon-Shortley sign;
  P_m^m = sqrt((2m+1)/(2m)) cos(lat) P_(m-1)^(m-1),   P_(n+1)^m = (mu P_n^m - e_n^m P_(n-1)^m) / e_(n+1)^m,
  e_n^m = sqrt((n^2 - m^2) / (4 n^2 - 1)),   (1 - mu^2) dP_n^m/dmu = -n e_(n+1)^m P_(n+1)^m + (n+1) e_n^m P_(n-1)^m
  f(mu, lambda) = sum_m c_m Re(sum_n psi_n^m P_n^m(mu) e^(i m lambda)),  c_0 = 1, c_m = 2,  m <= NMEN.
Vectorised over the latitudes; the longitude sum is a matrix product with e^(i m lambda_i) at the longitudes themselves, so the
half-cell shift of a shifted grid enters through lambda_i and nothing else."""
import functools

import numpy as np

RA = 6371229.0
FLAGS = dict(scders=True, vorgp=True, divgp=True, uvder=True)


def eps_nm(n, m):
    n = np.asarray(n, dtype=np.float64)
    return np.sqrt((n * n - float(m) * m) / (4.0 * n * n - 1.0))


def lonlat_rows(nlat, shifted):
    """(mu, cos(lat)) of the rows of the lat-lon grid as INV_TRANS(LDLATLON) returns them, north to south.  Unshifted (nlat odd):
    NDGL = nlat + 1 rows, 90 - (j-1) 180 / (nlat-1) degrees for j = 1 .. NDGL/2 (pole ... equator) and their mirrors, so the equator
    comes twice.  Shifted (nlat even): NDGL = nlat rows at 90 - (j - 1/2) 180 / nlat."""
    if shifted:
        assert nlat % 2 == 0
        th = (np.arange(nlat // 2) + 0.5) * np.pi / nlat
        mu, c = np.cos(th), np.sin(th)
    else:
        assert nlat % 2 == 1
        h = (nlat + 1) // 2
        th = np.arange(h) * np.pi / (nlat - 1)
        mu, c = np.cos(th), np.sin(th)
        mu[0], c[0] = 1.0, 0.0
        mu[-1], c[-1] = 0.0, 1.0
    return np.concatenate([mu, -mu[::-1]]), np.concatenate([c, c[::-1]])


class SeriesRef:
    """The series on the rows `mu` (cos(lat) = `cth`, default sqrt((1 - mu)(1 + mu))) x `nlon` longitudes (i + lon_shift) 2 pi / nlon."""

    def __init__(self, nsmax, nasm0, mu, nlon, lon_shift=0.0, cth=None, ra=RA):
        self.N, self.nasm0, self.nlon, self.ra = int(nsmax), np.asarray(nasm0), int(nlon), float(ra)
        self.mu = np.asarray(mu, dtype=np.float64)
        # (1 - mu)(1 + mu), not 1 - mu^2: the rounding of mu^2 is 3e-12 of cos^2 on the first row of a 384-row Gaussian grid
        self.cth = np.sqrt((1.0 - self.mu) * (1.0 + self.mu)) if cth is None else np.asarray(cth, dtype=np.float64)
        self.nmen = min(self.N, (self.nlon - 1) // 2)
        self.lam = (np.arange(self.nlon) + lon_shift) * (2.0 * np.pi / self.nlon)
        self.nlat = self.mu.size
        self.ngptot = self.nlat * self.nlon

    def legendre(self, m, pmm):
        """P[n - m][lat], n = m .. N + 1, from the sectoral values pmm = P_m^m, and H[n - m][lat] = (1 - mu^2) dP_n^m / dmu, n = m .. N"""
        N, mu = self.N, self.mu
        P = np.zeros((N + 2 - m, mu.size))
        P[0] = pmm
        P[1] = mu * P[0] / eps_nm(m + 1, m)
        for n in range(m + 1, N + 1):
            P[n + 1 - m] = (mu * P[n - m] - eps_nm(n, m) * P[n - 1 - m]) / eps_nm(n + 1, m)
        n = np.arange(m, N + 1)
        H = -(n * eps_nm(n + 1, m))[:, None] * P[1:]
        H[1:] += ((n + 1) * eps_nm(n, m))[1:, None] * P[:-2]
        return P[:-1], H

    def coefficients(self, spec, which="P"):
        """Fourier coefficients F[fld][lat][m] (complex) of the fields spec[nspec2][fld]: sum_n psi_n^m P_n^m (or H_n^m)"""
        N = self.N
        F = np.zeros((spec.shape[1], self.nlat, self.nmen + 1), dtype=np.complex128)
        pmm = np.ones(self.nlat)
        for m in range(self.nmen + 1):
            if m > 0:
                pmm = np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * self.cth * pmm
            P, H = self.legendre(m, pmm)
            i0 = self.nasm0[m] - 1
            psi = spec[i0:i0 + 2 * (N - m + 1):2] + 1j * spec[i0 + 1:i0 + 2 * (N - m + 1):2]  # [n - m][fld]
            F[:, :, m] = psi.T @ (P if which == "P" else H)
        return F

    def legpol(self, m):
        """P_n^m(mu), [n - m][lat], n = m .. N"""
        pmm = np.ones(self.nlat)
        for k in range(1, m + 1):
            pmm = np.sqrt((2.0 * k + 1.0) / (2.0 * k)) * self.cth * pmm
        return self.legendre(m, pmm)[0]

    def to_grid(self, F, ew=False, scale=None):
        """[fld][lat * nlon] grid fields of the coefficients F; ew: the east-west derivative d/dlambda; scale[lat]: row factors"""
        m = np.arange(self.nmen + 1)
        if ew:
            F = F * (1j * m)
        c = np.where(m == 0, 1.0, 2.0)[:, None]
        Er, Ei = c * np.cos(np.outer(m, self.lam)), c * np.sin(np.outer(m, self.lam))
        g = F.real @ Er - F.imag @ Ei  # [fld][lat][lon]
        if scale is not None:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                g = g * scale[None, :, None]
        return g.reshape(F.shape[0], -1)

    def inv_trans(self, spvor=None, spdiv=None, spsc=None, spu=None, spv=None, scders=False, vorgp=False, divgp=False, uvder=False):
        """The grid fields of INV_TRANS in its order -- [vor] [div] u v scalars [N-S derivatives] [E-W derivatives of u, v] [E-W derivatives
        of the scalars] -- as [fld][point].  spu, spv: the spectral (U, V) = (u, v) cos(lat) of VORDIV_TO_UV for spvor, spdiv (exact when
        these vanish at n = NSMAX: VORDIV_TO_UV stops at n <= NSMAX).  Rows with cos(lat) = 0 hold inf / nan in the fields that carry
        1 / cos(lat)."""
        out = []
        with np.errstate(divide="ignore"):
            rc = 1.0 / self.cth
        if spvor is not None:
            if vorgp:
                out.append(self.to_grid(self.coefficients(spvor)))
            if vorgp or divgp:
                out.append(self.to_grid(self.coefficients(spdiv)))
            FU, FV = self.coefficients(spu), self.coefficients(spv)
            out += [self.to_grid(FU, scale=rc), self.to_grid(FV, scale=rc)]
        if spsc is not None:
            FS = self.coefficients(spsc)
            out.append(self.to_grid(FS))
            if scders:
                out.append(self.to_grid(self.coefficients(spsc, "H"), scale=rc / self.ra))
        if spvor is not None and uvder:
            out += [self.to_grid(FU, ew=True, scale=rc * rc / self.ra), self.to_grid(FV, ew=True, scale=rc * rc / self.ra)]
        if spsc is not None and scders:
            out.append(self.to_grid(FS, ew=True, scale=rc / self.ra))
        return np.concatenate(out, axis=0)


def wind_spectrum(rng, nasm0, nsmax, nspec2, nf):
    """Random vorticity / divergence with zero (0,0) and zero n = NSMAX coefficients (see SeriesRef.inv_trans)"""
    from tests.common import n_of_index, random_spectrum
    sp = random_spectrum(rng, nasm0, nsmax, nspec2, nf, True)
    sp[n_of_index(nasm0, nsmax, nspec2) == nsmax] = 0.0
    return sp


# ---- what the emulator tier and the GPU tier share: inputs, the order of the fields, one parity case --------------------------------
def spectra(nsmax, seed=3, nuv=1, nsc=2):
    """(oracle of the truncation, vor, div, scalars, U, V): winds with zero (0,0) and n = NSMAX coefficients"""
    from oracle.oracle import Oracle
    from tests.common import random_spectrum
    o = Oracle(nsmax, np.full(2 * (nsmax + 1), 4 * (nsmax + 1), dtype=np.int32), lazy=True)
    rng = np.random.default_rng(seed)
    vor = wind_spectrum(rng, o.nasm0, nsmax, o.nspec2, nuv)
    div = wind_spectrum(rng, o.nasm0, nsmax, o.nspec2, nuv)
    sc = random_spectrum(rng, o.nasm0, nsmax, o.nspec2, nsc, False)
    u, v = o.vordiv_to_uv(vor, div)
    return o, vor, div, sc, u, v


def field_groups(nuv, nsc):
    """(name, first field, count, carries 1 / cos(lat)) of the fields of INV_TRANS with FLAGS, in its order"""
    names = [("vor", nuv, False), ("div", nuv, False), ("u", nuv, True), ("v", nuv, True), ("scalar", nsc, False), ("nsder", nsc, True),
             ("u_ew", nuv, True), ("v_ew", nuv, True), ("scalar_ew", nsc, True)]
    out, f0 = [], 0
    for nm, cnt, acos in names:
        out.append((nm, f0, cnt, acos))
        f0 += cnt
    return out



@functools.lru_cache(maxsize=4)
def reference_fields(nsmax, nlat, nlon, seed=3):
    """(vor, div, scalars, the fields of the series with every derivative) of one lat-lon grid; nlat even: the shifted grid"""
    shifted = nlat % 2 == 0
    o, vor, div, sc, u, v = spectra(nsmax, seed)
    mu, cth = lonlat_rows(nlat, shifted)
    ref = SeriesRef(nsmax, o.nasm0, mu, nlon, 0.5 if shifted else 0.0, cth=cth)
    return vor, div, sc, ref.inv_trans(spvor=vor, spdiv=div, spsc=sc, spu=u, spv=v, **FLAGS)


def lonlat_case(et, nsmax, nlat, nlon, nproma=None, precision=8, to=None, back=None, setup_kw=None, seed=3):
    """INV_TRANS(LDLATLON) with every derivative against the series; returns {field group: error relative to the maximum of the
    reference field}.  Left out: on the unshifted grid the two pole rows of the fields that carry 1 / cos(lat), nothing else."""
    shifted = nlat % 2 == 0
    dt = np.float32 if precision == 4 else np.float64
    to = to or (lambda a: np.ascontiguousarray(a, dtype=dt))
    back = back or (lambda a: np.asarray(a, dtype=np.float64))
    vor, div, sc, gref = reference_fields(nsmax, nlat, nlon, seed)
    mu = lonlat_rows(nlat, shifted)[0]
    r = et.setup_trans(nsmax, nlat if shifted else nlat - 1, kdlon=nlon, ldll=True, ldshiftll=shifted, precision=precision, **(setup_kw or {}))
    try:
        ng = et.trans_inq(r, "ngptot")
        ndgl = et.trans_inq(r, "ndgl")
        assert ndgl == mu.size and ng == ndgl * nlon == gref.shape[1]
        npr = nproma or ng
        gp = to(np.zeros(((ng - 1) // npr + 1, gref.shape[0], npr)))
        et.inv_trans(r, pspvor=to(vor), pspdiv=to(div), pspscalar=to(sc), pgp=gp, kproma=npr, ldlatlon=True, ldscders=True, ldvorgp=True,
                     lddivgp=True, lduvder=True)
        from tests.common import unblock
        g = unblock(back(gp), ng)
    finally:
        et.trans_release(r)
    assert np.isfinite(g).all()  # the pole rows of u, v and the derivatives are finite
    rows = np.ones(ndgl, dtype=bool)
    if not shifted:
        rows[0] = rows[-1] = False
    pts = np.repeat(rows, nlon)
    errs = {}
    for nm, f0, cnt, acos in field_groups(1, 2):
        sel = pts if acos else np.ones(ng, dtype=bool)
        a, b = g[f0:f0 + cnt][:, sel], gref[f0:f0 + cnt][:, sel]
        assert np.isfinite(b).all()
        errs[nm] = (np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max()
    print("lonlat T%d %dx%d nproma %s precision %d: %s" % (nsmax, nlat, nlon, nproma, precision, " ".join("%s %.2e" % kv for kv in errs.items())))
    return errs, g
