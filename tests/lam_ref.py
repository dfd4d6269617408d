"""NumPy model of the limited-area bi-Fourier transforms (ESETUP_TRANS / EINV_TRANS / EDIR_TRANS).

Written from the definitions in INTEGRATION.md ("Limited-area transforms"), with numpy.fft and nothing of the library:
the tests compare the library with this model, and the first test pins the model to the reference's known-answer pair
tests/golden/antwrp1300.

Spectral arrays have the shape (nspec2, nfld) -- PSPEC(nfld, nspec2) in Fortran order -- and grid fields the shape
(ndgl, ndlon): row after row as the caller stores them, the point index fastest.
"""
import numpy as np


def ellips(M, N):
    """KNTMP(0:M): the largest y-wavenumber n of every x-wavenumber m inside the ellipse."""
    k = np.zeros(M + 1, dtype=np.int64)
    k[0] = N
    for m in range(1, M):
        k[m] = int(float(N) / float(M) * np.sqrt(float(M * M - m * m)) + 1e-10)
    if M > 0:
        k[M] = 0
    return k


def zigzag(M, nprw):
    """Owning W-set (0-based) of every x-wavenumber 0..M: up 1..nprw, down nprw..1, and so on."""
    out, ik, ind = [], 0, 1
    for _ in range(M + 1):
        ik += ind
        if ik > nprw:
            ik, ind = nprw, -1
        elif ik < 1:
            ik, ind = 1, 1
        out.append(ik - 1)
    return np.array(out)


class LamRef:
    def __init__(self, ndlon, ndgl, M, N, exwn, eywn, myms=None):
        self.ndlon, self.ndgl, self.M, self.N = ndlon, ndgl, M, N
        self.exwn, self.eywn = float(exwn), float(eywn)
        self.kntmp = ellips(M, N)
        self.myms = list(range(M + 1)) if myms is None else list(myms)
        self.ncpl2m = {m: 2 * (int(self.kntmp[m]) + 1) for m in self.myms}
        self.nesm0, pos = {}, 1
        for m in self.myms:  # one-based start of every block, local wavenumbers ascending
            self.nesm0[m] = pos
            pos += 4 * (int(self.kntmp[m]) + 1)
        self.nspec2 = pos - 1
        self.nspec2g = 4 * int(np.sum(self.kntmp + 1))
        self.ngptot = ndlon * ndgl

    # ---- spectral layout -------------------------------------------------------------------
    def unpack(self, sp):
        """(nspec2, nf) reals -> a, b complex (nf, M+1, N+1), zero outside the ellipse and for foreign m."""
        sp = np.asarray(sp, dtype=np.float64)
        nf = sp.shape[1]
        a = np.zeros((nf, self.M + 1, self.N + 1), dtype=np.complex128)
        b = np.zeros_like(a)
        for m in self.myms:
            i0, nn = self.nesm0[m] - 1, int(self.kntmp[m]) + 1
            blk = sp[i0:i0 + 4 * nn].reshape(nn, 4, nf)
            a[:, m, :nn] = (blk[:, 0] + 1j * blk[:, 1]).T
            b[:, m, :nn] = (blk[:, 2] + 1j * blk[:, 3]).T
        return a, b

    def pack(self, a, b):
        nf = a.shape[0]
        sp = np.zeros((self.nspec2, nf))
        for m in self.myms:
            i0, nn = self.nesm0[m] - 1, int(self.kntmp[m]) + 1
            blk = sp[i0:i0 + 4 * nn].reshape(nn, 4, nf)
            blk[:, 0], blk[:, 1] = a[:, m, :nn].real.T, a[:, m, :nn].imag.T
            blk[:, 2], blk[:, 3] = b[:, m, :nn].real.T, b[:, m, :nn].imag.T
        return sp

    def clean(self, sp):
        """Zeros in the entries that do not enter the inverse transform: a_i, b_i of n = 0, b of m = 0."""
        a, b = self.unpack(sp)
        a[:, :, 0] = a[:, :, 0].real
        b[:, :, 0] = b[:, :, 0].real
        b[:, 0, :] = 0.0
        return self.pack(a, b)

    def random_spec(self, rng, nf, wind=False):
        """U(-0.5, 0.5) in every entry that enters the transform.  wind: for vorticity and divergence -- the amplitude grows with the
        wavenumber, |k| / |k|max, so that the WIND they stand for is white.  The wind of a white vorticity is red, u ~ vor / |k|; a
        direct transform returns every coefficient of u with an absolute error of eps times the largest one, whatever the
        implementation, and vorticity multiplies that by |k|: eps |k|max / |k|min of the largest vorticity coefficient -- in float32
        at 1536 x 1440, 6e-8 x 767 = 4.6e-5 before any constant, above the 3e-5 the float32 library is held to (measured with white
        vorticity on an MI355X: 1.5e-5 at 400 x 300, 7.2e-5 at 1536 x 1440).  A white wind asks the same of every coefficient."""
        sp = rng.uniform(-0.5, 0.5, (self.nspec2, nf))
        if wind:
            a, b = self.unpack(sp)
            kx, ky = self._k()
            k = np.sqrt(kx * kx + ky * ky)
            a, b = a * (k / k.max()), b * (k / k.max())
            sp = self.pack(a, b)
        return self.clean(sp)

    # ---- operators on (a, b) ---------------------------------------------------------------
    def _k(self):
        kx = self.exwn * np.arange(self.M + 1)[None, :, None]
        ky = self.eywn * np.arange(self.N + 1)[None, None, :]
        return kx, ky

    def ddx(self, a, b):  # i m EXWN on F_m = A + i B
        kx, _ = self._k()
        return -kx * b, kx * a

    def ddy(self, a, b):  # i n EYWN on the y-coefficient
        _, ky = self._k()
        return 1j * ky * a, 1j * ky * b

    def mask(self, a):
        out = np.zeros_like(a)
        for m in range(self.M + 1):
            out[:, m, :int(self.kntmp[m]) + 1] = a[:, m, :int(self.kntmp[m]) + 1]
        return out

    # ---- the transforms ---------------------------------------------------------------------
    def synth(self, a, b):
        """(a, b) -> grid (nf, ndgl, ndlon)."""
        nf, L, N = a.shape[0], self.ndgl, self.N
        C = np.zeros((nf, self.M + 1, L), dtype=np.complex128)
        C[:, :, :N + 1] = a + 1j * b
        for n in range(1, N + 1):
            C[:, :, L - n] += np.conj(a[:, :, n]) + 1j * np.conj(b[:, :, n])
        F = np.fft.ifft(C, axis=2) * L                       # F_m(j), sign +
        X = np.zeros((nf, L, self.ndlon // 2 + 1), dtype=np.complex128)
        X[:, :, :self.M + 1] = np.transpose(F, (0, 2, 1))
        return np.fft.irfft(X, n=self.ndlon, axis=2) * self.ndlon   # c2r, unnormalised

    def analyse(self, g):
        """grid (nf, ndgl, ndlon) -> (a, b), truncated to the ellipse, structural zeros written."""
        L, N = self.ndgl, self.N
        X = np.fft.rfft(g, axis=2)[:, :, :self.M + 1] / self.ndlon
        Z = np.fft.fft(X, axis=1) / L                       # Z[f, k, m]
        Zp = np.transpose(Z[:, :N + 1, :], (0, 2, 1))
        idx = (-np.arange(N + 1)) % L
        Zm = np.conj(np.transpose(Z[:, idx, :], (0, 2, 1)))
        a, b = 0.5 * (Zp + Zm), -0.5j * (Zp - Zm)
        a, b = self.mask(a), self.mask(b)
        a[:, :, 0], b[:, :, 0] = a[:, :, 0].real, b[:, :, 0].real
        b[:, 0, :] = 0.0
        return a, b

    def inv_trans(self, spvor=None, spdiv=None, spsc=None, meanu=None, meanv=None, scders=False, vorgp=False, divgp=False,
                  uvder=False):
        """Grid fields (nfields, ndgl, ndlon) in the order of INV_TRANS:
        [vor] [div] u v scalars [N-S derivatives] [E-W derivatives of u, of v] [E-W derivatives of the scalars]."""
        out = []
        nuv = 0 if spvor is None else np.asarray(spvor).shape[1]
        if nuv:
            va, vb = self.unpack(spvor)
            da, db = self.unpack(spdiv)
            kx, ky = self._k()
            lap = -(kx * kx + ky * ky) + 0.0 * va.real
            il = np.zeros_like(lap)
            il[lap != 0] = 1.0 / lap[lap != 0]
            dxd, dyv = self.ddx(da, db), self.ddy(va, vb)
            dxv, dyd = self.ddx(va, vb), self.ddy(da, db)
            ua, ub = il * (dxd[0] - dyv[0]), il * (dxd[1] - dyv[1])
            wa, wb = il * (dxv[0] + dyd[0]), il * (dxv[1] + dyd[1])
            ua[:, 0, 0] = np.zeros(nuv) if meanu is None else np.asarray(meanu, dtype=np.float64)
            wa[:, 0, 0] = np.zeros(nuv) if meanv is None else np.asarray(meanv, dtype=np.float64)
            ub[:, 0, 0] = wb[:, 0, 0] = 0.0
            if vorgp:
                out.append(self.synth(va, vb))
            if divgp or vorgp:
                out.append(self.synth(da, db))
            out.append(self.synth(ua, ub))
            out.append(self.synth(wa, wb))
        nsc = 0 if spsc is None else np.asarray(spsc).shape[1]
        if nsc:
            sa, sb = self.unpack(spsc)
            out.append(self.synth(sa, sb))
            if scders:
                out.append(self.synth(*self.ddy(sa, sb)))
        if nuv and uvder:
            out.append(self.synth(*self.ddx(ua, ub)))
            out.append(self.synth(*self.ddx(wa, wb)))
        if nsc and scders:
            out.append(self.synth(*self.ddx(sa, sb)))
        return np.concatenate(out, axis=0)

    def dir_trans(self, g, nuv=0, nsc=0):
        """g: (2 nuv + nsc, ndgl, ndlon) = u, v, scalars -> spvor, spdiv, spsc, meanu, meanv."""
        g = np.asarray(g, dtype=np.float64)
        res = [None, None, None, None, None]
        if nuv:
            ua, ub = self.analyse(g[:nuv])
            wa, wb = self.analyse(g[nuv:2 * nuv])
            dxv, dyu = self.ddx(wa, wb), self.ddy(ua, ub)
            dxu, dyv = self.ddx(ua, ub), self.ddy(wa, wb)
            va, vb = dxv[0] - dyu[0], dxv[1] - dyu[1]
            da, db = dxu[0] + dyv[0], dxu[1] + dyv[1]
            for x in (va, vb, da, db):  # the structural zeros of the outputs
                x[:, :, 0] = x[:, :, 0].real
            vb[:, 0, :] = 0.0
            db[:, 0, :] = 0.0
            res[0], res[1] = self.pack(self.mask(va), self.mask(vb)), self.pack(self.mask(da), self.mask(db))
            res[3], res[4] = ua[:, 0, 0].real.copy(), wa[:, 0, 0].real.copy()
        if nsc:
            res[2] = self.pack(*self.analyse(g[2 * nuv:2 * nuv + nsc]))
        return tuple(res)
