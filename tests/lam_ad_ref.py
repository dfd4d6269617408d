"""NumPy model of the limited-area adjoints EINV_TRANSAD / EDIR_TRANSAD, on top of LamRef (tests/lam_ref.py).

Written from the closed forms of INTEGRATION.md ("Limited-area adjoints"); tests/test_lam_ad_model.py holds it to the dense
transposes of LamRef.inv_trans and LamRef.dir_trans.  Inner products: plain sums over the grid points of every grid field and
over the NSPEC2 reals of every spectral field plus the means.  Array shapes as in LamRef.
"""
import numpy as np

from tests.lam_ref import LamRef


class LamAdRef(LamRef):
    def _w(self):
        wm = np.where(np.arange(self.M + 1) == 0, 1.0, 2.0)[None, :, None]
        wn = np.where(np.arange(self.N + 1) == 0, 1.0, 2.0)[None, None, :]
        return wm, wn

    def synth_t(self, g):
        """The transpose of LamRef.synth: grid (nf, ndgl, ndlon) -> (a, b); zeros in the entries that synth does not read."""
        L, N = self.ndgl, self.N
        wm, _ = self._w()
        X = np.fft.rfft(g, axis=2)[:, :, :self.M + 1]       # unnormalised r2c, truncated
        Z = np.fft.fft(X, axis=1)                           # Z[f, k, m]
        Zp = np.transpose(Z[:, :N + 1, :], (0, 2, 1))
        Zm = np.conj(np.transpose(Z[:, (-np.arange(N + 1)) % L, :], (0, 2, 1)))
        a, b = wm * (Zp + Zm), -1j * wm * (Zp - Zm)
        a[:, :, 0], b[:, :, 0] = wm[:, :, 0] * Zp[:, :, 0].real, wm[:, :, 0] * Zp[:, :, 0].imag
        a, b = self.mask(a), self.mask(b)
        b[:, 0, :] = 0.0
        return a, b

    def analyse_t(self, a, b):
        """The transpose of LamRef.analyse: (a, b) -> grid; the entries that analyse writes as structural zeros are not read."""
        L, N = self.ndgl, self.N
        wm, _ = self._w()
        a, b = self.mask(np.array(a)), self.mask(np.array(b))
        a[:, :, 0], b[:, :, 0] = a[:, :, 0].real, b[:, :, 0].real
        b[:, 0, :] = 0.0
        nf = a.shape[0]
        C = np.zeros((nf, self.M + 1, L), dtype=np.complex128)
        C[:, :, 0] = a[:, :, 0] + 1j * b[:, :, 0]
        for n in range(1, N + 1):
            C[:, :, n] = 0.5 * (a[:, :, n] + 1j * b[:, :, n])
            C[:, :, L - n] += 0.5 * (np.conj(a[:, :, n]) + 1j * np.conj(b[:, :, n]))
        F = np.fft.ifft(C, axis=2) * L / wm
        X = np.zeros((nf, L, self.ndlon // 2 + 1), dtype=np.complex128)
        X[:, :, :self.M + 1] = np.transpose(F, (0, 2, 1))
        return np.fft.irfft(X, n=self.ndlon, axis=2) / L    # c2r times 1 / (NDLON NDGL)

    def inv_transad(self, g, nuv=0, nsc=0, scders=False, vorgp=False, divgp=False, uvder=False):
        """g: the grid fields of LamRef.inv_trans, (nfields, ndgl, ndlon) -> spvor, spdiv, spsc, meanu, meanv."""
        g = np.asarray(g, dtype=np.float64)
        divgp = divgp or vorgp
        pos, grp = 0, {}
        names = ([("vor", nuv)] if vorgp and nuv else []) + ([("div", nuv)] if divgp and nuv else []) + \
            ([("u", nuv), ("v", nuv)] if nuv else []) + ([("sc", nsc)] if nsc else []) + ([("nsd", nsc)] if scders and nsc else []) + \
            ([("uew", nuv), ("vew", nuv)] if uvder and nuv else []) + ([("scew", nsc)] if scders and nsc else [])
        for nm, cnt in names:
            grp[nm] = self.synth_t(g[pos:pos + cnt])
            pos += cnt
        assert pos == g.shape[0]
        sub = lambda x, y: (x[0] - y[0], x[1] - y[1])
        res = [None, None, None, None, None]
        if nuv:
            u, v = grp["u"], grp["v"]
            if uvder:
                u, v = sub(u, self.ddx(*grp["uew"])), sub(v, self.ddx(*grp["vew"]))
            self.wind_max = max(np.abs(np.stack(u + v)).max(), 1e-300)  # the largest coefficient of the wind: the scale of the means
            kx, ky = self._k()
            lap = -(kx * kx + ky * ky) + 0.0 * u[0].real
            il = np.zeros_like(lap)
            il[lap != 0] = 1.0 / lap[lap != 0]
            dyu, dxv, dxu, dyv = self.ddy(*u), self.ddx(*v), self.ddx(*u), self.ddy(*v)
            va, vb = il * (dyu[0] - dxv[0]), il * (dyu[1] - dxv[1])
            da, db = il * (-dxu[0] - dyv[0]), il * (-dxu[1] - dyv[1])
            if vorgp:
                va, vb = va + grp["vor"][0], vb + grp["vor"][1]
            if divgp:
                da, db = da + grp["div"][0], db + grp["div"][1]
            res[0], res[1] = self.clean(self.pack(self.mask(va), self.mask(vb))), self.clean(self.pack(self.mask(da), self.mask(db)))
            res[3], res[4] = u[0][:, 0, 0].real.copy(), v[0][:, 0, 0].real.copy()
        if nsc:
            s = grp["sc"]
            if scders:
                s = sub(sub(s, self.ddy(*grp["nsd"])), self.ddx(*grp["scew"]))
            res[2] = self.clean(self.pack(self.mask(s[0]), self.mask(s[1])))
        return tuple(res)

    def dir_transad(self, spvor=None, spdiv=None, spsc=None, meanu=None, meanv=None):
        """-> grid fields (2 nuv + nsc, ndgl, ndlon) = u, v, scalars."""
        out = []
        nuv = 0 if spvor is None else np.asarray(spvor).shape[1]
        if nuv:
            va, vb = self.unpack(self.clean(spvor))
            da, db = self.unpack(self.clean(spdiv))
            dyv, dxd, dxv, dyd = self.ddy(va, vb), self.ddx(da, db), self.ddx(va, vb), self.ddy(da, db)
            ua, ub = dyv[0] - dxd[0], dyv[1] - dxd[1]
            wa, wb = -dxv[0] - dyd[0], -dxv[1] - dyd[1]
            ua[:, 0, 0] = np.zeros(nuv) if meanu is None else np.asarray(meanu, dtype=np.float64)
            wa[:, 0, 0] = np.zeros(nuv) if meanv is None else np.asarray(meanv, dtype=np.float64)
            ub[:, 0, 0] = wb[:, 0, 0] = 0.0
            out += [self.analyse_t(ua, ub), self.analyse_t(wa, wb)]
        if spsc is not None and np.asarray(spsc).shape[1]:
            out.append(self.analyse_t(*self.unpack(spsc)))
        return np.concatenate(out, axis=0)
