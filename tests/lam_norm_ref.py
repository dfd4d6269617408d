"""NumPy restatements of the limited-area norms and global layouts (ESPECNORM, EGPNORM_TRANS, EDIST_* / EGATH_*), built on LamRef
(tests/lam_ref.py: kntmp, nesm0) and nothing of the library.  Definitions: INTEGRATION.md, "Limited-area transforms".

Sums are math.fsum (correctly rounded) of terms computed in float64; the callers hand in arrays already rounded to the library's
precision, held as float64.  Spectral arrays are (nspec2, nfld), grid fields (nfld, ndgl * ndlon), as in tests/lam_ref.py."""
import math

import numpy as np


def npme(kntmp):
    """NPME(0:M) from its recurrence: NPME(0) = 1, NPME(m) = NPME(m - 1) + KNTMP(m - 1) + 1 -- the zero-based position of (m, n = 0)
    in the metric PMET."""
    out = [1]
    for m in range(1, len(kntmp)):
        out.append(out[-1] + int(kntmp[m - 1]) + 1)
    return np.array(out, dtype=np.int64)


def pmet_size(kntmp):
    """elements PMET must hold: NPME(KMSMAX) + KNTMP(KMSMAX) + 1"""
    return int(npme(kntmp)[-1] + int(kntmp[-1]) + 1)


def spec_terms(ref, sp, pmet=None):
    """w(m, n) (a_r^2 + a_i^2 + b_r^2 + b_i^2) of every (m, n) of ref.myms: {m: (KNTMP(m) + 1, nfld) float64}"""
    sp = np.asarray(sp, dtype=np.float64)
    pos = npme(ref.kntmp)
    out = {}
    for m in ref.myms:
        nn = int(ref.kntmp[m]) + 1
        i0 = ref.nesm0[m] - 1
        blk = sp[i0:i0 + 4 * nn].reshape(nn, 4, -1)
        t = blk[:, 0] ** 2 + blk[:, 1] ** 2 + blk[:, 2] ** 2 + blk[:, 3] ** 2
        if pmet is not None:
            t = np.asarray(pmet, dtype=np.float64)[pos[m]:pos[m] + nn, None] * t
        out[m] = t
    return out


def spec_sums(ref, sp, pmet=None):
    """S(f, m) for the wavenumbers of ref.myms in that order: (len(myms), nfld)"""
    terms = spec_terms(ref, sp, pmet)
    nf = np.asarray(sp).shape[1]
    return np.array([[math.fsum(terms[m][:, f].tolist()) for f in range(nf)] for m in ref.myms]).reshape(len(ref.myms), nf)


def spec_norm(ref, sp, pmet=None):
    """PNORM(f) = sqrt(sum over all (m, n) of the terms); ref must hold every wavenumber (the one-task layout)"""
    assert list(ref.myms) == list(range(ref.M + 1))
    terms = spec_terms(ref, sp, pmet)
    allt = np.concatenate([terms[m] for m in ref.myms], axis=0)
    return np.array([math.sqrt(math.fsum(allt[:, f].tolist())) for f in range(allt.shape[1])])


def gp_norms(fields, ndgl, ndlon, precision=8):
    """(PAVE, PMIN, PMAX) of fields (nfld, ndgl * ndlon): PAVE = sum over the rows of w (row sum) / NDLON, w = 1 / NDGL, rounded to
    real(4) first in the single-precision library (REAL(PW,JPRB))."""
    g = np.asarray(fields, dtype=np.float64).reshape(-1, ndgl, ndlon)
    w = 1.0 / ndgl
    if precision == 4:
        w = float(np.float32(w))
    ave = np.array([math.fsum(math.fsum(row.tolist()) * w / ndlon for row in f) for f in g])
    return ave, g.reshape(g.shape[0], -1).min(axis=1), g.reshape(g.shape[0], -1).max(axis=1)


def bands(ndgl, nproc):
    """first row of every task's band of whole rows and NDGL: the first mod(NDGL, nproc) bands are one row longer"""
    return [r * (ndgl // nproc) + min(r, ndgl % nproc) for r in range(nproc + 1)]


def local_spec_index(one, myms):
    """positions in the global (one-task) spectral field of a task's coefficients, in its local order"""
    return np.concatenate([np.arange(one.nesm0[m] - 1, one.nesm0[m] - 1 + 4 * (int(one.kntmp[m]) + 1)) for m in myms])
