"""The NumPy model of the limited-area adjoints (tests/lam_ad_ref.py) against the dense transposes of LamRef.inv_trans and
LamRef.dir_trans: pins the definition of EINV_TRANSAD / EDIR_TRANSAD without the library.  One wind field and one scalar; the
input vector of the inverse map is (vor, div, scalar, meanu, meanv), NSPEC2 reals each and the two means."""
import itertools

import numpy as np
import pytest

from tests.lam_ad_ref import LamAdRef
from tests.lam_common import units

SIZES = [(20, 18, 9, 8), (12, 10, 0, 4), (12, 10, 5, 0), (15, 11, 7, 5)]
FLAGS = [dict(zip(("scders", "vorgp", "divgp", "uvder"), c)) for c in itertools.product((False, True), repeat=4)]


def _ref(size):
    ndlon, ndgl, M, N = size
    return LamAdRef(ndlon, ndgl, M, N, *units(ndlon, ndgl))


def _spec_basis(ref):
    """The unit vectors of (vor, div, sc, meanu, meanv) as 3 nspec2 + 2 'fields'."""
    n, K = ref.nspec2, 3 * ref.nspec2 + 2
    vor, div, sc, mu, mv = np.zeros((n, K)), np.zeros((n, K)), np.zeros((n, K)), np.zeros(K), np.zeros(K)
    vor[np.arange(n), np.arange(n)] = 1.0
    div[np.arange(n), n + np.arange(n)] = 1.0
    sc[np.arange(n), 2 * n + np.arange(n)] = 1.0
    mu[3 * n], mv[3 * n + 1] = 1.0, 1.0
    return vor, div, sc, mu, mv


def _spec_vec(vor, div, sc, mu, mv):
    """(nspec2, K) x 3, (K,) x 2 -> (3 nspec2 + 2, K)"""
    return np.concatenate([vor, div, sc, mu[None], mv[None]], axis=0)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "".join(k[0] if v else "-" for k, v in f.items()))
def test_inv_transad_is_transpose(size, flags):
    ref = _ref(size)
    K = 3 * ref.nspec2 + 2
    # (EINV_TRANS does not read a_i, b_i of n = 0 and b of m = 0; LamRef.synth would: those unit vectors become zero columns)
    vor, div, sc, mu, mv = _spec_basis(ref)
    g = ref.inv_trans(ref.clean(vor), ref.clean(div), ref.clean(sc), mu, mv, **flags)  # (nfields K, ndgl, ndlon), field group outer
    nfields = g.shape[0] // K
    A = g.reshape(nfields, K, ref.ngptot).transpose(0, 2, 1).reshape(nfields * ref.ngptot, K)
    # the model on the unit vectors of the grid side, field by field
    At = np.zeros((K, nfields * ref.ngptot))
    eye = np.eye(ref.ngptot).reshape(ref.ngptot, 1, ref.ndgl, ref.ndlon)
    for f in range(nfields):
        gin = np.zeros((ref.ngptot, nfields, ref.ndgl, ref.ndlon))
        gin[:, f:f + 1] = eye
        gin = gin.transpose(1, 0, 2, 3).reshape(nfields * ref.ngptot, ref.ndgl, ref.ndlon)  # group outer, unit vector inner
        r = ref.inv_transad(gin, nuv=ref.ngptot, nsc=ref.ngptot, **flags)
        At[:, f * ref.ngptot:(f + 1) * ref.ngptot] = _spec_vec(*r)
    assert np.abs(At - A.T).max() <= 1e-12 * np.abs(A).max()
    # the entries that do not enter EINV_TRANS: zero columns of A, exact zeros of the model
    assert np.all(At[np.all(A == 0.0, axis=0)] == 0.0)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_dir_transad_is_transpose(size):
    ref = _ref(size)
    K, npt = 3 * ref.nspec2 + 2, ref.ngptot
    eye = np.eye(npt).reshape(npt, ref.ndgl, ref.ndlon)
    zero = np.zeros_like(eye)
    cols = []
    for f in range(3):  # unit vectors of u, v, scalar
        gin = np.concatenate([eye if f == k else zero for k in range(3)])
        cols.append(_spec_vec(*ref.dir_trans(gin, nuv=npt, nsc=npt)))
    B = np.concatenate(cols, axis=1)  # (K, 3 npt)
    g = ref.dir_transad(*_spec_basis(ref))  # (3 K, ndgl, ndlon)
    Bt = g.reshape(3, K, npt).transpose(0, 2, 1).reshape(3 * npt, K)
    assert np.abs(Bt - B.T).max() <= 1e-12 * np.abs(B).max()
    # garbage in the entries that EDIR_TRANS writes as structural zeros is not read
    dead = np.all(B[:3 * ref.nspec2] == 0.0, axis=1).reshape(3, ref.nspec2)
    rng = np.random.default_rng(5)
    x = [rng.uniform(-1, 1, (ref.nspec2, 2)) for _ in range(3)]
    y = [np.where(dead[k][:, None], 1e30, x[k]) for k in range(3)]
    mu, mv = rng.uniform(-1, 1, 2), rng.uniform(-1, 1, 2)
    assert np.array_equal(ref.dir_transad(*[ref.clean(a) for a in x], mu, mv), ref.dir_transad(*y, mu, mv))
