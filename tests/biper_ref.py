"""NumPy model of the biperiodicisation routines (FPBIPERE, ETIBIHIE, the Boyd window, HORIZ_FIELD) as INTEGRATION.md, section
"Biperiodicisation", defines them: every operation is carried out in the dtype of the input, in the order the Fortran routines of
etrans/biper write them, with no fused multiply-add, so that the results are the reference's bytes (tests/test_biper_model.py holds
them to tests/golden/biper).  The functions return new arrays; the inputs stay as they are."""
import math

import numpy as np


def _coef(v1, v2, vu, vum1, n, u, lam, dt):
    """A, B, C, D of the cubic that continues a line known on 1..u over u+1..n (espline_mod.F90, PALFA = 0)"""
    k = dt(n - u + 1)
    kp1 = k + dt(1)
    ea = ((v1 - vu) / k - vu + vum1) * dt(6) / kp1
    eb = (v2 - v1 - (v1 - vu) / k) * dt(6) / kp1
    mm = dt(4) - lam * lam
    m1 = (dt(2) * ea - lam * eb) / mm
    m2 = (dt(2) * eb - lam * ea) / mm
    return vu, (v1 - vu) / k - (dt(2) * m1 + m2) * k / dt(6), dt(0.5) * m1, (m2 - m1) / (dt(6) * k)


def spline(w, UX, UY, bix, biy, lam_of_y=False):
    """w[y, f, x], in place"""
    Y, _, X = w.shape
    dt = w.dtype.type
    kx = dt(X - UX + 1)
    lamx = kx / (kx + dt(1))
    if bix:
        v = w[:UY]
        A, B, C, D = _coef(v[..., 0], v[..., 1], v[..., UX - 1], v[..., UX - 2], X, UX, lamx, dt)
        for j in range(1, X - UX + 1):
            zj = dt(j)
            v[..., UX - 1 + j] = A + zj * (B + zj * (C + D * zj))
    if biy:
        ky = dt(Y - UY + 1)
        lam = ky / (ky + dt(1)) if lam_of_y else lamx  # the reference uses the x direction's (espline_mod.F90:179-181)
        v = w[:, :, :X if bix else UX]
        A, B, C, D = _coef(v[0], v[1], v[UY - 1], v[UY - 2], Y, UY, lam, dt)
        for j in range(1, Y - UY + 1):
            zj = dt(j)
            v[UY - 1 + j] = A + zj * (B + zj * (C + zj * D))


def _stencil(z, dt):
    xp, xm = np.roll(z, -1, 2), np.roll(z, 1, 2)
    yp, ym = np.roll(z, -1, 0), np.roll(z, 1, 0)
    pp, mp = np.roll(xp, -1, 0), np.roll(xm, -1, 0)  # (x+1, y+1), (x-1, y+1)
    pm, mm = np.roll(xp, 1, 0), np.roll(xm, 1, 0)    # (x+1, y-1), (x-1, y-1)
    return (dt(4) * z + dt(2) * (xp + xm + yp + ym) + pp + mp + pm + mm) / dt(16)


def smooth(w, UX, UY, bix, biy, fewer=0):
    """w[y, f, x], in place (esmoothe_mod.F90).  A direction that is off has UX == X or UY == Y, so the periodic wrap of np.roll is
    the reference's wrap in every case."""
    Y, _, X = w.shape
    dt = w.dtype.type
    iend = (max(X - UX, Y - UY) + 1) // 2 - fewer
    X1 = X2 = X
    Y1 = Y2 = Y
    if bix and not biy:
        Y1 = Y2 = UY
    if biy and not bix:
        X1 = X2 = UX
    for l in range(1, iend + 1):
        lo, hi = UX + l, X1 - l + 1  # one-based, inclusive
        if lo <= hi:
            s = _stencil(w, dt)
            w[:Y2, :, lo - 1:hi] = s[:Y2, :, lo - 1:hi]
        lo, hi = UY + l, Y1 - l + 1
        if lo <= hi:
            s = _stencil(w, dt)
            w[lo - 1:hi, :, :X2] = s[lo - 1:hi, :, :X2]


def core(w, UX, UY, bix=True, biy=True, lam_of_y=False, fewer=0):
    spline(w, UX, UY, bix, biy, lam_of_y)
    smooth(w, UX, UY, bix, biy, fewer)
    return w


def fpbipere(a, UX, UY, X, Y, ldzon, **kw):
    """a[f, KD1] -> new array.  The C+I rows lie X (ldzon) or UX apart on input and X apart on output."""
    nf = a.shape[0]
    w = np.zeros((Y, nf, X), dtype=a.dtype)
    ld = X if ldzon else UX
    for y in range(UY):
        w[y, :, :UX] = a[:, y * ld:y * ld + UX]
    core(w, UX, UY, **kw)
    out = a.copy()
    out[:, :X * Y] = w.transpose(1, 0, 2).reshape(nf, X * Y)
    return out


def etibihie(a, X, Y, UX, UY, kstart, bix, biy, **kw):
    """a[y, f, kstart..kdlsm] -> new array; x = 1 lies 1 - kstart elements into a row"""
    o = 1 - kstart
    out = a.copy()
    w = out[:, :, o:o + X].copy()
    w[UY:] = 0
    w[:, :, UX:] = 0
    core(w, UX, UY, bix, biy, **kw)
    out[:, :, o:o + X] = w
    return out


def boyd_window(n, scale, dtype):
    """b(j), j = 1..n (ewindowe_mod.F90:107-131); erf is evaluated in double on the argument of the routine's precision and rounded"""
    dt = np.dtype(dtype).type
    b = np.zeros(n, dtype=dtype)
    for j in range(1, n + 1):
        t = dt(-n - 1 + 2 * j) / dt(n + 1)
        l = t / np.sqrt(dt(1) - t * t)
        b[j - 1] = (dt(1) + dt(math.erf(float(dt(scale) * l)))) / dt(2)
    return b


def boyd(a, X, Y, bx, by):
    """a[f, (X + Wx) * (Y + Wy)] -> new array: the x blend on every row, then the y blend on every column"""
    Wx, Wy = len(bx), len(by)
    dt = a.dtype.type
    out = a.copy()
    w = out.reshape(a.shape[0], Y + Wy, X + Wx)
    w[:, :, X:] = bx * w[:, :, :Wx] + (dt(1) - bx) * w[:, :, X:]
    w[:, Y:, :] = by[:, None] * w[:, :Wy, :] + (dt(1) - by[:, None]) * w[:, Y:, :]
    return out


def horiz_field(kx, ky, dtype):
    """out[y, x].  The Fortran expression mixes default-real literals and integers with PPI, a JPRB parameter whose value is the
    default-real 3.141592: in the 4-byte library everything is real(4); in the 8-byte library (jx + 0.5 imax), (jy + 0.7 imax) and
    the literal 0.1 are real(4) values and the rest of the expression is real(8)."""
    dt = np.dtype(dtype).type
    f4 = np.float32
    imax = max(kx, ky)
    ppi = dt(f4(3.141592))
    jx = (np.arange(1, kx + 1).astype(f4) + f4(0.5) * f4(imax))[None, :]
    jy = (np.arange(1, ky + 1).astype(f4) + f4(0.7) * f4(imax))[:, None]
    arg = ppi * jx.astype(dtype) * jy.astype(dtype) / dt(imax ** 2) + dt(1)
    # the C library's sin / sinf, which the Fortran runtime and the library's host code call (NumPy's float32 sine is another routine)
    if np.dtype(dtype) == np.float64:
        s = np.array([[math.sin(float(v)) for v in row] for row in arg], dtype=dtype)
    else:
        s = np.array([[_libm().sinf(float(v)) for v in row] for row in arg], dtype=dtype)
    return dt(280) * (dt(1) + dt(f4(0.1)) * s)


def _libm():
    import ctypes
    import ctypes.util
    lm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lm.sinf.restype = ctypes.c_float
    lm.sinf.argtypes = [ctypes.c_float]
    return lm
