"""Cases and checks shared by tests/test_biper_emu.py (the CPU functional emulator) and tests/test_biper_gpu.py (the HIP library):
FPBIPERE, ETIBIHIE, Boyd's window and HORIZ_FIELD through the C-ABI and the Python layer, with host and device arrays, against the
goldens of tests/golden/biper (bytes of the reference's CPU routines, see its README.txt) and, beyond them, against the NumPy model
of tests/biper_ref.py, which tests/test_biper_model.py pins to the same goldens byte for byte.

Every comparison of spline / smoothing / blending output is for equal bytes: the kernels keep the reference's order of operations
and form no fused multiply-add, and +, -, *, / and the conversions from integers are correctly rounded on both sides.  The one bound
is on the weights of Boyd's window, which go through erf: 2 units in the last place, because two erf implementations that are each
within 1 ulp of the true value can differ by that much and the C library need not be the one the goldens were made with."""
import ctypes as C
import functools
import os

import numpy as np

from tests import biper_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "biper")
DT = {8: np.float64, 4: np.float32}
TAG = {8: "dp", 4: "sp"}
SENT = -777.25
# X, Y, UX, UY, fields
FP_CASES = [(14, 10, 9, 7, 2), (65, 66, 64, 63, 3), (70, 67, 58, 64, 1), (67, 70, 64, 58, 3)]
# X, Y, UX, UY, fields, LDBIX, LDBIY; KSTART = -1, KDLSM = KDLON + 2
ET_CASES = [(40, 12, 33, 12, 2, True, False), (12, 40, 12, 33, 2, False, True), (30, 28, 25, 21, 2, True, True)]
KSTART = -1
BOYD = (24, 22, 20, 18, 2, 3, 2.5)  # X, Y, UX, UY, fields, KDBOYD(3) = KDBOYD(6), PLBOYD
HORIZ = [(24, 18), (7, 31)]


@functools.lru_cache(maxsize=None)
def _load(name):
    a = np.load(os.path.join(GOLD, name + ".npy"))
    a.setflags(write=False)
    return a


def golden(name):
    return _load(name)


def fp_name(case, zon, esz):
    return "fpbipere_%dx%d_%dx%d_zon%d_%s" % (case[:4] + (int(zon), TAG[esz]))


def et_name(case, esz):
    return "etibihie_%dx%d_%dx%d_%s" % (case[:4] + (TAG[esz],))


def boyd_name(esz):
    return "boyd_%dx%d_%dx%d_%s" % (BOYD[:4] + (TAG[esz],))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Mem:
    """Where the array of a call lives.  host: a NumPy array, staged by the library.  device: a torch tensor on cuda:0; on the
    emulator, whose device memory is host memory, a NumPy array passed as EMI_MEM_DEVICE, which takes the in-place path."""

    def __init__(self, kind, emu):
        self.kind, self.emu = kind, emu
        self.space = 0 if kind == "host" else 1
        self.kw = {"mem_space": 1} if (emu and kind == "device") else {}

    def to(self, a):
        if self.kind == "host" or self.emu:
            return np.array(a, copy=True, order="C")
        import torch
        return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")

    def back(self, t):
        return t if isinstance(t, np.ndarray) else t.cpu().numpy()

    def ptr(self, t):
        return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def cabi_fpbipere(et, mem, t, esz, UX, UY, X, Y, knubi, kd1, kdadd=0, ldzon=0, ldboyd=0, kdboyd=None, plboyd=None):
    kb = None if kdboyd is None else (C.c_int * 6)(*kdboyd)
    pl = None if plboyd is None else C.byref(C.c_double(plboyd))
    return et.lib().emi_fpbipere(mem.space, esz, mem.ptr(t), UX, UY, X, Y, knubi, kd1, kdadd, int(ldzon), int(ldboyd), kb, pl)


def cabi_etibihie(et, mem, t, esz, X, Y, knubi, UX, UY, kstart, kdlsm, bix, biy, kdadd=0):
    return et.lib().emi_etibihie(mem.space, esz, mem.ptr(t), X, Y, knubi, UX, UY, kstart, kdlsm, int(bix), int(biy), kdadd)


def last_error(et):
    return et.lib().emi_last_error().decode()


# ---- the goldens ------------------------------------------------------------------------------------------------------------------
def golden_fpbipere(et, mem, case, zon, esz, via):
    """via "cabi": the call periodicises the first NF fields of an array of NF + 1; the surplus field, the tail of KD1 beyond X * Y and
    C+I must keep their input bytes.  via "py": the Python layer on the golden's own array."""
    X, Y, UX, UY, nf = case
    gin, gout = golden(fp_name(case, zon, esz) + "_in"), golden(fp_name(case, zon, esz) + "_out")
    kd1 = gin.shape[1]
    if via == "cabi":
        a = np.concatenate([gin, np.full((1, kd1), SENT, dtype=gin.dtype)])
        a[nf, ::3] = np.nan
        t = mem.to(a)
        rc = cabi_fpbipere(et, mem, t, esz, UX, UY, X, Y, nf, kd1, ldzon=zon)
        assert rc == 0, last_error(et)
        out = mem.back(t)
        assert same(out[nf], a[nf]), "the surplus field was written"
        out = out[:nf]
    else:
        t = mem.to(gin)
        et.fpbipere(t, UX, UY, X, Y, ldzon=bool(zon), **mem.kw)
        out = mem.back(t)
    assert same(out[:, X * Y:], gin[:, X * Y:]), "the tail of KD1 was written"
    if zon:
        v, g = out[:, :X * Y].reshape(nf, Y, X), gin[:, :X * Y].reshape(nf, Y, X)
        assert same(v[:, :UY, :UX], g[:, :UY, :UX]), "C+I was changed"
    assert np.isfinite(out[:, :X * Y]).all()
    assert same(out, gout), "max difference %g" % np.abs(out - gout).max()


def golden_etibihie(et, mem, case, esz, via):
    X, Y, UX, UY, nf, bix, biy = case
    gin, gout = golden(et_name(case, esz) + "_in"), golden(et_name(case, esz) + "_out")
    t = mem.to(gin)
    if via == "cabi":
        assert cabi_etibihie(et, mem, t, esz, X, Y, nf, UX, UY, KSTART, X + 2, bix, biy) == 0, last_error(et)
    else:
        et.etibihie(t, X, Y, UX, UY, KSTART, X + 2, bix, biy, **mem.kw)
    out = mem.back(t)
    o = 1 - KSTART
    assert same(out[:, :, :o], gin[:, :, :o]) and same(out[:, :, o + X:], gin[:, :, o + X:]), "the guard columns were written"
    assert same(out[:UY, :, o:o + UX], gin[:UY, :, o:o + UX]), "C+I was changed"
    assert same(out, gout), "max difference %g" % np.nanmax(np.abs(out - gout))


def ulps(a, b):
    it = np.int64 if a.dtype == np.float64 else np.int32
    return int(np.abs(a.view(it).astype(np.int64) - b.view(it).astype(np.int64)).max())


def golden_boyd(et, mem, esz, via):
    """the library's weights lie within 2 ulp of the golden ones (module docstring); the blended field is, byte for byte, what the
    model makes of the library's own weights"""
    X, Y, UX, UY, nf, bw, pl = BOYD
    Wx, Wy = 2 * bw + X - UX, 2 * bw + Y - UY
    nm = boyd_name(esz)
    gin = golden(nm + "_in")
    if via == "cabi":
        bx, by = np.zeros(Wx, dtype=DT[esz]), np.zeros(Wy, dtype=DT[esz])
        assert et.lib().emi_boyd_window(Wx, pl, esz, bx.ctypes.data) == 0 and et.lib().emi_boyd_window(Wy, pl, esz, by.ctypes.data) == 0
    else:
        bx, by = et.boyd_window(Wx, pl, DT[esz]), et.boyd_window(Wy, pl, DT[esz])
    ux, uy = ulps(bx, golden(nm + "_bx")), ulps(by, golden(nm + "_by"))
    print("Boyd weights: %d and %d ulp from the golden ones (bound 2)" % (ux, uy))
    assert ux <= 2 and uy <= 2
    t = mem.to(gin)
    kb = [0, 0, bw, 0, 0, bw]
    if via == "cabi":
        assert cabi_fpbipere(et, mem, t, esz, UX, UY, X, Y, nf, gin.shape[1], ldzon=1, ldboyd=1, kdboyd=kb, plboyd=pl) == 0, last_error(et)
    else:
        et.fpbipere(t, UX, UY, X, Y, ldzon=True, ldboyd=True, kdboyd=kb, plboyd=pl, **mem.kw)
    out = mem.back(t)
    assert same(out, R.boyd(gin, X, Y, bx, by))
    if ux == 0 and uy == 0:
        assert same(out, golden(nm + "_out"))


def golden_horiz(et, esz, via):
    for kx, ky in HORIZ:
        g = golden("horiz_field_%dx%d_%s" % (kx, ky, TAG[esz]))
        if via == "cabi":
            out = np.zeros((ky, kx), dtype=DT[esz])
            assert et.lib().emi_horiz_field(kx, ky, esz, out.ctypes.data) == 0
        else:
            out = et.horiz_field(kx, ky, DT[esz])
        assert same(out, g), np.abs(out - g).max()


# ---- beyond the goldens: against the model ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_case(X, Y, UX, UY, nf, esz, zon, tail, seed):
    """(input, model output) of an FPBIPERE call: C+I random in [-1, 1), E NaN, `tail` sentinels behind X * Y"""
    ci = np.random.default_rng(seed).uniform(-1.0, 1.0, (nf, UY, UX))
    a = np.full((nf, X * Y + tail), np.nan)
    a[:, X * Y:] = SENT
    if zon:
        a[:, :X * Y].reshape(nf, Y, X)[:, :UY, :UX] = ci
    else:
        a[:, :UX * UY] = ci.reshape(nf, -1)
    a = a.astype(DT[esz])
    ref = R.fpbipere(a, UX, UY, X, Y, zon)
    a.setflags(write=False)
    ref.setflags(write=False)
    return a, ref


def model_fpbipere(et, mem, X, Y, UX, UY, nf, esz, zon=True, tail=0, seed=11):
    a, ref = model_case(X, Y, UX, UY, nf, esz, zon, tail, seed)
    t = mem.to(a)
    et.fpbipere(t, UX, UY, X, Y, ldzon=zon, **mem.kw)
    out = mem.back(t)
    assert np.isfinite(out).all()
    assert same(out, ref), "max difference %g" % np.abs(out - ref).max()
    return a, out


def field_independence(et, mem, esz):
    """130 x 20 (C+I 127 x 9), 65 fields: the call equals the model, and field f is the same bytes when it is called alone and when
    the fields come in the opposite order"""
    X, Y, UX, UY, nf = 130, 20, 127, 9, 65
    a, out = model_fpbipere(et, mem, X, Y, UX, UY, nf, esz)
    for f in (0, 31, 64):
        t = mem.to(a[f:f + 1])
        et.fpbipere(t, UX, UY, X, Y, ldzon=True, **mem.kw)
        assert same(mem.back(t)[0], out[f]), f
    t = mem.to(a[::-1])
    et.fpbipere(t, UX, UY, X, Y, ldzon=True, **mem.kw)
    assert same(mem.back(t)[::-1], out)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def refusals(et, mem, esz):
    """every refusal returns its error, names the routine and leaves the array untouched, through the C-ABI and the Python layer"""
    X, Y, UX, UY, nf = 14, 10, 9, 7, 2
    rng = np.random.default_rng(5)
    kb = [0, 0, 2, 0, 0, 2]
    fp = [  # keyword changes of a good FPBIPERE call, and a piece of the message
        (dict(kdadd=1), "FPBIPERE: KDADD"),
        (dict(UX=1), "FPBIPERE: KDLUX = 1"),
        (dict(UY=1), "FPBIPERE: KDLUX = 9, KDGUX = 1"),
        (dict(UX=15), "FPBIPERE: KDLUX > KDLON"),
        (dict(UY=11), "FPBIPERE: KDLUX > KDLON OR KDGUX > KDGL"),
        (dict(kd1=X * Y - 1), "FPBIPERE: KD1 = 139 TOO SMALL"),
        (dict(ldboyd=1, plboyd=2.5), "FPBIPERE: Boyd periodization requires KDBOYD argument"),
        (dict(ldboyd=1, kdboyd=kb), "FPBIPERE: Boyd periodization requires PLBOYD argument"),
        (dict(ldboyd=1, kdboyd=kb, plboyd=2.5), "FPBIPERE: BOYD WINDOW WITH KDLON - KDLUX = 5 /= KDGL - KDGUX = 3"),
        (dict(ldboyd=1, kdboyd=kb, plboyd=2.5, UY=5), "FPBIPERE: BOYD WINDOW NEEDS KD1"),
        (dict(ldboyd=1, kdboyd=kb, plboyd=2.5, UY=5, nf=1), "FPBIPERE: KD1 = 141 TOO SMALL"),
        (dict(ldboyd=1, kdboyd=[0, 0, 5, 0, 0, 5], plboyd=2.5, UY=5, nf=1), "FPBIPERE: BOYD WINDOW WIDER THAN THE DOMAIN"),
    ]
    for ch, text in fp:
        q = dict(UX=UX, UY=UY, kd1=X * Y + 1, kdadd=0, nf=nf, ldboyd=0, kdboyd=None, plboyd=None)
        q.update(ch)
        a = rng.uniform(-1.0, 1.0, (q["nf"], q["kd1"])).astype(DT[esz])
        t = mem.to(a)
        rc = cabi_fpbipere(et, mem, t, esz, q["UX"], q["UY"], X, Y, q["nf"], q["kd1"], kdadd=q["kdadd"], ldzon=1, ldboyd=q["ldboyd"], kdboyd=q["kdboyd"],
                           plboyd=q["plboyd"])
        assert rc < 0 and text in last_error(et), (ch, rc, last_error(et))
        assert same(mem.back(t), a), ch
        try:
            et.fpbipere(t, q["UX"], q["UY"], X, Y, ldzon=True, ldboyd=bool(q["ldboyd"]), kdboyd=q["kdboyd"], plboyd=q["plboyd"], kdadd=q["kdadd"], **mem.kw)
        except et.TransError as e:
            assert text in str(e), (ch, str(e))
        else:
            raise AssertionError("not refused: %r" % (ch,))
        assert same(mem.back(t), a), ch
    X, Y, UX, UY, nf = 30, 28, 25, 21, 2
    ei = [
        (dict(kdadd=1), "ETIBIHIE: KDADD"),
        (dict(bix=False), "ETIBIHIE: LDBIX = .FALSE. REQUIRES KDLUX = KDLON"),
        (dict(biy=False), "ETIBIHIE: LDBIY = .FALSE. REQUIRES KDGUX = KDGL"),
        (dict(kstart=2), "ETIBIHIE: KSTART = 2 > 1"),
        (dict(kdlsm=X - 1), "ETIBIHIE: KSTART = -1 > 1 OR KDLSM = 29 < KDLON = 30"),
        (dict(UX=1), "ETIBIHIE: KDLUX = 1"),
        (dict(UY=1, bix=False, UX=X), "ETIBIHIE: KDLUX = 30, KDGUX = 1"),
        (dict(UX=31), "ETIBIHIE: KDLUX > KDLON"),
    ]
    for ch, text in ei:
        q = dict(UX=UX, UY=UY, kstart=KSTART, kdlsm=X + 2, kdadd=0, bix=True, biy=True)
        q.update(ch)
        a = rng.uniform(-1.0, 1.0, (Y, nf, q["kdlsm"] - q["kstart"] + 1)).astype(DT[esz])
        t = mem.to(a)
        rc = cabi_etibihie(et, mem, t, esz, X, Y, nf, q["UX"], q["UY"], q["kstart"], q["kdlsm"], q["bix"], q["biy"], kdadd=q["kdadd"])
        assert rc < 0 and text in last_error(et), (ch, rc, last_error(et))
        assert same(mem.back(t), a), ch
        try:
            et.etibihie(t, X, Y, q["UX"], q["UY"], q["kstart"], q["kdlsm"], q["bix"], q["biy"], kdadd=q["kdadd"], **mem.kw)
        except et.TransError as e:
            assert text in str(e), (ch, str(e))
        else:
            raise AssertionError("not refused: %r" % (ch,))
        assert same(mem.back(t), a), ch
    # both directions off: nothing to do, nothing written
    a = rng.uniform(-1.0, 1.0, (Y, nf, X + 4)).astype(DT[esz])
    t = mem.to(a)
    et.etibihie(t, X, Y, X, Y, KSTART, X + 2, False, False, **mem.kw)
    assert same(mem.back(t), a)
