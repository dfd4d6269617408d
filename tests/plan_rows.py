"""Limited-area handles whose rows all have one length and select one recorded FFT plan: what tests/test_gpu_mr_plans.py (the direct
mixed-radix plans of tests/mr_cover.py) and tests/test_gpu_conv_classes.py (the chirp-z and generic classes of tests/conv_cover.py) share.
`check(et, handle, n, precision)` is the plan assertion of the list that the caller works through."""
from tests.lam_common import lam_case, units
from tests.test_lam_gpu import TOL, mover, white_check

NDGL, KSMAX = 12, 5


class Handle:
    """a limited-area handle of NDGL rows of n points whose rows select the recorded plan of n"""

    def __init__(self, et, n, precision, check, kmsmax=None):
        self.et, self.n, self.precision, self.check = et, n, precision, check
        self.M = (n - 1) // 2 if kmsmax is None else kmsmax

    def __enter__(self):
        exwn, eywn = units(self.n, NDGL)
        self.r = self.et.esetup_trans(self.M, KSMAX, NDGL, kdlon=self.n, pexwn=exwn, peywn=eywn, precision=self.precision)
        try:
            self.check(self.et, self.r, self.n, self.precision)
        except BaseException:
            self.et.trans_release(self.r)
            raise
        return self

    def __exit__(self, *exc):
        self.et.trans_release(self.r)


def cut(n):
    """an odd NPROMA smaller than the row: rows cross blocks and fields start on odd elements -- the copy into the LDS with the pad index
    and the perm[] copy out of it"""
    return 4093 if n > 4093 else n - 1


def forward(et, n, precision, nproma, check, label, kmsmax=None):
    """lam_case (winds, scalars, all four flags) and lam_white_case on one handle, under the bounds of tests/test_lam_gpu.py; label: what
    the printed figures are called.  Returns the largest band-limited error."""
    to, back = mover("device", precision)
    with Handle(et, n, precision, check, kmsmax) as h:
        errs, _ = lam_case(et, n, NDGL, h.M, KSMAX, nproma=nproma, precision=precision, to_dev=to, to_host=back, kresol=h.r)
        print(label, "fp%d" % (8 * precision), "KMSMAX", h.M, "band-limited %.1e" % max(errs.values()))
        assert max(errs.values()) < TOL[precision], errs
        if precision == 4:
            assert max(errs.values()) > 1e-9  # really computed in float
        white_check(et, n, NDGL, h.M, KSMAX, "device", precision, "%s KMSMAX %d" % (label, h.M), nproma=nproma, kresol=h.r)
    return max(errs.values())
