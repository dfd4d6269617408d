"""The covering list of the chirp-z (Bluestein) and generic FFT classes -- every kernel family but the direct mixed-radix one, whose list
is tests/mr_cover.py --, shared by tests/test_emu_conv_classes.py and tests/test_gpu_conv_classes.py.

fft_choose (csrc/ectrans_mi.hip) gives a row of n points a kernel family (the "fftplan" inquiry: 0 generic in-LDS k_fft_inv / k_fft_dir,
1 k_fft_*_hot, 2 k_fft_*_r16, 3 k_fft_*_r16p, 5 k_fft_*_gm), a work length ("fftwork") and a number of fields per workgroup; the three
together are the CLASS of the row.  A class is one convolution length with one set of tables and one LDS layout, and the first and the
last row length of it are where it goes wrong first: the last one fills the convolution (2 sz - 1 of S points; a convolution one short
aliases into the top bins only), the first one leaves the most padding.  The generic kernels walk a factor list at run time (the
"fftfac" inquiry: pass count, then the factors); there every length is a class of its own.

COVER[precision] freezes (row length, switches, (family, work length, fields per workgroup)) as the three inquiries reported them when
the emulator library was asked for every even length 4 ... ENUM_EVEN and every odd length 3 ... ENUM_ODD (sphere handles with NSMAX = 1
and 60 row lengths per set-up; `python -m tests.conv_cover` repeats it), FACTORS[precision] the factor lists of the rows of the generic
passes (families 0 and 5).  CLASSES[precision] is the enumeration itself: (parity, family, work length, fields) -> (first, last length),
all 65 + 80 (fp64) and 46 + 80 (fp32) of them.  `choose` builds the list so that `missing` is empty:
  * default switches: the first and the last length of EVERY class of CLASSES -- the Bluestein ones (work length != sz) as the classes of
    families 1, 2, 3, 5 and the short and the odd rows of family 0, and the 7-smooth lengths with a run-time factor list, each its own first
    and last.  The last odd class is followed to its end (3071) beyond ENUM_ODD.  k_fft_*_gm: 10242 and 10486 in fp64; in fp32 the rows
    10242 ... 10486 are family 0 and the family starts above 20480 points: 20484 (GM_FP32) alone, because the tables of such a row take
    1.1 s of set-up each on the GPU host (S sz = 2.5e8 long-double terms of the filter sum), a test of it 1.1 ... 1.7 s in all;
  * the classes that only a switch reaches: k_fft_*_hot with S = 2048, 2560, 3072, 4096 (EMI_FFT_R16=0) and the in-place classes of the rows
    above 4096 points that the split kernels take by default (EMI_FFT_R16S=0), of each the longest row that the switch moves there;
  * EMI_FFT_MR=0: per family the longest row up to ENUM_EVEN whose half length is a product of three mixed-radix radices (fp32, family 5:
    24334 = 2 x 23^3, the only such row above 20480);
  * run-time factor lists, real-packed (even) and complex (odd) rows apart: every radix of the generic passes in the first, in an inner
    and in the last pass (a list of one pass counts as a first pass only), and every fields-per-workgroup value.  The rows with default switches do not suffice for the even ones (they
    are few and long), so the pool holds the mixed-radix rows under EMI_FFT_MR=0 too, and `choose` adds greedily from it.  NEVER lists
    what no row of the pool has: factorize_smooth orders a list 8 ... 8, 4 | 2, 3 ..., 5 ..., 7 ..., so 4 and 2 are never followed by an 8,
    and an odd row has the radices 3, 5, 7 only;
  * at least ODD_HALF even lengths with an odd half length (NLOEN = 2 mod 4: such a row never splits).
The tests assert through the inquiries that every length still selects its recorded class (`assert_class`), that the list still
covers all of the above, and that the neighbour of every first and last length lies in another class: a retuned fft_choose, hot-plan
list or LDS rule fails them by name instead of silently moving the tests onto other code.

What the list is for -- three mutations of a scratch emulator build (none committed), each run through tests/test_emu_conv_classes.py and
tests/test_emu_parity.py; the latter passes on all three:
  * the real-pack twiddles rtw[k], 100 < k < sz - 100, with the angle x 1.0001 (fft_fill_length): the whole rows of 638, 1028, 1250 and 1278
    points fail with 2.0e-4 ... 2.4e-4 (unmutated 1e-15; at KMSMAX = 15 the mutant is as good as the original);
  * the LDS swizzle with the mask 31 for 15 -- FPAD(i) = i ^ ((i >> 3) & 15) -- where k_fft_dir and k_fft_dir_hot read bin k out of the work
    array (the slots differ from k = 128 on): the same four rows fail with 0.92 ... 1.4;
  * `k2 < nmen` for `k2 <= nmen` where k_fft_inv_hot loads the mirror bin for fin_pair (bin sz - 1 of a full-bandwidth row is lost): the rows
    of 638, 1028 and 1278 points (k_fft_*_hot) fail with 3.9e-2 ... 5.4e-2.
"""
import contextlib
import os

ENUM_EVEN = 10488  # TCo2559-sized rows: the range that was enumerated
ENUM_ODD = 2999
ODD_END = 3101     # ... and how far the last odd class is followed
ODD_HALF = 5
GM_FP32 = 20484
MR_FORCED_FP32_GM = 24334
RADICES = (2, 3, 4, 5, 7, 8)  # the butterflies of the generic passes (FFT_DISPATCH, csrc/emi_kernels_body.h)
POSITIONS = ("first", "inner", "last")
MR_FAMILY, GM_FAMILY = 4, 5
SWITCHES = {"": {}, "MR=0": {"EMI_FFT_MR": "0"}, "R16=0": {"EMI_FFT_R16": "0"}, "R16S=0": {"EMI_FFT_R16S": "0"}}
HOT_ONLY_BY_SWITCH = {"R16=0": (2048, 2560, 3072, 4096), "R16S=0": (4608, 5120, 6144, 7680, 8192)}  # work lengths of k_fft_*_hot
MR_RADICES = {8: (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 23)}
MR_RADICES[4] = MR_RADICES[8] + (18, 20, 21)


def half(n):
    """the length of the complex transform of a row of n points"""
    return n if n % 2 else n // 2


def runtime_list(n, cls):
    """the row runs its own factor list through the generic passes (no convolution)"""
    return cls[0] == 0 and cls[1] == half(n)


def three_radices(sz, precision):
    rs = MR_RADICES[precision]
    return any(sz % a == 0 and (sz // a) % b == 0 and (sz // a) // b in rs for a in rs for b in rs)


def features(n, cls, fac):
    """what a row with a run-time factor list covers; a list of one pass counts as a first pass only -- a last pass comes after others,
    with their twiddles and strides"""
    f = {("fields", n % 2, cls[2]), ("radix", n % 2, fac[0], "first")}
    if len(fac) > 1:
        f.add(("radix", n % 2, fac[-1], "last"))
    return f | {("radix", n % 2, R, "inner") for R in fac[1:-1]}


def required(precision):
    full = {("radix", par, R, pos) for par in (0, 1) for R in RADICES for pos in POSITIONS}
    return (full | {("fields", par, k) for par in (0, 1) for k in FIELDS[precision][par]}) - set(NEVER[precision])


def missing(cover, precision, factors=None):
    """the coverage conditions that the list `cover` = [(n, switches, class)] does not meet (empty: all met)"""
    factors = FACTORS[precision] if factors is None else factors
    miss = []
    for key, ends in sorted(CLASSES[precision].items()):
        for n in sorted(set(ends)):
            if (n, "", key[1:]) not in cover or n % 2 != key[0]:
                miss.append(("class", key, n))
    for sw, works in HOT_ONLY_BY_SWITCH.items():
        for S in works:
            if not any(s == sw and c[:2] == (1, S) and (sw == "R16=0" or n > 4096) for n, s, c in cover):
                miss.append(("switch", sw, S))
    for fam in (0, 1, 2, 3, GM_FAMILY):
        if not any(s == "MR=0" and c[0] == fam and c[1] != half(n) and three_radices(n // 2, precision) for n, s, c in cover):
            miss.append(("EMI_FFT_MR=0", fam))
    have = set()
    for n, s, c in cover:
        if runtime_list(n, c):
            have |= features(n, c, factors[(n, s)])
    miss += sorted(required(precision) - have, key=str)
    odd = sum(n % 2 == 0 and (n // 2) % 2 for n, _, _ in cover)
    if odd < ODD_HALF:
        miss.append(("odd half lengths", odd))
    return miss


@contextlib.contextmanager
def switched(sw):
    """the switches of `sw` in the environment of the set-ups inside (the tests use monkeypatch.setenv instead)"""
    old = {k: os.environ.get(k) for k in SWITCHES[sw]}
    os.environ.update(SWITCHES[sw])
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


def enumerate_classes(et, precision, ns):
    """{n: (family, work length, fields per workgroup, factors)} of the row lengths `ns` through the "fftplan", "fftwork" and "fftfac"
    inquiries of the library behind `et`: sphere handles with NSMAX = 1 and 60 distinct row lengths each"""
    import numpy as np
    table, ns = {}, list(ns)
    for i in range(0, len(ns), 60):
        part = ns[i:i + 60]
        r = et.setup_trans(1, 2 * len(part), np.array(part + part[::-1], dtype=np.int32), precision=precision)
        try:
            plan, work, fac = et.trans_inq(r, "fftplan"), et.trans_inq(r, "fftwork"), et.trans_inq(r, "fftfac")
            for j, n in enumerate(part):
                table[n] = (int(plan[j][0]), int(work[j]), int(plan[j][4]), tuple(int(x) for x in fac[j][1:1 + fac[j][0]]))
        finally:
            et.trans_release(r)
    return table


def enumerate_all(et, precision):
    """the tables that `choose` needs, by switch: all lengths with default switches; the direct mixed-radix rows under EMI_FFT_MR=0; the
    40 lengths below each work length of HOT_ONLY_BY_SWITCH under its switch"""
    with switched(""):
        tabs = {"": enumerate_classes(et, precision, list(range(4, ENUM_EVEN + 1, 2)) + list(range(3, ODD_END + 1, 2)) +
                                      ([GM_FP32] if precision == 4 else []))}
    mr = [n for n, c in tabs[""].items() if c[0] == MR_FAMILY and n <= ENUM_EVEN]
    with switched("MR=0"):
        tabs["MR=0"] = enumerate_classes(et, precision, mr + ([MR_FORCED_FP32_GM] if precision == 4 else []))
    for sw, works in HOT_ONLY_BY_SWITCH.items():
        with switched(sw):
            tabs[sw] = enumerate_classes(et, precision, [n for S in works for n in range(S - 80, S + 2, 2)])
    return tabs


def choose(tabs, precision):
    """-> (cover, classes, factors, never, fields): see the module docstring"""
    D = tabs[""]
    classes = {}
    for n in sorted(D):
        key = (n % 2,) + D[n][:3]
        if D[n][0] == MR_FAMILY or (n > (ENUM_ODD if n % 2 else ENUM_EVEN) and key not in classes and n != GM_FP32):
            continue
        classes.setdefault(key, [n, n])[1] = n
    classes = {k: tuple(v) for k, v in classes.items()}
    cover = {(n, "", k[1:]) for k, v in classes.items() for n in v}
    for sw, works in HOT_ONLY_BY_SWITCH.items():  # the longest row that the switch moves into the class
        for S in works:
            n = max(n for n, c in tabs[sw].items() if c[:2] == (1, S) and D[n][0] in (2, 3))
            cover.add((n, sw, tabs[sw][n][:3]))
    F = tabs["MR=0"]
    for fam in (0, 1, 2, 3, GM_FAMILY):
        n = max(n for n, c in F.items() if c[0] == fam and c[1] != half(n) and three_radices(n // 2, precision))
        cover.add((n, "MR=0", F[n][:3]))
    pool = {(n, sw): c for sw in ("", "MR=0") for n, c in tabs[sw].items() if runtime_list(n, c) and (sw or (n % 2,) + c[:3] in classes)}
    feat = {k: features(k[0], c, c[3]) for k, c in pool.items()}
    allf = set().union(*feat.values())
    need = set(allf)
    for n, sw, c in cover:
        if (n, sw) in feat:
            need -= feat[(n, sw)]
    while need:  # the row that adds the most, the shorter one of equals
        k = max(feat, key=lambda k: (len(feat[k] & need), -k[0]))
        cover.add((k[0], k[1], pool[k][:3]))
        need -= feat[k]
    cover = sorted(cover)
    factors = {(n, sw): tabs[sw][n][3] for n, sw, c in cover if c[0] in (0, GM_FAMILY)}
    full = {("radix", par, R, pos) for par in (0, 1) for R in RADICES for pos in POSITIONS}
    fields = {par: tuple(sorted({f[2] for f in allf if f[0] == "fields" and f[1] == par})) for par in (0, 1)}
    return cover, classes, factors, sorted(full - allf), fields


def entries(precision, upto=None, sw=None):
    return [e for e in COVER[precision] if (upto is None or e[0] <= upto) and (sw is None or e[1] == sw)]


def last_entries(precision):
    """of every class (whatever the switches) the longest row of the list: where the cut rows and the adjoints run"""
    last = {}
    for e in COVER[precision]:
        k = (e[0] % 2,) + e[2]
        if k not in last or last[k][0] < e[0]:
            last[k] = e
    return sorted(last.values())


def thinned_entries(precision):
    """where the cut rows and the adjoints run: what they add to the whole rows is the grid-side copy of a row that crosses NPROMA blocks
    and the `adj` scalings, which are code of a kernel and not of a length.  Every class of the families 1, 2, 3 is a kernel of its own
    (a template instance per work length): the longest row of each.  The generic passes and their global-scratch twin are one kernel
    for all lengths: the longest row per (parity, family, convolution or run-time list, fields per workgroup)."""
    out = {}
    for e in last_entries(precision):
        n, _, c = e
        k = c if c[0] in (1, 2, 3) else (n % 2, c[0], runtime_list(n, c), c[2])
        if k not in out or out[k][0] < n:
            out[k] = e
    return sorted(out.values())


def ident(e, precision=None):
    return "%d%s%s" % (e[0], "-" + e[1] if e[1] else "", "-fp%d" % (8 * precision) if precision else "")


def assert_class(et, handle, n, precision, sw="", rows=None, inq=None):
    """the rows `rows` (default: all) of `handle` have n points: they select the class, and where recorded the factor list, of the entry
    (n, sw) of the list; inq: et.etrans_inq (default) or et.trans_inq"""
    inq = inq or et.etrans_inq
    want = [c for m, s, c in COVER[precision] if (m, s) == (n, sw)]
    assert len(want) == 1, (n, sw, want)
    plan, work, fac = inq(handle, "fftplan"), inq(handle, "fftwork"), inq(handle, "fftfac")
    rows = range(len(work)) if rows is None else rows
    got = {(int(plan[j][0]), int(work[j]), int(plan[j][4])) for j in rows}
    hint = " -- retuned fft_choose, hot-plan list or LDS rule?  Choose the covering list again (python -m tests.conv_cover, tests/conv_cover.py)"
    assert got == {want[0]}, "row length %d %s, precision %d: expected the class (family, work length, fields per workgroup) = %s, the library selects %s%s" % (
        n, sw, precision, want[0], sorted(got), hint)
    if (n, sw) in FACTORS[precision]:
        gotf = {tuple(int(x) for x in fac[j][1:1 + fac[j][0]]) for j in rows}
        assert gotf == {FACTORS[precision][(n, sw)]}, "row length %d %s, precision %d: expected the factor list %s, the library has %s%s" % (
            n, sw, precision, FACTORS[precision][(n, sw)], sorted(gotf), hint)


# ---- the frozen enumeration (python -m tests.conv_cover prints these tables) ------------------------------------------------------------
COVER = {4: [(3, '', (0, 3, 16)), (5, '', (0, 5, 16)), (7, '', (0, 7, 16)), (9, '', (0, 9, 16)), (11, '', (0, 24, 16)), (13, '', (0, 32, 16)),
     (15, '', (0, 15, 16)), (17, '', (0, 40, 16)), (19, '', (0, 40, 16)), (21, '', (0, 21, 16)), (23, '', (0, 64, 16)),
     (25, '', (0, 25, 16)), (27, '', (0, 27, 16)), (31, '', (0, 64, 16)), (33, '', (0, 72, 16)), (35, '', (0, 35, 16)),
     (37, '', (0, 80, 16)), (39, '', (0, 80, 16)), (41, '', (0, 96, 16)), (45, '', (0, 45, 16)), (47, '', (0, 96, 16)),
     (49, '', (0, 49, 16)), (51, '', (0, 120, 16)), (58, '', (0, 64, 16)), (59, '', (0, 120, 16)), (61, '', (0, 128, 16)),
     (62, '', (0, 64, 16)), (63, '', (0, 63, 16)), (64, 'MR=0', (0, 32, 16)), (65, '', (0, 160, 16)), (74, '', (0, 80, 16)),
     (75, '', (0, 75, 16)), (79, '', (0, 160, 16)), (81, '', (0, 81, 16)), (82, '', (0, 96, 16)), (83, '', (0, 192, 16)),
     (94, '', (0, 96, 16)), (95, '', (0, 192, 16)), (96, 'MR=0', (0, 48, 16)), (97, '', (0, 256, 16)), (105, '', (0, 105, 16)),
     (106, '', (0, 120, 16)), (118, '', (0, 120, 16)), (122, '', (0, 128, 16)), (124, '', (0, 128, 16)), (125, '', (0, 125, 16)),
     (127, '', (0, 256, 16)), (128, 'MR=0', (0, 64, 16)), (129, '', (0, 320, 16)), (134, '', (0, 160, 16)), (135, '', (0, 135, 16)),
     (147, '', (0, 147, 16)), (158, '', (0, 160, 16)), (159, '', (0, 320, 16)), (161, '', (0, 384, 8)), (164, '', (0, 192, 16)),
     (175, '', (0, 175, 16)), (188, '', (0, 192, 16)), (189, '', (0, 189, 16)), (191, '', (0, 384, 8)), (193, '', (0, 512, 8)),
     (194, '', (1, 256, 8)), (225, '', (0, 225, 16)), (243, '', (0, 243, 16)), (245, '', (0, 245, 16)), (254, '', (1, 256, 8)),
     (255, '', (0, 512, 8)), (256, 'MR=0', (0, 128, 16)), (257, '', (0, 576, 8)), (258, '', (1, 320, 8)), (287, '', (0, 576, 8)),
     (289, '', (0, 640, 8)), (315, '', (0, 315, 16)), (318, '', (1, 320, 8)), (319, '', (0, 640, 8)), (321, '', (0, 768, 4)),
     (326, '', (1, 384, 4)), (343, '', (0, 343, 8)), (375, '', (0, 375, 8)), (382, '', (1, 384, 4)), (383, '', (0, 768, 4)),
     (385, '', (0, 960, 4)), (386, '', (1, 512, 4)), (405, '', (0, 405, 8)), (441, '', (0, 441, 8)), (479, '', (0, 960, 4)),
     (481, '', (0, 1024, 4)), (508, '', (1, 512, 4)), (511, '', (0, 1024, 4)), (513, '', (0, 1280, 4)), (514, '', (1, 576, 4)),
     (525, '', (0, 525, 8)), (567, '', (0, 567, 8)), (574, '', (1, 576, 4)), (580, '', (1, 640, 4)), (625, '', (0, 625, 8)),
     (638, '', (1, 640, 4)), (639, '', (0, 1280, 4)), (641, '', (0, 1536, 2)), (642, '', (1, 768, 2)), (675, '', (0, 675, 4)),
     (729, '', (0, 729, 4)), (735, '', (0, 735, 4)), (766, '', (1, 768, 2)), (767, '', (0, 1536, 2)), (769, '', (0, 2048, 2)),
     (772, '', (1, 960, 2)), (875, '', (0, 875, 4)), (945, '', (0, 945, 4)), (958, '', (1, 960, 2)), (962, '', (1, 1024, 2)),
     (1022, '', (1, 1024, 2)), (1023, '', (0, 2048, 2)), (1025, '', (0, 2560, 2)), (1028, '', (1, 1280, 2)), (1029, '', (0, 1029, 4)),
     (1125, '', (0, 1125, 4)), (1215, '', (0, 1215, 4)), (1225, '', (0, 1225, 4)), (1250, '', (0, 625, 8)), (1278, '', (1, 1280, 2)),
     (1279, '', (0, 2560, 2)), (1281, '', (0, 3072, 1)), (1282, '', (1, 1536, 1)), (1323, '', (0, 1323, 2)), (1344, 'MR=0', (0, 672, 4)),
     (1534, '', (1, 1536, 1)), (1535, '', (0, 3072, 1)), (1537, '', (0, 4096, 1)), (1538, '', (2, 2048, 1)), (1575, '', (0, 1575, 2)),
     (1701, '', (0, 1701, 2)), (1715, '', (0, 1715, 2)), (1875, '', (0, 1875, 2)), (2025, '', (0, 2025, 2)), (2046, '', (2, 2048, 1)),
     (2046, 'R16=0', (1, 2048, 1)), (2047, '', (0, 4096, 1)), (2049, '', (0, 4608, 1)), (2050, '', (2, 2560, 1)), (2187, '', (0, 2187, 2)),
     (2205, '', (0, 2205, 2)), (2303, '', (0, 4608, 1)), (2305, '', (0, 5120, 1)), (2401, '', (0, 2401, 2)), (2558, '', (2, 2560, 1)),
     (2558, 'R16=0', (1, 2560, 1)), (2559, '', (0, 5120, 1)), (2561, '', (0, 6144, 1)), (2562, '', (2, 3072, 1)), (2625, '', (0, 2625, 1)),
     (2835, '', (0, 2835, 1)), (3070, '', (2, 3072, 1)), (3070, 'R16=0', (1, 3072, 1)), (3071, '', (0, 6144, 1)), (3074, '', (2, 4096, 1)),
     (4094, '', (2, 4096, 1)), (4094, 'R16=0', (1, 4096, 1)), (4096, 'MR=0', (2, 4096, 1)), (4098, '', (1, 4608, 1)),
     (4100, '', (3, 2560, 1)), (4374, '', (0, 2187, 2)), (4604, 'R16S=0', (1, 4608, 1)), (4606, '', (1, 4608, 1)), (4610, '', (1, 5120, 1)),
     (4802, '', (0, 2401, 2)), (5116, '', (3, 2560, 1)), (5116, 'R16S=0', (1, 5120, 1)), (5118, '', (1, 5120, 1)), (5122, '', (1, 6144, 1)),
     (5124, '', (3, 3072, 1)), (5250, '', (0, 2625, 1)), (6140, '', (3, 3072, 1)), (6140, 'R16S=0', (1, 6144, 1)), (6142, '', (1, 6144, 1)),
     (6146, '', (1, 7680, 1)), (6148, '', (3, 4096, 1)), (6250, '', (0, 3125, 1)), (7290, '', (0, 3645, 1)), (7350, '', (0, 3675, 1)),
     (7676, 'R16S=0', (1, 7680, 1)), (7678, '', (1, 7680, 1)), (7682, '', (1, 8192, 1)), (8160, 'MR=0', (3, 4096, 1)),
     (8186, '', (1, 8192, 1)), (8188, '', (3, 4096, 1)), (8188, 'R16S=0', (1, 8192, 1)), (8194, '', (1, 10240, 1)),
     (8748, '', (0, 4374, 1)), (8750, '', (0, 4375, 1)), (9604, '', (0, 4802, 1)), (9800, '', (0, 4900, 1)), (10000, '', (0, 5000, 1)),
     (10200, 'MR=0', (1, 10240, 1)), (10206, '', (0, 5103, 1)), (10238, '', (1, 10240, 1)), (10242, '', (0, 12288, 1)),
     (10290, '', (0, 5145, 1)), (10486, '', (0, 12288, 1)), (10488, 'MR=0', (0, 12288, 1)), (20484, '', (5, 24576, 1)),
     (24334, 'MR=0', (5, 24576, 1))],
 8: [(3, '', (0, 3, 16)), (5, '', (0, 5, 16)), (7, '', (0, 7, 16)), (9, '', (0, 9, 16)), (11, '', (0, 24, 16)), (13, '', (0, 32, 16)),
     (15, '', (0, 15, 16)), (17, '', (0, 40, 16)), (19, '', (0, 40, 16)), (21, '', (0, 21, 16)), (23, '', (0, 64, 16)),
     (25, '', (0, 25, 16)), (27, '', (0, 27, 16)), (31, '', (0, 64, 16)), (32, 'MR=0', (0, 16, 16)), (33, '', (0, 72, 16)),
     (35, '', (0, 35, 16)), (37, '', (0, 80, 16)), (39, '', (0, 80, 16)), (41, '', (0, 96, 16)), (45, '', (0, 45, 16)),
     (47, '', (0, 96, 16)), (49, '', (0, 49, 16)), (51, '', (0, 120, 16)), (58, '', (0, 64, 16)), (59, '', (0, 120, 16)),
     (61, '', (0, 128, 16)), (62, '', (0, 64, 16)), (63, '', (0, 63, 16)), (65, '', (0, 160, 16)), (74, '', (0, 80, 16)),
     (75, '', (0, 75, 16)), (79, '', (0, 160, 16)), (81, '', (0, 81, 16)), (82, '', (0, 96, 16)), (83, '', (0, 192, 8)),
     (94, '', (0, 96, 16)), (95, '', (0, 192, 8)), (97, '', (0, 256, 8)), (105, '', (0, 105, 16)), (106, '', (0, 120, 16)),
     (118, '', (0, 120, 16)), (122, '', (0, 128, 16)), (124, '', (0, 128, 16)), (125, '', (0, 125, 16)), (127, '', (0, 256, 8)),
     (128, 'MR=0', (0, 64, 16)), (129, '', (0, 320, 8)), (134, '', (0, 160, 16)), (135, '', (0, 135, 16)), (147, '', (0, 147, 16)),
     (158, '', (0, 160, 16)), (159, '', (0, 320, 8)), (161, '', (0, 384, 4)), (164, '', (0, 192, 8)), (175, '', (0, 175, 8)),
     (184, 'MR=0', (0, 192, 8)), (188, '', (0, 192, 8)), (189, '', (0, 189, 8)), (191, '', (0, 384, 4)), (193, '', (0, 512, 4)),
     (194, '', (1, 256, 8)), (225, '', (0, 225, 8)), (243, '', (0, 243, 8)), (245, '', (0, 245, 8)), (254, '', (1, 256, 8)),
     (255, '', (0, 512, 4)), (257, '', (0, 576, 4)), (258, '', (1, 320, 8)), (287, '', (0, 576, 4)), (289, '', (0, 640, 4)),
     (315, '', (0, 315, 8)), (318, '', (1, 320, 8)), (319, '', (0, 640, 4)), (321, '', (0, 768, 2)), (326, '', (1, 384, 4)),
     (343, '', (0, 343, 4)), (375, '', (0, 375, 4)), (382, '', (1, 384, 4)), (383, '', (0, 768, 2)), (385, '', (0, 960, 2)),
     (386, '', (1, 512, 4)), (405, '', (0, 405, 4)), (441, '', (0, 441, 4)), (479, '', (0, 960, 2)), (481, '', (0, 1024, 2)),
     (508, '', (1, 512, 4)), (511, '', (0, 1024, 2)), (512, 'MR=0', (0, 256, 8)), (513, '', (0, 1280, 2)), (514, '', (1, 576, 4)),
     (525, '', (0, 525, 4)), (567, '', (0, 567, 4)), (574, '', (1, 576, 4)), (580, '', (1, 640, 4)), (625, '', (0, 625, 4)),
     (638, '', (1, 640, 4)), (639, '', (0, 1280, 2)), (641, '', (0, 1536, 1)), (642, '', (1, 768, 2)), (675, '', (0, 675, 2)),
     (729, '', (0, 729, 2)), (735, '', (0, 735, 2)), (766, '', (1, 768, 2)), (767, '', (0, 1536, 1)), (769, '', (0, 2048, 1)),
     (772, '', (1, 960, 2)), (875, '', (0, 875, 2)), (945, '', (0, 945, 2)), (958, '', (1, 960, 2)), (962, '', (1, 1024, 2)),
     (1022, '', (1, 1024, 2)), (1023, '', (0, 2048, 1)), (1025, '', (0, 2560, 1)), (1028, '', (1, 1280, 2)), (1029, '', (0, 1029, 2)),
     (1125, '', (0, 1125, 2)), (1215, '', (0, 1215, 2)), (1225, '', (0, 1225, 2)), (1250, '', (0, 625, 4)), (1278, '', (1, 1280, 2)),
     (1279, '', (0, 2560, 1)), (1281, '', (0, 3072, 1)), (1282, '', (1, 1536, 1)), (1296, 'MR=0', (0, 648, 2)), (1323, '', (0, 1323, 1)),
     (1534, '', (1, 1536, 1)), (1535, '', (0, 3072, 1)), (1537, '', (0, 4096, 1)), (1538, '', (2, 2048, 1)), (1575, '', (0, 1575, 1)),
     (1701, '', (0, 1701, 1)), (1715, '', (0, 1715, 1)), (1875, '', (0, 1875, 1)), (2025, '', (0, 2025, 1)), (2046, '', (2, 2048, 1)),
     (2046, 'R16=0', (1, 2048, 1)), (2047, '', (0, 4096, 1)), (2049, '', (0, 4608, 1)), (2050, '', (2, 2560, 1)), (2187, '', (0, 2187, 1)),
     (2205, '', (0, 2205, 1)), (2303, '', (0, 4608, 1)), (2305, '', (0, 5120, 1)), (2401, '', (0, 2401, 1)), (2558, '', (2, 2560, 1)),
     (2558, 'R16=0', (1, 2560, 1)), (2559, '', (0, 5120, 1)), (2561, '', (0, 6144, 1)), (2562, '', (2, 3072, 1)), (2625, '', (0, 2625, 1)),
     (2835, '', (0, 2835, 1)), (3070, '', (2, 3072, 1)), (3070, 'R16=0', (1, 3072, 1)), (3071, '', (0, 6144, 1)), (3074, '', (2, 4096, 1)),
     (4094, '', (2, 4096, 1)), (4094, 'R16=0', (1, 4096, 1)), (4096, 'MR=0', (2, 4096, 1)), (4098, '', (1, 4608, 1)),
     (4100, '', (3, 2560, 1)), (4374, '', (0, 2187, 1)), (4410, '', (0, 2205, 1)), (4604, 'R16S=0', (1, 4608, 1)), (4606, '', (1, 4608, 1)),
     (4610, '', (1, 5120, 1)), (4802, '', (0, 2401, 1)), (5116, '', (3, 2560, 1)), (5116, 'R16S=0', (1, 5120, 1)), (5118, '', (1, 5120, 1)),
     (5122, '', (1, 6144, 1)), (5124, '', (3, 3072, 1)), (5250, '', (0, 2625, 1)), (5670, '', (0, 2835, 1)), (6140, '', (3, 3072, 1)),
     (6140, 'R16S=0', (1, 6144, 1)), (6142, '', (1, 6144, 1)), (6146, '', (1, 7680, 1)), (6148, '', (3, 4096, 1)), (6174, '', (0, 3087, 1)),
     (6250, '', (0, 3125, 1)), (7290, '', (0, 3645, 1)), (7350, '', (0, 3675, 1)), (7676, 'R16S=0', (1, 7680, 1)), (7678, '', (1, 7680, 1)),
     (7682, '', (1, 8192, 1)), (7938, '', (0, 3969, 1)), (8160, 'MR=0', (3, 4096, 1)), (8188, '', (3, 4096, 1)),
     (8188, 'R16S=0', (1, 8192, 1)), (8190, '', (1, 8192, 1)), (8194, '', (1, 10240, 1)), (8232, '', (0, 4116, 1)),
     (8400, '', (0, 4200, 1)), (8640, '', (0, 4320, 1)), (8748, '', (0, 4374, 1)), (8750, '', (0, 4375, 1)), (8820, '', (0, 4410, 1)),
     (8960, '', (0, 4480, 1)), (9000, '', (0, 4500, 1)), (9072, '', (0, 4536, 1)), (9216, '', (0, 4608, 1)), (9408, '', (0, 4704, 1)),
     (9450, '', (0, 4725, 1)), (9600, '', (0, 4800, 1)), (9604, '', (0, 4802, 1)), (9720, '', (0, 4860, 1)), (9800, '', (0, 4900, 1)),
     (10000, '', (0, 5000, 1)), (10080, '', (0, 5040, 1)), (10166, 'MR=0', (1, 10240, 1)), (10206, '', (0, 5103, 1)),
     (10238, '', (1, 10240, 1)), (10240, '', (0, 5120, 1)), (10242, '', (5, 12288, 1)), (10290, '', (0, 5145, 1)),
     (10368, '', (0, 5184, 1)), (10486, '', (5, 12288, 1)), (10488, 'MR=0', (5, 12288, 1))]}
CLASSES = {4: {(0, 0, 64, 16): (58, 62),
     (0, 0, 80, 16): (74, 74),
     (0, 0, 96, 16): (82, 94),
     (0, 0, 120, 16): (106, 118),
     (0, 0, 128, 16): (122, 124),
     (0, 0, 160, 16): (134, 158),
     (0, 0, 192, 16): (164, 188),
     (0, 0, 625, 8): (1250, 1250),
     (0, 0, 2187, 2): (4374, 4374),
     (0, 0, 2401, 2): (4802, 4802),
     (0, 0, 2625, 1): (5250, 5250),
     (0, 0, 3125, 1): (6250, 6250),
     (0, 0, 3645, 1): (7290, 7290),
     (0, 0, 3675, 1): (7350, 7350),
     (0, 0, 4374, 1): (8748, 8748),
     (0, 0, 4375, 1): (8750, 8750),
     (0, 0, 4802, 1): (9604, 9604),
     (0, 0, 4900, 1): (9800, 9800),
     (0, 0, 5000, 1): (10000, 10000),
     (0, 0, 5103, 1): (10206, 10206),
     (0, 0, 5145, 1): (10290, 10290),
     (0, 0, 12288, 1): (10242, 10486),
     (0, 1, 256, 8): (194, 254),
     (0, 1, 320, 8): (258, 318),
     (0, 1, 384, 4): (326, 382),
     (0, 1, 512, 4): (386, 508),
     (0, 1, 576, 4): (514, 574),
     (0, 1, 640, 4): (580, 638),
     (0, 1, 768, 2): (642, 766),
     (0, 1, 960, 2): (772, 958),
     (0, 1, 1024, 2): (962, 1022),
     (0, 1, 1280, 2): (1028, 1278),
     (0, 1, 1536, 1): (1282, 1534),
     (0, 1, 4608, 1): (4098, 4606),
     (0, 1, 5120, 1): (4610, 5118),
     (0, 1, 6144, 1): (5122, 6142),
     (0, 1, 7680, 1): (6146, 7678),
     (0, 1, 8192, 1): (7682, 8186),
     (0, 1, 10240, 1): (8194, 10238),
     (0, 2, 2048, 1): (1538, 2046),
     (0, 2, 2560, 1): (2050, 2558),
     (0, 2, 3072, 1): (2562, 3070),
     (0, 2, 4096, 1): (3074, 4094),
     (0, 3, 2560, 1): (4100, 5116),
     (0, 3, 3072, 1): (5124, 6140),
     (0, 3, 4096, 1): (6148, 8188),
     (0, 5, 24576, 1): (20484, 20484),
     (1, 0, 3, 16): (3, 3),
     (1, 0, 5, 16): (5, 5),
     (1, 0, 7, 16): (7, 7),
     (1, 0, 9, 16): (9, 9),
     (1, 0, 15, 16): (15, 15),
     (1, 0, 21, 16): (21, 21),
     (1, 0, 24, 16): (11, 11),
     (1, 0, 25, 16): (25, 25),
     (1, 0, 27, 16): (27, 27),
     (1, 0, 32, 16): (13, 13),
     (1, 0, 35, 16): (35, 35),
     (1, 0, 40, 16): (17, 19),
     (1, 0, 45, 16): (45, 45),
     (1, 0, 49, 16): (49, 49),
     (1, 0, 63, 16): (63, 63),
     (1, 0, 64, 16): (23, 31),
     (1, 0, 72, 16): (33, 33),
     (1, 0, 75, 16): (75, 75),
     (1, 0, 80, 16): (37, 39),
     (1, 0, 81, 16): (81, 81),
     (1, 0, 96, 16): (41, 47),
     (1, 0, 105, 16): (105, 105),
     (1, 0, 120, 16): (51, 59),
     (1, 0, 125, 16): (125, 125),
     (1, 0, 128, 16): (61, 61),
     (1, 0, 135, 16): (135, 135),
     (1, 0, 147, 16): (147, 147),
     (1, 0, 160, 16): (65, 79),
     (1, 0, 175, 16): (175, 175),
     (1, 0, 189, 16): (189, 189),
     (1, 0, 192, 16): (83, 95),
     (1, 0, 225, 16): (225, 225),
     (1, 0, 243, 16): (243, 243),
     (1, 0, 245, 16): (245, 245),
     (1, 0, 256, 16): (97, 127),
     (1, 0, 315, 16): (315, 315),
     (1, 0, 320, 16): (129, 159),
     (1, 0, 343, 8): (343, 343),
     (1, 0, 375, 8): (375, 375),
     (1, 0, 384, 8): (161, 191),
     (1, 0, 405, 8): (405, 405),
     (1, 0, 441, 8): (441, 441),
     (1, 0, 512, 8): (193, 255),
     (1, 0, 525, 8): (525, 525),
     (1, 0, 567, 8): (567, 567),
     (1, 0, 576, 8): (257, 287),
     (1, 0, 625, 8): (625, 625),
     (1, 0, 640, 8): (289, 319),
     (1, 0, 675, 4): (675, 675),
     (1, 0, 729, 4): (729, 729),
     (1, 0, 735, 4): (735, 735),
     (1, 0, 768, 4): (321, 383),
     (1, 0, 875, 4): (875, 875),
     (1, 0, 945, 4): (945, 945),
     (1, 0, 960, 4): (385, 479),
     (1, 0, 1024, 4): (481, 511),
     (1, 0, 1029, 4): (1029, 1029),
     (1, 0, 1125, 4): (1125, 1125),
     (1, 0, 1215, 4): (1215, 1215),
     (1, 0, 1225, 4): (1225, 1225),
     (1, 0, 1280, 4): (513, 639),
     (1, 0, 1323, 2): (1323, 1323),
     (1, 0, 1536, 2): (641, 767),
     (1, 0, 1575, 2): (1575, 1575),
     (1, 0, 1701, 2): (1701, 1701),
     (1, 0, 1715, 2): (1715, 1715),
     (1, 0, 1875, 2): (1875, 1875),
     (1, 0, 2025, 2): (2025, 2025),
     (1, 0, 2048, 2): (769, 1023),
     (1, 0, 2187, 2): (2187, 2187),
     (1, 0, 2205, 2): (2205, 2205),
     (1, 0, 2401, 2): (2401, 2401),
     (1, 0, 2560, 2): (1025, 1279),
     (1, 0, 2625, 1): (2625, 2625),
     (1, 0, 2835, 1): (2835, 2835),
     (1, 0, 3072, 1): (1281, 1535),
     (1, 0, 4096, 1): (1537, 2047),
     (1, 0, 4608, 1): (2049, 2303),
     (1, 0, 5120, 1): (2305, 2559),
     (1, 0, 6144, 1): (2561, 3071)},
 8: {(0, 0, 64, 16): (58, 62),
     (0, 0, 80, 16): (74, 74),
     (0, 0, 96, 16): (82, 94),
     (0, 0, 120, 16): (106, 118),
     (0, 0, 128, 16): (122, 124),
     (0, 0, 160, 16): (134, 158),
     (0, 0, 192, 8): (164, 188),
     (0, 0, 625, 4): (1250, 1250),
     (0, 0, 2187, 1): (4374, 4374),
     (0, 0, 2205, 1): (4410, 4410),
     (0, 0, 2401, 1): (4802, 4802),
     (0, 0, 2625, 1): (5250, 5250),
     (0, 0, 2835, 1): (5670, 5670),
     (0, 0, 3087, 1): (6174, 6174),
     (0, 0, 3125, 1): (6250, 6250),
     (0, 0, 3645, 1): (7290, 7290),
     (0, 0, 3675, 1): (7350, 7350),
     (0, 0, 3969, 1): (7938, 7938),
     (0, 0, 4116, 1): (8232, 8232),
     (0, 0, 4200, 1): (8400, 8400),
     (0, 0, 4320, 1): (8640, 8640),
     (0, 0, 4374, 1): (8748, 8748),
     (0, 0, 4375, 1): (8750, 8750),
     (0, 0, 4410, 1): (8820, 8820),
     (0, 0, 4480, 1): (8960, 8960),
     (0, 0, 4500, 1): (9000, 9000),
     (0, 0, 4536, 1): (9072, 9072),
     (0, 0, 4608, 1): (9216, 9216),
     (0, 0, 4704, 1): (9408, 9408),
     (0, 0, 4725, 1): (9450, 9450),
     (0, 0, 4800, 1): (9600, 9600),
     (0, 0, 4802, 1): (9604, 9604),
     (0, 0, 4860, 1): (9720, 9720),
     (0, 0, 4900, 1): (9800, 9800),
     (0, 0, 5000, 1): (10000, 10000),
     (0, 0, 5040, 1): (10080, 10080),
     (0, 0, 5103, 1): (10206, 10206),
     (0, 0, 5120, 1): (10240, 10240),
     (0, 0, 5145, 1): (10290, 10290),
     (0, 0, 5184, 1): (10368, 10368),
     (0, 1, 256, 8): (194, 254),
     (0, 1, 320, 8): (258, 318),
     (0, 1, 384, 4): (326, 382),
     (0, 1, 512, 4): (386, 508),
     (0, 1, 576, 4): (514, 574),
     (0, 1, 640, 4): (580, 638),
     (0, 1, 768, 2): (642, 766),
     (0, 1, 960, 2): (772, 958),
     (0, 1, 1024, 2): (962, 1022),
     (0, 1, 1280, 2): (1028, 1278),
     (0, 1, 1536, 1): (1282, 1534),
     (0, 1, 4608, 1): (4098, 4606),
     (0, 1, 5120, 1): (4610, 5118),
     (0, 1, 6144, 1): (5122, 6142),
     (0, 1, 7680, 1): (6146, 7678),
     (0, 1, 8192, 1): (7682, 8190),
     (0, 1, 10240, 1): (8194, 10238),
     (0, 2, 2048, 1): (1538, 2046),
     (0, 2, 2560, 1): (2050, 2558),
     (0, 2, 3072, 1): (2562, 3070),
     (0, 2, 4096, 1): (3074, 4094),
     (0, 3, 2560, 1): (4100, 5116),
     (0, 3, 3072, 1): (5124, 6140),
     (0, 3, 4096, 1): (6148, 8188),
     (0, 5, 12288, 1): (10242, 10486),
     (1, 0, 3, 16): (3, 3),
     (1, 0, 5, 16): (5, 5),
     (1, 0, 7, 16): (7, 7),
     (1, 0, 9, 16): (9, 9),
     (1, 0, 15, 16): (15, 15),
     (1, 0, 21, 16): (21, 21),
     (1, 0, 24, 16): (11, 11),
     (1, 0, 25, 16): (25, 25),
     (1, 0, 27, 16): (27, 27),
     (1, 0, 32, 16): (13, 13),
     (1, 0, 35, 16): (35, 35),
     (1, 0, 40, 16): (17, 19),
     (1, 0, 45, 16): (45, 45),
     (1, 0, 49, 16): (49, 49),
     (1, 0, 63, 16): (63, 63),
     (1, 0, 64, 16): (23, 31),
     (1, 0, 72, 16): (33, 33),
     (1, 0, 75, 16): (75, 75),
     (1, 0, 80, 16): (37, 39),
     (1, 0, 81, 16): (81, 81),
     (1, 0, 96, 16): (41, 47),
     (1, 0, 105, 16): (105, 105),
     (1, 0, 120, 16): (51, 59),
     (1, 0, 125, 16): (125, 125),
     (1, 0, 128, 16): (61, 61),
     (1, 0, 135, 16): (135, 135),
     (1, 0, 147, 16): (147, 147),
     (1, 0, 160, 16): (65, 79),
     (1, 0, 175, 8): (175, 175),
     (1, 0, 189, 8): (189, 189),
     (1, 0, 192, 8): (83, 95),
     (1, 0, 225, 8): (225, 225),
     (1, 0, 243, 8): (243, 243),
     (1, 0, 245, 8): (245, 245),
     (1, 0, 256, 8): (97, 127),
     (1, 0, 315, 8): (315, 315),
     (1, 0, 320, 8): (129, 159),
     (1, 0, 343, 4): (343, 343),
     (1, 0, 375, 4): (375, 375),
     (1, 0, 384, 4): (161, 191),
     (1, 0, 405, 4): (405, 405),
     (1, 0, 441, 4): (441, 441),
     (1, 0, 512, 4): (193, 255),
     (1, 0, 525, 4): (525, 525),
     (1, 0, 567, 4): (567, 567),
     (1, 0, 576, 4): (257, 287),
     (1, 0, 625, 4): (625, 625),
     (1, 0, 640, 4): (289, 319),
     (1, 0, 675, 2): (675, 675),
     (1, 0, 729, 2): (729, 729),
     (1, 0, 735, 2): (735, 735),
     (1, 0, 768, 2): (321, 383),
     (1, 0, 875, 2): (875, 875),
     (1, 0, 945, 2): (945, 945),
     (1, 0, 960, 2): (385, 479),
     (1, 0, 1024, 2): (481, 511),
     (1, 0, 1029, 2): (1029, 1029),
     (1, 0, 1125, 2): (1125, 1125),
     (1, 0, 1215, 2): (1215, 1215),
     (1, 0, 1225, 2): (1225, 1225),
     (1, 0, 1280, 2): (513, 639),
     (1, 0, 1323, 1): (1323, 1323),
     (1, 0, 1536, 1): (641, 767),
     (1, 0, 1575, 1): (1575, 1575),
     (1, 0, 1701, 1): (1701, 1701),
     (1, 0, 1715, 1): (1715, 1715),
     (1, 0, 1875, 1): (1875, 1875),
     (1, 0, 2025, 1): (2025, 2025),
     (1, 0, 2048, 1): (769, 1023),
     (1, 0, 2187, 1): (2187, 2187),
     (1, 0, 2205, 1): (2205, 2205),
     (1, 0, 2401, 1): (2401, 2401),
     (1, 0, 2560, 1): (1025, 1279),
     (1, 0, 2625, 1): (2625, 2625),
     (1, 0, 2835, 1): (2835, 2835),
     (1, 0, 3072, 1): (1281, 1535),
     (1, 0, 4096, 1): (1537, 2047),
     (1, 0, 4608, 1): (2049, 2303),
     (1, 0, 5120, 1): (2305, 2559),
     (1, 0, 6144, 1): (2561, 3071)}}
FACTORS = {4: {(3, ''): (3,),
     (5, ''): (5,),
     (7, ''): (7,),
     (9, ''): (3, 3),
     (11, ''): (8, 3),
     (13, ''): (8, 4),
     (15, ''): (3, 5),
     (17, ''): (8, 5),
     (19, ''): (8, 5),
     (21, ''): (3, 7),
     (23, ''): (8, 8),
     (25, ''): (5, 5),
     (27, ''): (3, 3, 3),
     (31, ''): (8, 8),
     (33, ''): (8, 3, 3),
     (35, ''): (5, 7),
     (37, ''): (8, 2, 5),
     (39, ''): (8, 2, 5),
     (41, ''): (8, 4, 3),
     (45, ''): (3, 3, 5),
     (47, ''): (8, 4, 3),
     (49, ''): (7, 7),
     (51, ''): (8, 3, 5),
     (58, ''): (8, 8),
     (59, ''): (8, 3, 5),
     (61, ''): (8, 8, 2),
     (62, ''): (8, 8),
     (63, ''): (3, 3, 7),
     (64, 'MR=0'): (8, 4),
     (65, ''): (8, 4, 5),
     (74, ''): (8, 2, 5),
     (75, ''): (3, 5, 5),
     (79, ''): (8, 4, 5),
     (81, ''): (3, 3, 3, 3),
     (82, ''): (8, 4, 3),
     (83, ''): (8, 8, 3),
     (94, ''): (8, 4, 3),
     (95, ''): (8, 8, 3),
     (96, 'MR=0'): (8, 2, 3),
     (97, ''): (8, 8, 4),
     (105, ''): (3, 5, 7),
     (106, ''): (8, 3, 5),
     (118, ''): (8, 3, 5),
     (122, ''): (8, 8, 2),
     (124, ''): (8, 8, 2),
     (125, ''): (5, 5, 5),
     (127, ''): (8, 8, 4),
     (128, 'MR=0'): (8, 8),
     (129, ''): (8, 8, 5),
     (134, ''): (8, 4, 5),
     (135, ''): (3, 3, 3, 5),
     (147, ''): (3, 7, 7),
     (158, ''): (8, 4, 5),
     (159, ''): (8, 8, 5),
     (161, ''): (8, 8, 2, 3),
     (164, ''): (8, 8, 3),
     (175, ''): (5, 5, 7),
     (188, ''): (8, 8, 3),
     (189, ''): (3, 3, 3, 7),
     (191, ''): (8, 8, 2, 3),
     (193, ''): (8, 8, 8),
     (225, ''): (3, 3, 5, 5),
     (243, ''): (3, 3, 3, 3, 3),
     (245, ''): (5, 7, 7),
     (255, ''): (8, 8, 8),
     (256, 'MR=0'): (8, 8, 2),
     (257, ''): (8, 8, 3, 3),
     (287, ''): (8, 8, 3, 3),
     (289, ''): (8, 8, 2, 5),
     (315, ''): (3, 3, 5, 7),
     (319, ''): (8, 8, 2, 5),
     (321, ''): (8, 8, 4, 3),
     (343, ''): (7, 7, 7),
     (375, ''): (3, 5, 5, 5),
     (383, ''): (8, 8, 4, 3),
     (385, ''): (8, 8, 3, 5),
     (405, ''): (3, 3, 3, 3, 5),
     (441, ''): (3, 3, 7, 7),
     (479, ''): (8, 8, 3, 5),
     (481, ''): (8, 8, 8, 2),
     (511, ''): (8, 8, 8, 2),
     (513, ''): (8, 8, 4, 5),
     (525, ''): (3, 5, 5, 7),
     (567, ''): (3, 3, 3, 3, 7),
     (625, ''): (5, 5, 5, 5),
     (639, ''): (8, 8, 4, 5),
     (641, ''): (8, 8, 8, 3),
     (675, ''): (3, 3, 3, 5, 5),
     (729, ''): (3, 3, 3, 3, 3, 3),
     (735, ''): (3, 5, 7, 7),
     (767, ''): (8, 8, 8, 3),
     (769, ''): (8, 8, 8, 4),
     (875, ''): (5, 5, 5, 7),
     (945, ''): (3, 3, 3, 5, 7),
     (1023, ''): (8, 8, 8, 4),
     (1025, ''): (8, 8, 8, 5),
     (1029, ''): (3, 7, 7, 7),
     (1125, ''): (3, 3, 5, 5, 5),
     (1215, ''): (3, 3, 3, 3, 3, 5),
     (1225, ''): (5, 5, 7, 7),
     (1250, ''): (5, 5, 5, 5),
     (1279, ''): (8, 8, 8, 5),
     (1281, ''): (8, 8, 8, 2, 3),
     (1323, ''): (3, 3, 3, 7, 7),
     (1344, 'MR=0'): (8, 4, 3, 7),
     (1535, ''): (8, 8, 8, 2, 3),
     (1537, ''): (8, 8, 8, 8),
     (1575, ''): (3, 3, 5, 5, 7),
     (1701, ''): (3, 3, 3, 3, 3, 7),
     (1715, ''): (5, 7, 7, 7),
     (1875, ''): (3, 5, 5, 5, 5),
     (2025, ''): (3, 3, 3, 3, 5, 5),
     (2047, ''): (8, 8, 8, 8),
     (2049, ''): (8, 8, 8, 3, 3),
     (2187, ''): (3, 3, 3, 3, 3, 3, 3),
     (2205, ''): (3, 3, 5, 7, 7),
     (2303, ''): (8, 8, 8, 3, 3),
     (2305, ''): (8, 8, 8, 2, 5),
     (2401, ''): (7, 7, 7, 7),
     (2559, ''): (8, 8, 8, 2, 5),
     (2561, ''): (8, 8, 8, 4, 3),
     (2625, ''): (3, 5, 5, 5, 7),
     (2835, ''): (3, 3, 3, 3, 5, 7),
     (3071, ''): (8, 8, 8, 4, 3),
     (4374, ''): (3, 3, 3, 3, 3, 3, 3),
     (4802, ''): (7, 7, 7, 7),
     (5250, ''): (3, 5, 5, 5, 7),
     (6250, ''): (5, 5, 5, 5, 5),
     (7290, ''): (3, 3, 3, 3, 3, 3, 5),
     (7350, ''): (3, 5, 5, 7, 7),
     (8748, ''): (2, 3, 3, 3, 3, 3, 3, 3),
     (8750, ''): (5, 5, 5, 5, 7),
     (9604, ''): (2, 7, 7, 7, 7),
     (9800, ''): (4, 5, 5, 7, 7),
     (10000, ''): (8, 5, 5, 5, 5),
     (10206, ''): (3, 3, 3, 3, 3, 3, 7),
     (10242, ''): (8, 8, 8, 8, 3),
     (10290, ''): (3, 5, 7, 7, 7),
     (10486, ''): (8, 8, 8, 8, 3),
     (10488, 'MR=0'): (8, 8, 8, 8, 3),
     (20484, ''): (8, 8, 8, 8, 2, 3),
     (24334, 'MR=0'): (8, 8, 8, 8, 2, 3)},
 8: {(3, ''): (3,),
     (5, ''): (5,),
     (7, ''): (7,),
     (9, ''): (3, 3),
     (11, ''): (8, 3),
     (13, ''): (8, 4),
     (15, ''): (3, 5),
     (17, ''): (8, 5),
     (19, ''): (8, 5),
     (21, ''): (3, 7),
     (23, ''): (8, 8),
     (25, ''): (5, 5),
     (27, ''): (3, 3, 3),
     (31, ''): (8, 8),
     (32, 'MR=0'): (8, 2),
     (33, ''): (8, 3, 3),
     (35, ''): (5, 7),
     (37, ''): (8, 2, 5),
     (39, ''): (8, 2, 5),
     (41, ''): (8, 4, 3),
     (45, ''): (3, 3, 5),
     (47, ''): (8, 4, 3),
     (49, ''): (7, 7),
     (51, ''): (8, 3, 5),
     (58, ''): (8, 8),
     (59, ''): (8, 3, 5),
     (61, ''): (8, 8, 2),
     (62, ''): (8, 8),
     (63, ''): (3, 3, 7),
     (65, ''): (8, 4, 5),
     (74, ''): (8, 2, 5),
     (75, ''): (3, 5, 5),
     (79, ''): (8, 4, 5),
     (81, ''): (3, 3, 3, 3),
     (82, ''): (8, 4, 3),
     (83, ''): (8, 8, 3),
     (94, ''): (8, 4, 3),
     (95, ''): (8, 8, 3),
     (97, ''): (8, 8, 4),
     (105, ''): (3, 5, 7),
     (106, ''): (8, 3, 5),
     (118, ''): (8, 3, 5),
     (122, ''): (8, 8, 2),
     (124, ''): (8, 8, 2),
     (125, ''): (5, 5, 5),
     (127, ''): (8, 8, 4),
     (128, 'MR=0'): (8, 8),
     (129, ''): (8, 8, 5),
     (134, ''): (8, 4, 5),
     (135, ''): (3, 3, 3, 5),
     (147, ''): (3, 7, 7),
     (158, ''): (8, 4, 5),
     (159, ''): (8, 8, 5),
     (161, ''): (8, 8, 2, 3),
     (164, ''): (8, 8, 3),
     (175, ''): (5, 5, 7),
     (184, 'MR=0'): (8, 8, 3),
     (188, ''): (8, 8, 3),
     (189, ''): (3, 3, 3, 7),
     (191, ''): (8, 8, 2, 3),
     (193, ''): (8, 8, 8),
     (225, ''): (3, 3, 5, 5),
     (243, ''): (3, 3, 3, 3, 3),
     (245, ''): (5, 7, 7),
     (255, ''): (8, 8, 8),
     (257, ''): (8, 8, 3, 3),
     (287, ''): (8, 8, 3, 3),
     (289, ''): (8, 8, 2, 5),
     (315, ''): (3, 3, 5, 7),
     (319, ''): (8, 8, 2, 5),
     (321, ''): (8, 8, 4, 3),
     (343, ''): (7, 7, 7),
     (375, ''): (3, 5, 5, 5),
     (383, ''): (8, 8, 4, 3),
     (385, ''): (8, 8, 3, 5),
     (405, ''): (3, 3, 3, 3, 5),
     (441, ''): (3, 3, 7, 7),
     (479, ''): (8, 8, 3, 5),
     (481, ''): (8, 8, 8, 2),
     (511, ''): (8, 8, 8, 2),
     (512, 'MR=0'): (8, 8, 4),
     (513, ''): (8, 8, 4, 5),
     (525, ''): (3, 5, 5, 7),
     (567, ''): (3, 3, 3, 3, 7),
     (625, ''): (5, 5, 5, 5),
     (639, ''): (8, 8, 4, 5),
     (641, ''): (8, 8, 8, 3),
     (675, ''): (3, 3, 3, 5, 5),
     (729, ''): (3, 3, 3, 3, 3, 3),
     (735, ''): (3, 5, 7, 7),
     (767, ''): (8, 8, 8, 3),
     (769, ''): (8, 8, 8, 4),
     (875, ''): (5, 5, 5, 7),
     (945, ''): (3, 3, 3, 5, 7),
     (1023, ''): (8, 8, 8, 4),
     (1025, ''): (8, 8, 8, 5),
     (1029, ''): (3, 7, 7, 7),
     (1125, ''): (3, 3, 5, 5, 5),
     (1215, ''): (3, 3, 3, 3, 3, 5),
     (1225, ''): (5, 5, 7, 7),
     (1250, ''): (5, 5, 5, 5),
     (1279, ''): (8, 8, 8, 5),
     (1281, ''): (8, 8, 8, 2, 3),
     (1296, 'MR=0'): (8, 3, 3, 3, 3),
     (1323, ''): (3, 3, 3, 7, 7),
     (1535, ''): (8, 8, 8, 2, 3),
     (1537, ''): (8, 8, 8, 8),
     (1575, ''): (3, 3, 5, 5, 7),
     (1701, ''): (3, 3, 3, 3, 3, 7),
     (1715, ''): (5, 7, 7, 7),
     (1875, ''): (3, 5, 5, 5, 5),
     (2025, ''): (3, 3, 3, 3, 5, 5),
     (2047, ''): (8, 8, 8, 8),
     (2049, ''): (8, 8, 8, 3, 3),
     (2187, ''): (3, 3, 3, 3, 3, 3, 3),
     (2205, ''): (3, 3, 5, 7, 7),
     (2303, ''): (8, 8, 8, 3, 3),
     (2305, ''): (8, 8, 8, 2, 5),
     (2401, ''): (7, 7, 7, 7),
     (2559, ''): (8, 8, 8, 2, 5),
     (2561, ''): (8, 8, 8, 4, 3),
     (2625, ''): (3, 5, 5, 5, 7),
     (2835, ''): (3, 3, 3, 3, 5, 7),
     (3071, ''): (8, 8, 8, 4, 3),
     (4374, ''): (3, 3, 3, 3, 3, 3, 3),
     (4410, ''): (3, 3, 5, 7, 7),
     (4802, ''): (7, 7, 7, 7),
     (5250, ''): (3, 5, 5, 5, 7),
     (5670, ''): (3, 3, 3, 3, 5, 7),
     (6174, ''): (3, 3, 7, 7, 7),
     (6250, ''): (5, 5, 5, 5, 5),
     (7290, ''): (3, 3, 3, 3, 3, 3, 5),
     (7350, ''): (3, 5, 5, 7, 7),
     (7938, ''): (3, 3, 3, 3, 7, 7),
     (8232, ''): (4, 3, 7, 7, 7),
     (8400, ''): (8, 3, 5, 5, 7),
     (8640, ''): (8, 4, 3, 3, 3, 5),
     (8748, ''): (2, 3, 3, 3, 3, 3, 3, 3),
     (8750, ''): (5, 5, 5, 5, 7),
     (8820, ''): (2, 3, 3, 5, 7, 7),
     (8960, ''): (8, 8, 2, 5, 7),
     (9000, ''): (4, 3, 3, 5, 5, 5),
     (9072, ''): (8, 3, 3, 3, 3, 7),
     (9216, ''): (8, 8, 8, 3, 3),
     (9408, ''): (8, 4, 3, 7, 7),
     (9450, ''): (3, 3, 3, 5, 5, 7),
     (9600, ''): (8, 8, 3, 5, 5),
     (9604, ''): (2, 7, 7, 7, 7),
     (9720, ''): (4, 3, 3, 3, 3, 3, 5),
     (9800, ''): (4, 5, 5, 7, 7),
     (10000, ''): (8, 5, 5, 5, 5),
     (10080, ''): (8, 2, 3, 3, 5, 7),
     (10206, ''): (3, 3, 3, 3, 3, 3, 7),
     (10240, ''): (8, 8, 8, 2, 5),
     (10242, ''): (8, 8, 8, 8, 3),
     (10290, ''): (3, 5, 7, 7, 7),
     (10368, ''): (8, 8, 3, 3, 3, 3),
     (10486, ''): (8, 8, 8, 8, 3),
     (10488, 'MR=0'): (8, 8, 8, 8, 3)}}
NEVER = {4: [('radix', 1, 2, 'first'), ('radix', 1, 2, 'inner'), ('radix', 1, 2, 'last'), ('radix', 1, 4, 'first'), ('radix', 1, 4, 'inner'),
     ('radix', 1, 4, 'last'), ('radix', 1, 8, 'first'), ('radix', 1, 8, 'inner'), ('radix', 1, 8, 'last')],
 8: [('radix', 1, 2, 'first'), ('radix', 1, 2, 'inner'), ('radix', 1, 2, 'last'), ('radix', 1, 4, 'first'), ('radix', 1, 4, 'inner'),
     ('radix', 1, 4, 'last'), ('radix', 1, 8, 'first'), ('radix', 1, 8, 'inner'), ('radix', 1, 8, 'last')]}
FIELDS = {4: {0: (1, 2, 4, 8, 16), 1: (1, 2, 4, 8, 16)}, 8: {0: (1, 2, 4, 8, 16), 1: (1, 2, 4, 8, 16)}}


if __name__ == "__main__":  # choose the lists again, on the emulator library: python -m tests.conv_cover (two minutes on 8 cores)
    import pprint
    import ectrans_amd
    ectrans_amd._use_library_for_tests(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libectrans_mi_emu.so"))
    ectrans_amd.setup_trans0(kmax_resol=4)
    out = {}
    for prec in (8, 4):
        out[prec] = choose(enumerate_all(ectrans_amd, prec), prec)
    same = True
    for i, name in enumerate(("COVER", "CLASSES", "FACTORS", "NEVER", "FIELDS")):
        new = {p: out[p][i] for p in (8, 4)}
        same = same and new == globals().get(name)
        print("%s = %s" % (name, pprint.pformat(new, width=140, compact=True)))
    for prec in (8, 4):
        even, odd = (sum(k[0] == par for k in out[prec][1]) for par in (0, 1))
        print("# precision %d: %d even and %d odd classes, %d lengths in the list; missing: %s" % (prec, even, odd, len(out[prec][0]), missing(out[prec][0], prec) if same else "?"))
    print("# the committed tables are %s" % ("reproduced" if same else "NOT reproduced"))
