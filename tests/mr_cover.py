"""The covering list of the direct mixed-radix FFT plans (k_fft_dir_mr / k_fft_inv_mr, csrc/emi_mr_body.h), shared by
tests/test_emu_mr_plans.py and tests/test_gpu_mr_plans.py.

mr_choose (csrc/ectrans_mi.hip) picks the plan (A, B, C) of a row by a cost model; nobody chooses which radix lands in which pass.
COVER[precision] therefore freezes, per library precision, a list of row lengths WITH the plan each is expected to select -- as the
"fftplan" inquiry reported it when the plan of every even length up to ENUM_MAX was enumerated through the emulator library (sphere
handles with NSMAX = 1 and 60 distinct row lengths per set-up; 747 direct plans in the fp64 library, 877 in the fp32 one) -- chosen
greedily (`greedy`) so that the list meets `required(precision)`:
  * every radix of the precision in every pass position A, B, C (the fp32-only radices 18, 20, 21 never come first: no length selects
    them there);
  * one-, two- and three-pass plans;
  * the padded row pitch P1 = (B C) | 1 with pad 1 (B C even) and pad 0 (B C odd);
  * every fields-per-workgroup value 1, 2, 4, 8, 16 -- so the one-field branch (fbk == 1) of k_fft_inv_mr and the several-fields one;
  * at least ODD_HALF lengths with an odd half length;
  * the longest direct plan up to ENUM_MAX, and the longest one the family has at all (LONGEST: the work array fills the LDS).
The tests assert through the inquiry that every length still selects its recorded plan and (`missing`) that the list still covers
all of the above: a retuned mr_choose fails them by name instead of silently moving the tests onto other code."""

ENUM_MAX = 10488  # TCo2559-sized rows: the range that was enumerated
ODD_HALF = 5
RADICES = {8: (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 23)}  # EMI_MR_RADICES
RADICES[4] = RADICES[8] + (18, 20, 21)                                           # + EMI_MR_RADICES_F32
NEVER_FIRST = (18, 20, 21)
FIELDS = (1, 2, 4, 8, 16)
MR_FAMILY = 4  # "fftplan": 0 generic, 1 specialised in place, 2 register-resident, 3 split, 4 direct mixed radix, 5 global scratch


def features(n, plan):
    """what a row of n points with plan (A, B, C, fields per workgroup) covers"""
    A, B, C, fbk = plan
    f = {("radix", R, "ABC"[slot]) for slot, R in enumerate((A, B, C)) if R > 1}
    f.add(("passes", sum(R > 1 for R in (A, B, C))))
    f.add(("pad", 1 - (B * C) % 2))
    f.add(("fields", fbk))
    return f


def required(precision):
    req = {("radix", R, s) for R in RADICES[precision] for s in "ABC" if not (s == "A" and R in NEVER_FIRST)}
    req |= {("passes", k) for k in (1, 2, 3)} | {("pad", 0), ("pad", 1)} | {("fields", k) for k in FIELDS}
    return req


def missing(cover, precision):
    """the coverage conditions that the list `cover` = [(n, (A, B, C, fbk))] does not meet (empty: all met)"""
    have = set()
    for n, plan in cover:
        have |= features(n, plan)
    miss = sorted(required(precision) - have, key=str)
    odd = sum((n // 2) % 2 for n, _ in cover)
    if odd < ODD_HALF:
        miss.append(("odd half lengths", odd))
    for n in (ENUM_MAX, LONGEST[precision]):
        if n not in [c[0] for c in cover]:
            miss.append(("longest", n))
    return miss


def greedy(table, precision):
    """table {n: (A, B, C, fbk)} of every direct plan -> a covering list: the longest lengths, then repeatedly the length that adds the
    most missing features (ties: odd half length while fewer than ODD_HALF, then the shorter row), then odd half lengths as needed;
    lengths that the later choices made redundant are dropped again"""
    cover = [(n, table[n]) for n in sorted({max(k for k in table if k <= ENUM_MAX), max(table)})]
    need = set(required(precision))
    for n, p in cover:
        need -= features(n, p)
    while need:
        odd = sum((n // 2) % 2 for n, _ in cover)
        n = max(table, key=lambda k: (len(features(k, table[k]) & need), (k // 2) % 2 if odd < ODD_HALF else 0, -k))
        assert features(n, table[n]) & need, need
        cover.append((n, table[n]))
        need -= features(n, table[n])
    for n in sorted(table):
        if sum((k // 2) % 2 for k, _ in cover) >= ODD_HALF:
            break
        if (n // 2) % 2 and n not in [c[0] for c in cover]:
            cover.append((n, table[n]))
    for c in sorted(cover):  # keep the list minimal: every length is the only one for something
        rest = [x for x in cover if x != c]
        if not missing(rest, precision):
            cover = rest
    return sorted(cover)


def enumerate_plans(et, precision, ns):
    """{n: (A, B, C, fbk)} of those row lengths of `ns` that select a direct plan, through the "fftplan" inquiry of the library behind
    `et`: sphere handles with NSMAX = 1 and 60 distinct row lengths each, so that the per-length tables stay small"""
    import numpy as np
    table, ns = {}, list(ns)
    for i in range(0, len(ns), 60):
        half = ns[i:i + 60]
        r = et.setup_trans(1, 2 * len(half), np.array(half + half[::-1], dtype=np.int32), precision=precision)
        try:
            for n, row in zip(half, et.trans_inq(r, "fftplan")):
                if row[0] == MR_FAMILY:
                    table[n] = tuple(int(x) for x in row[1:])
        finally:
            et.trans_release(r)
    return table


def three_radices(sz, precision):
    """sz is a product of at most three radices: what a direct plan needs at least (beyond ENUM_MAX only such lengths are asked for --
    the convolution tables of the others take minutes to set up)"""
    rs = RADICES[precision]
    return any(sz % a == 0 and (sz // a == 1 or any((sz // a) % b == 0 and ((sz // a) // b == 1 or (sz // a) // b in rs) for b in rs)) for a in rs)


# the longest row with a direct plan: A (B C | 1) complex numbers of LDS per field, at most 160 KiB and 65535 elements
LONGEST = {8: 20102, 4: 24334}

# precision -> [(row length, (A, B, C, fields per workgroup))]
COVER = {
    8: [(16, (2, 2, 2, 16)), (34, (17, 1, 1, 16)), (36, (2, 3, 3, 16)), (40, (2, 2, 5, 16)), (46, (23, 1, 1, 16)),
        (68, (2, 17, 1, 16)), (108, (3, 3, 6, 16)), (128, (4, 4, 4, 16)), (330, (3, 5, 11, 8)), (648, (6, 6, 9, 4)), (686, (7, 7, 7, 4)),
        (1024, (8, 8, 8, 4)), (1350, (5, 9, 15, 2)), (2000, (10, 10, 10, 2)), (2574, (9, 11, 13, 1)), (3168, (11, 12, 12, 1)),
        (4732, (13, 13, 14, 1)), (6272, (14, 14, 16, 1)), (7650, (15, 15, 17, 1)), (9728, (16, 16, 19, 1)), (10488, (12, 19, 23, 1)),
        (20102, (19, 23, 23, 1))],
    4: [(16, (2, 2, 2, 16)), (34, (17, 1, 1, 16)), (36, (2, 3, 3, 16)), (38, (19, 1, 1, 16)), (40, (2, 2, 5, 16)),
        (56, (2, 2, 7, 16)), (128, (4, 4, 4, 16)), (144, (2, 6, 6, 16)), (160, (2, 5, 8, 16)), (200, (10, 10, 1, 16)), (440, (11, 20, 1, 16)),
        (462, (11, 21, 1, 16)), (500, (5, 5, 10, 16)), (648, (3, 9, 12, 8)), (650, (5, 5, 13, 8)), (756, (6, 7, 9, 8)), (1326, (3, 13, 17, 4)),
        (2178, (9, 11, 11, 4)), (2304, (8, 8, 18, 4)), (2646, (7, 9, 21, 2)), (4224, (11, 12, 16, 2)), (4500, (10, 15, 15, 2)),
        (5096, (13, 14, 14, 1)), (8512, (14, 16, 19, 1)), (10200, (15, 17, 20, 1)), (10368, (16, 18, 18, 1)), (10488, (12, 19, 23, 1)),
        (24334, (23, 23, 23, 1))],
}


def lengths(precision, upto=None):
    return [n for n, _ in COVER[precision] if upto is None or n <= upto]


def plan_of(precision, n):
    return dict(COVER[precision])[n]


def assert_plan(inq, n, precision):
    """inq: the (ndgl, 5) array of the "fftplan" inquiry of a handle whose rows all have n points"""
    got = {tuple(int(x) for x in row) for row in inq}
    assert got == {(MR_FAMILY,) + tuple(plan_of(precision, n))}, \
        "row length %d, precision %d: expected the direct mixed-radix plan %s, the library selects %s -- retuned mr_choose? Choose the covering list " \
        "again (tests/mr_cover.py)" % (n, precision, plan_of(precision, n), sorted(got))


if __name__ == "__main__":  # choose the lists again, on the emulator library: python -m tests.mr_cover (two minutes)
    import os
    import ectrans_amd
    ectrans_amd._use_library_for_tests(os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libectrans_mi_emu.so"))
    ectrans_amd.setup_trans0(kmax_resol=4)
    for prec in (8, 4):
        tab = enumerate_plans(ectrans_amd, prec, range(4, ENUM_MAX + 1, 2))
        print(prec, "direct plans up to %d:" % ENUM_MAX, len(tab))
        # (23^3 = 12167 is the longest product of three radices)
        tab.update(enumerate_plans(ectrans_amd, prec, [n for n in range(ENUM_MAX + 2, 24400, 2) if three_radices(n // 2, prec)]))
        LONGEST[prec] = max(tab)
        print(prec, "longest:", LONGEST[prec], greedy({n: p for n, p in tab.items() if n <= ENUM_MAX or n == LONGEST[prec]}, prec))
