"""Seeded inputs of the mutual-NN matching tests (CPU and GPU) on which a
wrong kernel shows, and the decoding of the 64-bit match keys
(include/pcr_math.h pcr_match_key) for assertion messages.

Every builder returns float32 arrays f1 [p, n1, c], f2 [p, n2, c]."""
import numpy as np

# (n1, n2) with every n at an edge of a 32-wide C/D block, of a wave's 64 or
# of a tile's 128: each of 1, 31 .. 33, 63 .. 65, 127 .. 129, 255 .. 257 once per side
TILE_EDGE_PAIRS = [(1, 257), (31, 129), (32, 65), (33, 1), (63, 128), (64, 33), (65, 31),
                   (127, 64), (128, 255), (129, 32), (255, 63), (256, 127), (257, 256)]

# (n1, n2, c, lo, hi): values in lo .. hi - 1; the measured tie shares are in
# tests/test_matching_cpu.py
ALPHABET_SHAPES = [(300, 260, 4, -1, 2), (1100, 200, 6, -2, 3), (130, 2100, 3, -1, 2),
                   (257, 257, 17, -1, 2)]

# duplicated-row index pairs of placed_ties(), b rows (a, b) both equal one a
# row.  As f2 columns: neighbouring lanes, lanes l / l ^ 16, one lane's two
# columns (offset 32), the two waves of a tile row (64), two tiles (128), the
# tile edge; the same again inside the second tile.
COLUMN_TIE_PAIRS = [(3, 4), (10, 26), (5, 37), (50, 114), (60, 188), (127, 128), (135, 136),
                    (150, 166), (193, 225)]
# As f1 rows (C/D layout row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5) + 32 ti +
# 64 wi): consecutive accumulator registers (1), lanes l / l ^ 32 (4),
# register groups (8), the two 32-row halves ti (32), two waves (64), two
# tiles (128), the tile edge.
ROW_TIE_PAIRS = [(2, 3), (9, 13), (17, 25), (6, 38), (20, 84), (100, 228), (127, 128),
                 (130, 131), (137, 141), (145, 153), (134, 166), (148, 212)]


def clustered(n1, n2, c, seed, p=1, nbase=40, noise=1e-4):
    """Rows = one of nbase random centres + noise: best and second-best diff
    lie within a few fp32 ulps of each other, so the argmin depends on the
    order of the channel sums (the share of rows / columns is asserted in
    tests/test_matching_cpu.py), and some diffs come out negative."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((p, nbase, c))

    def rows(n):
        pick = rng.integers(0, nbase, (p, n))
        x = np.take_along_axis(base, pick[:, :, None], axis=1)
        return (x + noise * rng.standard_normal((p, n, c))).astype(np.float32)
    return rows(n1), rows(n2)


def alphabet(n1, n2, c, lo, hi, seed, p=1):
    """Small integers: every product, sum and norm^2 sum is exact in fp32, so
    any summation order gives the same diff bits, and exact ties abound."""
    rng = np.random.default_rng(seed)
    f1 = rng.integers(lo, hi, (p, n1, c)).astype(np.float32)
    f2 = rng.integers(lo, hi, (p, n2, c)).astype(np.float32)
    return f1, f2


def permuted_copy(n1, n2, c, seed, p=1):
    """The smaller side is a permuted subset of the larger side's distinct
    rows: every row of the smaller side has its copy as unique mutual
    partner, so count == min(n1, n2)."""
    rng = np.random.default_rng(seed)
    big, small = max(n1, n2), min(n1, n2)
    x = rng.standard_normal((p, big, c), dtype=np.float32)
    y = np.stack([x[q, rng.permutation(big)[:small]] for q in range(p)])
    return (x, y) if n1 >= n2 else (y, x)


def placed_ties(pairs, n=260, c=8, seed=11):
    """a, b [1, n, c] distinct random rows, except b[lo] = b[hi] = a[7 k + 1]
    for the k-th (lo, hi) of pairs: the two copies give a's row the same diff
    bits (one chain, one norm), ~1e-6, against ~2 c elsewhere, so they are its
    unique minimum and np.argmin takes lo.  -> (a, b, rows [k], los [k])."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((1, n, c), dtype=np.float32)
    b = rng.standard_normal((1, n, c), dtype=np.float32)
    rows = np.array([7 * k + 1 for k in range(len(pairs))])
    for r, (lo, hi) in zip(rows, pairs):
        b[0, lo] = b[0, hi] = a[0, r]
    return a, b, rows, np.array([lo for lo, _ in pairs])


def special_values(seed=3, n1=140, n2=150, c=6):
    """name -> (f1, f2) [1, n, c]; the expected results are written out in
    tests/test_matching_cpu.py::test_special_values_by_hand."""
    rng = np.random.default_rng(seed)
    g1 = rng.standard_normal((1, n1, c), dtype=np.float32)
    g2 = rng.standard_normal((1, n2, c), dtype=np.float32)
    # no exact zeros: the sign of inf * x is then defined everywhere
    assert np.all(g1 != 0) and np.all(g2 != 0)
    out = {}

    def case(name, edit1=None, edit2=None):
        f1, f2 = g1.copy(), g2.copy()
        if edit1:
            edit1(f1[0])
        if edit2:
            edit2(f2[0])
        out[name] = (f1, f2)

    def put(rows, k, v):
        def edit(f):
            for r in rows:
                f[r, k] = v
        return edit

    def fill(v, rows=None):
        def edit(f):
            if rows is None:
                f[:] = v
            else:
                f[rows] = v
        return edit
    case("nan_one_f2", None, put([77], 2, np.nan))
    case("nan_two_f2", None, put([77, 20], 2, np.nan))
    case("nan_one_f1", put([33], 0, np.nan), None)
    case("nan_all", fill(np.nan), fill(np.nan))
    case("inf_f1", put([5], 1, np.inf), None)
    case("inf_f2", None, put([9], 3, np.inf))
    case("overflow_nan", fill(3e19, [7]), fill(3e19, [12]))
    out["overflow_inf"] = (np.full((1, n1, c), 1e19, np.float32), np.zeros((1, 130, c), np.float32))
    out["subnormal"] = (g1 * np.float32(2.0 ** -70), g2 * np.float32(2.0 ** -70))
    return out


def decode_key(key):
    """int64 / uint64 match key -> (diff bits, index): the inverse of
    pcr_match_key's mapping (a NaN diff decodes as 0x7fc00000)."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    u, idx = key >> 32, key & 0xFFFFFFFF
    if u == 0:
        bits = 0x7FC00000
    elif u & 0x80000000:
        bits = u & 0x7FFFFFFF
    else:
        bits = ~u & 0xFFFFFFFF
    return bits, idx


def key_diff(key):
    """the winning diff of a key as a Python float"""
    return float(np.array([decode_key(key)[0]], np.uint32).view(np.float32)[0])


def assert_keys_equal(got, exp, name):
    """np.array_equal on keys [p, n], naming the first differing element with
    both diffs in hex."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (name, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    if len(bad):
        q, i = bad[0]
        (gb, gi), (eb, ei) = decode_key(got[q, i]), decode_key(exp[q, i])
        raise AssertionError(
            "%s: %d of %d keys differ; first at pair %d element %d: got diff 0x%08x (%r) index %d, "
            "expected diff 0x%08x (%r) index %d" % (name, len(bad), got.size, q, i, gb,
                                                    key_diff(got[q, i]), gi, eb,
                                                    key_diff(exp[q, i]), ei))
