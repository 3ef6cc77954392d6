"""Oracle of the feature-space mutual-NN matching (SURVEY.md 8f row f1,
datasets/deepgmr_mn40.py:232-244) against the reference's own numpy
expression, and known answers.  CPU only.

The reference evaluates diff with numpy float32 (BLAS-order channel sums);
the oracle (and the GPU kernel, bit for bit) uses k-ordered fmaf chains.
Argmins therefore agree except where two candidates are within a few fp32
ulps of diff: such near-ties are excluded from the comparison (parity
unpinned there -- the reference's own result depends on its BLAS).  On the
exact small-integer inputs of tests/match_inputs.py every order gives the
same bits, so there the comparison has no exclusions; the second half of
this file also checks the conditions those inputs must meet (order
sensitivity, tie shares) and the special-value answers derived by hand."""
import numpy as np
import pytest

import oracle
import match_inputs as mi


def numpy_reference(a, b):
    """The reference's expression (deepgmr_mn40.py:235-243), float32."""
    diff = np.power(np.linalg.norm(a, axis=1, keepdims=True), 2) + \
        np.power(np.linalg.norm(b, axis=1, keepdims=True).T, 2) - 2 * np.dot(a, b.T)
    c12 = np.argmin(diff, axis=1)
    c21 = np.argmin(diff, axis=0)
    mask = c21[c12] == np.arange(c12.shape[0])
    return diff, c12, c21, np.arange(c12.shape[0])[mask], c12[mask]


def _clear(diff, axis, tol):
    """Rows (axis=1) / columns (axis=0) whose best and second-best diff differ
    by more than tol (relative to the magnitudes involved)."""
    s = np.sort(diff, axis=axis)
    best, second = np.take(s, 0, axis=axis), np.take(s, 1, axis=axis)
    scale = np.abs(diff).max(axis=axis) + 1e-30
    return (second - best) > tol * scale


@pytest.mark.parametrize("p,n1,n2,c", [(2, 300, 280, 64), (1, 257, 513, 33), (1, 128, 128, 512)])
def test_oracle_matches_numpy_reference(p, n1, n2, c):
    rng = np.random.default_rng(n1 + c)
    f1 = rng.standard_normal((p, n1, c), dtype=np.float32)
    f2 = rng.standard_normal((p, n2, c), dtype=np.float32)
    c12, c21, i1, i2, cnt = oracle.mutual_nn(f1, f2)
    for q in range(p):
        diff, r12, r21, ri1, ri2 = numpy_reference(f1[q], f2[q])
        ok_r = _clear(diff, 1, 1e-5)
        ok_c = _clear(diff, 0, 1e-5)
        assert ok_r.mean() > 0.9 and ok_c.mean() > 0.9
        assert np.array_equal(c12[q][ok_r], r12[ok_r])
        assert np.array_equal(c21[q][ok_c], r21[ok_c])
        if ok_r.all() and ok_c.all():
            assert cnt[q] == len(ri1)
            assert np.array_equal(i1[q, :cnt[q]], ri1) and np.array_equal(i2[q, :cnt[q]], ri2)
        assert np.all(i1[q, cnt[q]:] == -1) and np.all(i2[q, cnt[q]:] == -1)


def test_permuted_features_match_their_permutation():
    """feat2 = feat1 permuted (distinct rows): every point's mutual partner
    is itself, so idx2 = perm^-1[idx1] for all n points."""
    rng = np.random.default_rng(7)
    n, c = 200, 16
    f1 = rng.standard_normal((1, n, c), dtype=np.float32)
    perm = rng.permutation(n)
    f2 = f1[:, perm]
    c12, c21, i1, i2, cnt = oracle.mutual_nn(f1, f2)
    inv = np.argsort(perm)
    assert cnt[0] == n
    assert np.array_equal(i1[0], np.arange(n))
    assert np.array_equal(i2[0], inv)


def test_ties_take_the_first_index_and_nan_first():
    """np.argmin semantics: equal diffs -> the lowest index; a NaN diff wins
    (argmin returns the first NaN)."""
    f1 = np.zeros((1, 2, 2), np.float32)
    f1[0, 0] = [1, 0]
    f1[0, 1] = [0, 1]
    f2 = np.zeros((1, 3, 2), np.float32)
    f2[0, 0] = [0, 1]
    f2[0, 1] = [1, 0]
    f2[0, 2] = [1, 0]  # duplicate of row 1: row 0 of f1 ties between 1 and 2
    c12, c21, i1, i2, cnt = oracle.mutual_nn(f1, f2)
    assert list(c12[0]) == [1, 0]
    assert list(c21[0]) == [1, 0, 0]
    assert cnt[0] == 2 and list(i1[0]) == [0, 1] and list(i2[0]) == [1, 0]
    f2[0, 2] = [np.nan, 0]
    c12, c21, _, _, _ = oracle.mutual_nn(f1, f2)
    assert list(c12[0]) == [2, 2]


# ---- the inputs of tests/match_inputs.py: conditions on the inputs, the
# oracle against numpy with no exclusions, and answers derived by hand

def _hi(keys):
    return (np.asarray(keys).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def _lo(keys):
    return (np.asarray(keys).view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def _one_mutual_pair(i1, i2, cnt, a, b):
    assert cnt[0] == 1 and i1[0, 0] == a and i2[0, 0] == b
    assert np.all(i1[0, 1:] == -1) and np.all(i2[0, 1:] == -1)


def test_decode_key_inverts_the_key_mapping():
    # pcr_match_key by hand: +0 / -0 -> 0x80000000, 1.0 -> 0xBF800000,
    # -1.0 -> ~0xBF800000, +inf -> 0xFF800000, NaN -> 0
    for hi, bits in [(0x80000000, 0), (0xBF800000, 0x3F800000), (0x407FFFFF, 0xBF800000),
                     (0xFF800000, 0x7F800000), (0, 0x7FC00000), (0x7FFFFFFF, 0x80000000)]:
        assert mi.decode_key((hi << 32) | 17) == (bits, 17)
        assert mi.decode_key(np.uint64((hi << 32) | 17).view(np.int64)) == (bits, 17)
    with pytest.raises(AssertionError, match=r"0x3f800000 \(1.0\) index 2, expected diff 0x00000000"):
        mi.assert_keys_equal(np.array([[5, (0xBF800000 << 32) | 2]], np.uint64).view(np.int64),
                             np.array([[5, (0x80000000 << 32) | 1]], np.uint64).view(np.int64), "k")


@pytest.mark.parametrize("p,n1,n2,c", [(2, 300, 280, 64), (1, 1, 5, 3)])
def test_mutual_nn_keys_consistent_with_mutual_nn(p, n1, n2, c):
    rng = np.random.default_rng(n1)
    f1 = rng.standard_normal((p, n1, c), dtype=np.float32)
    f2 = rng.standard_normal((p, n2, c), dtype=np.float32)
    plain = oracle.mutual_nn(f1, f2)
    keyed = oracle.mutual_nn_keys(f1, f2)
    for a, b in zip(plain, keyed[:5]):
        assert np.array_equal(a, b)
    rb, cb = keyed[5], keyed[6]
    assert rb.shape == (p, n1) and cb.shape == (p, n2) and rb.dtype == np.int64
    assert np.array_equal(_lo(rb), plain[0]) and np.array_equal(_lo(cb), plain[1])
    # the winner's diff of row i is the winner's diff of its column when mutual
    for q in range(p):
        i, j = plain[2][q, :plain[4][q]], plain[3][q, :plain[4][q]]
        assert np.array_equal(_hi(rb[q, i]), _hi(cb[q, j]))


@pytest.mark.parametrize("n1,n2,c", [(600, 600, 64), (257, 385, 33)])
def test_clustered_input_is_order_sensitive(n1, n2, c):
    """A condition on the input, not on the oracle: summing the channels in
    numpy's BLAS order instead of the k-ordered chain moves at least 10 % of
    corr12 and of corr21 (measured: 45 % and 47 % at the first shape), and
    some winning diffs are negative (the key mapping's other branch)."""
    f1, f2 = mi.clustered(n1, n2, c, seed=n1 + c)
    c12, c21, _, _, _, rb, cb = oracle.mutual_nn_keys(f1, f2)
    _, r12, r21, _, _ = numpy_reference(f1[0], f2[0])
    s12, s21 = (c12[0] != r12).mean(), (c21[0] != r21).mean()
    print("clustered %dx%dx%d: corr12 moved %.3f corr21 moved %.3f" % (n1, n2, c, s12, s21))
    assert s12 >= 0.10 and s21 >= 0.10
    neg = lambda k: ((_hi(k) != 0) & (_hi(k) < 0x7FFFFFFF)).mean()  # noqa: E731
    print("negative winning diffs: rows %.4f columns %.4f" % (neg(rb), neg(cb)))
    assert neg(rb) > 0 or neg(cb) > 0


@pytest.mark.parametrize("n1,n2,c,lo,hi", mi.ALPHABET_SHAPES)
def test_oracle_equals_numpy_on_exact_alphabet(n1, n2, c, lo, hi):
    """Small integers: exact in any summation order, so the oracle equals the
    reference's numpy expression on every output with no exclusions -- and at
    least 20 % of the rows and of the columns attain their minimum more than
    once (the input must keep producing ties), so this pins np.argmin's
    first-index rule."""
    f1, f2 = mi.alphabet(n1, n2, c, lo, hi, seed=n1 + n2)
    c12, c21, i1, i2, cnt, rb, cb = oracle.mutual_nn_keys(f1, f2)
    for q in range(f1.shape[0]):
        diff, r12, r21, ri1, ri2 = numpy_reference(f1[q], f2[q])
        tr = ((diff == diff.min(axis=1, keepdims=True)).sum(axis=1) > 1).mean()
        tc = ((diff == diff.min(axis=0, keepdims=True)).sum(axis=0) > 1).mean()
        print("alphabet %dx%dx%d: tied rows %.2f tied columns %.2f" % (n1, n2, c, tr, tc))
        assert tr >= 0.20 and tc >= 0.20
        assert np.array_equal(c12[q], r12) and np.array_equal(c21[q], r21)
        assert cnt[q] == len(ri1)
        assert np.array_equal(i1[q, :cnt[q]], ri1) and np.array_equal(i2[q, :cnt[q]], ri2)
        assert np.all(i1[q, cnt[q]:] == -1) and np.all(i2[q, cnt[q]:] == -1)
        # the keys' diff bits are numpy's minima
        rd = np.array([mi.key_diff(k) for k in rb[q]])
        cd = np.array([mi.key_diff(k) for k in cb[q]])
        assert np.array_equal(rd, diff.min(axis=1)) and np.array_equal(cd, diff.min(axis=0))


def test_degenerate_features_by_hand():
    """All diffs equal: every argmin is index 0, one mutual pair (0, 0)."""
    rng = np.random.default_rng(2)
    row = rng.standard_normal(8, dtype=np.float32)
    for v in (np.zeros(8, np.float32), row):
        f1, f2 = np.tile(v, (1, 200, 1)), np.tile(v, (1, 300, 1))
        c12, c21, i1, i2, cnt = oracle.mutual_nn(f1, f2)
        assert np.all(c12 == 0) and np.all(c21 == 0)
        _one_mutual_pair(i1, i2, cnt, 0, 0)


def test_placed_ties_by_hand():
    """Duplicated rows at the strides of the kernel's reductions: the lower
    index wins, for rows (corr12) and, mirrored, for columns (corr21)."""
    a, b, rows, los = mi.placed_ties(mi.COLUMN_TIE_PAIRS)
    c12, c21, _, _, _, rb, _ = oracle.mutual_nn_keys(a, b)
    assert np.array_equal(c12[0, rows], los)
    assert np.array_equal(c21[0, los], rows)
    assert np.all(np.abs([mi.key_diff(k) for k in rb[0, rows]]) < 1e-4)
    a, b, cols, los = mi.placed_ties(mi.ROW_TIE_PAIRS)
    c12, c21, _, _, _ = oracle.mutual_nn(b, a)
    assert np.array_equal(c21[0, cols], los)
    assert np.array_equal(c12[0, los], cols)


def test_signed_zero_ties_take_the_first_index():
    """f2 = f1 on the exact alphabet: a row's diffs against its own copies
    tie at the minimum and the first copy wins.  A diff is never -0: it is
    x - y with x = sq1 + sq2 >= +0, and round-to-nearest gives -0 only from
    (-0) - (+0).  So the -0 -> +0 step of pcr_match_key cannot be reached
    through the matching (it is the key function's own contract)."""
    f1, _ = mi.alphabet(300, 1, 4, -1, 2, seed=9)
    c12, c21, _, _, _, rb, cb = oracle.mutual_nn_keys(f1, f1)
    first = np.array([np.flatnonzero((f1[0] == r).all(axis=1))[0] for r in f1[0]])
    assert (first != np.arange(300)).mean() > 0.5  # most rows have an earlier copy
    assert np.array_equal(c12[0], first) and np.array_equal(c21[0], first)
    _, r12, r21, _, _ = numpy_reference(f1[0], f1[0])
    assert np.array_equal(c12[0], r12) and np.array_equal(c21[0], r21)
    assert not np.any(_hi(rb) == 0x7FFFFFFF) and not np.any(_hi(cb) == 0x7FFFFFFF)


def test_special_values_by_hand():
    cases = mi.special_values()
    g1, g2 = cases["nan_one_f2"][0], cases["nan_one_f1"][1]  # the unedited sides
    b12, b21, _, _, _ = oracle.mutual_nn(g1, g2)
    n1, n2 = g1.shape[1], g2.shape[1]
    r1, r2 = np.arange(n1), np.arange(n2)

    # a NaN feature makes its whole row / column of diffs NaN: argmin takes
    # the first NaN
    c12, c21, i1, i2, cnt = oracle.mutual_nn(*cases["nan_one_f2"])
    assert np.all(c12 == 77) and c21[0, 77] == 0
    assert np.array_equal(c21[0, r2 != 77], b21[0, r2 != 77])
    _one_mutual_pair(i1, i2, cnt, 0, 77)
    c12, c21, i1, i2, cnt = oracle.mutual_nn(*cases["nan_two_f2"])
    assert np.all(c12 == 20) and c21[0, 77] == 0 and c21[0, 20] == 0
    _one_mutual_pair(i1, i2, cnt, 0, 20)
    c12, c21, i1, i2, cnt = oracle.mutual_nn(*cases["nan_one_f1"])
    assert np.all(c21 == 33) and c12[0, 33] == 0
    assert np.array_equal(c12[0, r1 != 33], b12[0, r1 != 33])
    _one_mutual_pair(i1, i2, cnt, 33, 0)
    c12, c21, i1, i2, cnt = oracle.mutual_nn(*cases["nan_all"])
    assert np.all(c12 == 0) and np.all(c21 == 0)
    _one_mutual_pair(i1, i2, cnt, 0, 0)

    # f1[5, 1] = +inf: |f1_5|^2 = inf and the dot is +inf where f2[j, 1] > 0
    # (diff = inf - inf = NaN) and -inf where < 0 (diff = +inf)
    c12, c21, _, _, _ = oracle.mutual_nn(*cases["inf_f1"])
    pos = g2[0, :, 1] > 0
    assert c12[0, 5] == np.flatnonzero(pos)[0]
    assert np.all(c21[0, pos] == 5) and np.all(c21[0, ~pos] != 5)
    assert np.array_equal(c12[0, r1 != 5], b12[0, r1 != 5])
    c12, c21, _, _, _ = oracle.mutual_nn(*cases["inf_f2"])
    pos = g1[0, :, 3] > 0
    assert c21[0, 9] == np.flatnonzero(pos)[0]
    assert np.all(c12[0, pos] == 9) and np.all(c12[0, ~pos] != 9)
    assert np.array_equal(c21[0, r2 != 9], b21[0, r2 != 9])

    # 3e19 squared overflows: |f|^2 = +inf on row 7 and column 12, their dot
    # is +inf too: diff[7, 12] = NaN, the rest of row 7 and column 12 = +inf
    c12, c21, i1, i2, cnt, rb, cb = oracle.mutual_nn_keys(*cases["overflow_nan"])
    assert c12[0, 7] == 12 and c21[0, 12] == 7
    assert _hi(rb)[0, 7] == 0 and _hi(cb)[0, 12] == 0
    assert 7 in i1[0, :cnt[0]] and i2[0, list(i1[0]).index(7)] == 12
    keep = (r1 != 7) & (b12[0] != 12)
    assert np.array_equal(c12[0, keep], b12[0, keep]) and np.all(c12[0, r1 != 7] != 12)
    keep = (r2 != 12) & (b21[0] != 7)
    assert np.array_equal(c21[0, keep], b21[0, keep]) and np.all(c21[0, r2 != 12] != 7)

    # 1e19 rows against zeros: every diff is +inf (key 0xFF800000), index 0
    # wins (a device sentinel above every key must stay above this one)
    c12, c21, i1, i2, cnt, rb, cb = oracle.mutual_nn_keys(*cases["overflow_inf"])
    assert np.all(c12 == 0) and np.all(c21 == 0)
    assert np.all(_hi(rb) == 0xFF800000) and np.all(_hi(cb) == 0xFF800000)
    _one_mutual_pair(i1, i2, cnt, 0, 0)

    # 2^-70 features: products and channel sums are subnormal (a condition on
    # the input: every winning diff is subnormal or zero, not all are zero;
    # flushing any of them to zero would change these keys)
    f1, f2 = cases["subnormal"]
    _, _, _, _, _, rb, cb = oracle.mutual_nn_keys(f1, f2)
    d = np.abs(np.array([mi.key_diff(k) for k in np.concatenate([rb[0], cb[0]])]))
    assert np.all(d < np.finfo(np.float32).tiny) and (d > 0).mean() > 0.5
