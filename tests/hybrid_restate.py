"""The hybrid (radius + max_nn) neighbour search's contract (include/pcr_hybrid.h,
DESIGN.md 4.8g) restated in numpy as brute force over all pairs: np.float32,
the fmaf of oracle/np_restate.py, a lexsort on (bits of d, j).  It knows
nothing of cells.  Also the inputs the CPU and the GPU tests share."""
import numpy as np

from oracle.np_restate import fmaf

F = np.float32
INF_BITS = 0x7F800000


# ---------------------------------------------------------------- contract
def pair_dist(p):
    """[3, m] -> d [m, m], d[i, j] = fmaf(tz, tz, fmaf(ty, ty, tx * tx)) with
    t = p_i - p_j"""
    with np.errstate(all="ignore"):
        t = (p[:, :, None] - p[:, None, :]).astype(F)
        return fmaf(t[2], t[2], fmaf(t[1], t[1], (t[0] * t[0]).astype(F)))


def search_cloud(xyz, radius, k, count=None):
    """One cloud [3, n] -> dist [k, n], idx [k, n], nbr_count [n], within [n]"""
    xyz = np.asarray(xyz, F)
    n = xyz.shape[1]
    m = n if count is None else min(max(int(count), 0), n)
    r2 = F(radius) * F(radius)
    dist = np.full((k, n), np.inf, F)
    idx = np.full((k, n), -1, np.int32)
    cnt, within = np.zeros(n, np.int32), np.zeros(n, np.int32)
    if m == 0:
        return dist, idx, cnt, within
    d = pair_dist(xyz[:, :m])
    with np.errstate(all="ignore"):
        inr = d <= r2  # a NaN fails; r2 is finite, so an infinite d fails
    for i in range(m):
        j = np.nonzero(inr[i])[0]
        row = d[i, j]
        order = np.lexsort((j, row.view(np.uint32)))[:k]
        within[i] = len(j)
        cnt[i] = len(order)
        dist[:len(order), i] = row[order]
        idx[:len(order), i] = j[order]
    return dist, idx, cnt, within


def search(xyz, radius, k, counts=None):
    """[b, 3, n] -> dist [b, k, n], idx [b, k, n], nbr_count [b, n], within
    [b, n]"""
    xyz = np.asarray(xyz, F)
    per = [search_cloud(xyz[q], radius, k, None if counts is None else counts[q])
           for q in range(xyz.shape[0])]
    return tuple(np.stack([p[a] for p in per]) for a in range(4))


_cache = {}


def expected(name, k):
    """the restatement of case `name` at k, computed once"""
    key = (name, k)
    if key not in _cache:
        xyz, radius, _, counts = cases()[name]
        _cache[key] = search(xyz, radius, k, counts)
    return _cache[key]


def assert_same_bits(got, exp, what=""):
    g = np.ascontiguousarray(got)
    e = np.ascontiguousarray(exp)
    assert g.shape == e.shape and g.dtype == e.dtype, (what, g.shape, e.shape, g.dtype, e.dtype)
    if g.dtype == F:
        g, e = g.view(np.uint32), e.view(np.uint32)
    bad = np.argwhere(g != e)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def assert_same(got, exp, what=""):
    for g, e, name in zip(got, exp, ("dist", "idx", "nbr_count", "within")):
        if g is not None:
            assert_same_bits(g, e, (what, name))


def wave_cap():
    """PCR_HYBRID_WAVE_CAP of include/pcr_hybrid.h: the in-radius keys a wave of
    the query kernel buffers"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = open(os.path.join(root, "include", "pcr_hybrid.h")).read()
    return int(re.search(r"#define\s+PCR_HYBRID_WAVE_CAP\s+(\d+)", head).group(1))


def assert_reaches(name):
    """On the restatement, never on the code under test: the input `name`
    reaches the branch it is there for"""
    xyz, radius, ks, counts = cases()[name]
    res = {k: expected(name, k) for k in ks}
    dist, idx, cnt, within = res[ks[-1]]
    n = xyz.shape[2]
    if name.startswith("size_"):
        assert xyz.shape[0] == 3 and ks == (1, 7, 128)
        assert (cnt >= 1).all() and (res[1][2] == 1).all()
        assert (res[1][1][:, 0] == np.arange(n)).all()  # the nearest is the point itself
        if n > 2:
            assert within.max() > 7  # k = 7 cuts
        if n < 128:
            assert (cnt == within).all() and cnt.max() <= n  # k > n: nothing is cut
    elif name == "both":
        assert ks == (16,) and n == 300
        assert (within < 16).any() and (within == 16).any() and (within > 16).any()
    elif name == "overflow":
        assert n == 1500 and n > wave_cap()
        for k in (128, 5):
            assert (res[k][3] == n).all() and (res[k][2] == k).all()
    elif name == "lattice":
        # interior points have 7 within the radius, six of them at d == r2
        # exactly; k = 4 cuts inside the tie and the lower indices win
        p = 1 + 6 * (1 + 6 * 1)
        dist, idx, cnt, within = res[16]
        assert within[0, p] == 7 and within[0, 0] == 4 and within[0].max() == 7
        assert (dist[0, 1:7, p] == F(0.0625)).all() and dist[0, 0, p] == 0
        assert idx[0, :7, p].tolist() == [p, p - 36, p - 6, p - 1, p + 1, p + 6, p + 36]
        assert res[4][1][0, :, p].tolist() == [p, p - 36, p - 6, p - 1]
        assert res[4][2][0, p] == 4 and res[4][3][0, p] == 7
    elif name == "lattice_inside":
        assert within[0, 1 + 6 * (1 + 6 * 1)] == 7
    elif name == "lattice_outside":
        # one ulp wider: the corner's neighbours, at the spacing itself, fall
        # outside (further along, i * spacing rounds some gaps back to the radius)
        assert within[0, 0] == 1 and within[0, 1] == 1 and within[0, 6] == 1 and within[0, 36] == 1
    elif name == "lattice_shifted":
        assert 2 <= within.max() <= 7
    elif name == "tiny_radius":
        assert (cnt == 1).all() and (within == 1).all()
        assert np.ptp(xyz[0], axis=1).min() > 32 * 1000 * radius  # extent far above G * radius
    elif name == "far_from_origin":
        assert xyz.min() >= 1.0e6 and within.max() > 1
    elif name == "duplicates":
        # a copy with index >= 128 lists copies 0 .. 127, not itself
        same = (xyz[0][:, :, None] == xyz[0][:, None, :]).all(axis=0).sum(axis=1)
        dup = np.nonzero(same == 200)[0]  # the copies, in index order
        assert len(dup) == 200 and (within[0, dup] >= 200).all()
        late = dup[128:]
        assert late.min() >= 128
        for i in late:
            assert idx[0, :, i].tolist() == dup[:128].tolist() and i not in idx[0, :, i]
            assert not dist[0, :, i].any()
    elif name.startswith("ragged"):
        # rows at or past the count are empty, no row names a padded index
        assert counts.tolist() == [130, 0, 1, 77] and n == 130
        for q, m in enumerate(counts):
            assert (idx[q, :, m:] == -1).all() and not cnt[q, m:].any() and not within[q, m:].any()
            assert idx[q].max() < m or m == 0
            assert m == 0 or cnt[q, :m].min() >= 1
        other = expected("ragged_copies" if name == "ragged_nan" else "ragged_nan", ks[-1])
        assert np.array_equal(idx, other[1])  # the padding's content changes nothing
    elif name == "non_finite":
        for bad in (17, 40, 63):
            assert cnt[0, bad] == 0 and not (idx[0] == bad).any()
        assert np.median(cnt[0]) >= 4
    elif name == "huge":
        # a huge finite point is valid: within the radius of itself alone
        assert cnt[0, 5] == 1 and cnt[0, 50] == 1 and cnt[0, 77] == 1 and cnt[0, 78] == 1
        assert np.median(cnt[0]) >= 4
    else:
        raise AssertionError("no branch stated for %s" % name)


# ------------------------------------------------------------------ inputs
def cube(rng, n, scale=1.0, shift=0.0):
    return (rng.uniform(0.0, scale, (3, n)) + shift).astype(F)


def lattice(spacing, shift=(0.0, 0.0, 0.0), side=6):
    """side^3 points, index = x + side * (y + side * z), coordinate = (fp32)
    i * spacing + shift, every operation in fp32"""
    i = np.arange(side, dtype=F)
    g = np.stack(np.meshgrid(i, i, i, indexing="ij"), axis=0).reshape(3, -1)[::-1]
    s = np.asarray(shift, F)[:, None]
    return ((g * F(spacing)).astype(F) + s).astype(F)


_cases = None


def cases():
    """name -> (xyz [b, 3, n], radius, ks, counts or None)"""
    global _cases
    if _cases is not None:
        return _cases
    c = {}
    # sizes: three different clouds per batch, k = 1, a middle one, 128 (> n up to 65)
    for n in (1, 2, 63, 65, 129):
        rng = np.random.default_rng(100 + n)
        xyz = np.stack([cube(rng, n), cube(rng, n, 2.0, -3.0), cube(rng, n, 0.5, 7.0)])
        c["size_%d" % n] = (xyz, 0.45, (1, 7, 128), None)
    # both selection branches in one cloud: a sparse cube and a dense cluster
    rng = np.random.default_rng(7)
    xyz = np.concatenate([cube(rng, 150), (0.5 + 0.05 * rng.standard_normal((3, 150))).astype(F)],
                         axis=1)
    c["both"] = (xyz[None], 0.07, (16,), None)
    # more within the radius than a wave buffers: one cell, everybody a neighbour
    c["overflow"] = (cube(np.random.default_rng(8), 1500)[None], 2.0, (128, 5), None)
    # cell edges and ties: neighbours at d == r2 exactly, just inside, just outside
    r = F(0.25)
    c["lattice"] = (lattice(r)[None], r, (4, 16), None)
    c["lattice_shifted"] = (lattice(r, (-3.3, 17.1, 0.7))[None], r, (4, 16), None)
    c["lattice_inside"] = (lattice(r * (F(1) - F(2.0 ** -23)))[None], r, (4, 16), None)
    c["lattice_outside"] = (lattice(r * (F(1) + F(2.0 ** -23)))[None], r, (4, 16), None)
    # sparse and fine
    c["tiny_radius"] = (cube(np.random.default_rng(9), 200, 100.0, -50.0)[None], 1e-4, (8,), None)
    c["far_from_origin"] = (cube(np.random.default_rng(10), 200, 4.0, 1.0e6)[None], 0.5, (16,),
                            None)
    # duplicates: 200 copies of one point, then 100 others
    rng = np.random.default_rng(11)
    xyz = cube(rng, 300)
    xyz[:, :200] = xyz[:, :1]
    xyz = xyz[:, rng.permutation(300)]
    c["duplicates"] = (xyz[None], 0.3, (128,), None)
    # ragged: padding of NaN, and of copies of valid points
    rng = np.random.default_rng(12)
    counts = np.array([130, 0, 1, 77], np.int32)
    xyz = np.stack([cube(rng, 130) for _ in range(4)])
    nan_pad, copy_pad = xyz.copy(), xyz.copy()
    for q, m in enumerate(counts):
        nan_pad[q, :, m:] = np.nan
        if m:
            copy_pad[q, :, m:] = xyz[q][:, np.arange(130 - m) % m]
    c["ragged_nan"] = (nan_pad, 0.3, (16,), counts)
    c["ragged_copies"] = (copy_pad, 0.3, (16,), counts)
    # non-finite and huge coordinates among valid points
    rng = np.random.default_rng(13)
    xyz = cube(rng, 100)
    xyz[1, 17] = np.nan
    xyz[:, 40] = np.inf
    xyz[0, 63] = -np.inf
    c["non_finite"] = (xyz[None], 0.3, (16,), None)
    xyz = cube(rng, 100)
    xyz[:, 5] = 3e38
    xyz[:, 50] = -3e38
    xyz[0, 77] = 3e38
    xyz[2, 78] = -3e38
    c["huge"] = (xyz[None], 0.3, (16,), None)
    _cases = c
    return c
