"""Numpy restatement of the grid subsampling contract (include/pcr_gridsub.h,
DESIGN.md 4.8e), written from the reference's text
(cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:24-31,
53-56, 87-94; cpp_utils/cloud/cloud.h:120-123) with np.float32 scalars: every
operation rounds to fp32 on its own, the sums are sequential loops that start
at 0.0 (np.sum is pairwise and would not do), cells come in ascending key.
Also the clouds the CPU and GPU tests share."""
import numpy as np

F = np.float32
MAX_DIM = 1 << 20
SAT_DIM = 1 << 30


def _bound(v, low):
    """min (low) or max of v; a zero result is -0.0 for the minimum when any
    -0.0 is present, +0.0 for the maximum when any +0.0 is (pcr_gridsub_ord)"""
    r = v.min() if low else v.max()
    if r == 0:
        zeros = v[v == 0]
        neg = np.signbit(zeros)
        r = F(-0.0) if (low and neg.any()) else F(0.0) if (low or (~neg).any()) else F(-0.0)
    return F(r)


def cellf(p, origin, dl):
    """max(0, floorf((p - origin) / dl)) in fp32 (p: scalar or array)"""
    with np.errstate(all="ignore"):
        q = np.floor((np.asarray(p, F) - F(origin)) / F(dl))
    return np.where(q > 0, q, F(0.0)).astype(F)


def grid(mn, mx, dl):
    """origin [3], dims [3], status (0 or 3)"""
    dl = F(dl)
    origin, dims, status = np.zeros(3, F), np.zeros(3, np.int32), 0
    with np.errstate(all="ignore"):
        inv = F(1.0) / dl
        for d in range(3):
            origin[d] = F(np.floor(F(mn[d]) * inv)) * dl
            q = cellf(mx[d], origin[d], dl)
            dims[d] = (int(q) if q < F(SAT_DIM) else SAT_DIM) + 1
            if not np.isfinite(origin[d]) or dims[d] > MAX_DIM:
                status = 3
    return origin, dims, status


def grid_subsample(xyz, cell, features=None, count=None):
    """One cloud: xyz [3, n] float32, features [c, n] or None, count: the
    first `count` points are valid (None: n) -> the dict of
    ops.grid_subsample for that cloud (numpy, full size, zero / -1 padded)."""
    xyz = np.asarray(xyz, F)
    n = xyz.shape[1]
    c = 0 if features is None else features.shape[0]
    dl = F(cell)
    out = dict(xyz=np.zeros((3, n), F), features=None if features is None else np.zeros((c, n), F),
               count=0, cell_of=np.full(n, -1, np.int32), cell_count=np.zeros(n, np.int32),
               origin=np.zeros(3, F), dims=np.zeros(3, np.int32), status=0)
    m = n if count is None else int(count)
    if m < 1 or m > n:
        out["status"] = 1
        return out
    pts = xyz[:, :m]
    if not np.isfinite(pts).all():
        out["status"] = 2
        return out
    mn = [_bound(pts[d], True) for d in range(3)]
    mx = [_bound(pts[d], False) for d in range(3)]
    out["origin"], out["dims"], out["status"] = grid(mn, mx, dl)
    if out["status"]:
        return out
    nx, ny = int(out["dims"][0]), int(out["dims"][1])
    idx = [cellf(pts[d], out["origin"][d], dl).astype(np.int64) for d in range(3)]
    keys = [int(idx[0][i]) + nx * (int(idx[1][i]) + ny * int(idx[2][i])) for i in range(m)]
    slot_of_key = {k: s for s, k in enumerate(sorted(set(keys)))}
    cells = len(slot_of_key)
    rows = pts if features is None else np.concatenate([pts, np.asarray(features, F)[:, :m]])
    acc = np.zeros((3 + c, cells), F)  # +0.0
    cnt = np.zeros(cells, np.int32)
    for i in range(m):  # ascending point index
        s = slot_of_key[keys[i]]
        acc[:, s] = acc[:, s] + rows[:, i]
        cnt[s] += 1
        out["cell_of"][i] = s
    for s in range(cells):
        out["xyz"][:, s] = acc[:3, s] * F(1.0 / float(cnt[s]))
        if c:
            out["features"][:, s] = acc[3:, s] / F(cnt[s])
    out["count"] = cells
    out["cell_count"][:cells] = cnt
    return out


def grid_subsample_batch(xyz, cell, features=None, counts=None):
    """[b, 3, n] -> the batched dict (stacked per-cloud results)"""
    b = xyz.shape[0]
    per = [grid_subsample(xyz[q], cell, None if features is None else features[q],
                          None if counts is None else counts[q]) for q in range(b)]
    out = {}
    for k in per[0]:
        out[k] = None if per[0][k] is None else np.stack([np.asarray(p[k]) for p in per])
    out["count"] = out["count"].astype(np.int32)
    out["status"] = out["status"].astype(np.int32)
    return out


# ------------------------------------------------------------------ clouds
def random_cloud(rng, n, c=0, spread=1.0, shift=0.0):
    xyz = (rng.standard_normal((3, n)) * spread + shift).astype(F)
    feat = rng.standard_normal((c, n)).astype(F) if c else None
    return xyz, feat


def edge_clouds():
    """name -> (xyz [3, n], features or None, cell): the occupancy and
    coordinate edge cases both test files pin"""
    rng = np.random.default_rng(99)
    out = {}
    # all points in one cell (n = 70 and n = 1500): a cube well inside a cell
    for n in (70, 1500):
        xyz = (0.5 + 0.2 * rng.random((3, n))).astype(F)
        out["one_cell_%d" % n] = (xyz, rng.standard_normal((3, n)).astype(F), 1.0)
    # every point in its own cell: a 7 x 6 x 5 lattice of cell centres, shuffled
    g = np.stack(np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij"))
    lat = ((g.reshape(3, -1) + 0.5) * 0.25).astype(F)[:, rng.permutation(210)]
    out["own_cell"] = (lat, rng.standard_normal((2, 210)).astype(F), 0.25)
    # duplicated points: 40 distinct points, each repeated 1 .. 9 times, shuffled
    base, _ = random_cloud(rng, 40)
    dup = np.repeat(base, rng.integers(1, 10, 40), axis=1)
    dup = dup[:, rng.permutation(dup.shape[1])]
    out["duplicates"] = (dup, rng.standard_normal((1, dup.shape[1])).astype(F), 0.3)
    # negative coordinates only
    neg, nf = random_cloud(rng, 300, 3, 0.5, -7.0)
    out["negative"] = (neg, nf, 0.2)
    # points on cell faces: multiples of the cell size, both signs (dl = 0.25
    # is exact; dl = 0.1 is not, the faces then fall where the fp32 ops put them)
    k = rng.integers(-6, 7, (3, 200))
    out["faces_exact"] = ((k * 0.25).astype(F), None, 0.25)
    out["faces_tenth"] = ((k.astype(F) * F(0.1)).astype(F), rng.standard_normal((1, 200)).astype(F),
                          0.1)
    # origin rounds above min: index -1 before the clamp
    clamp = np.array([[4.7, 4.75, 4.85, 5.3], [4.7, 4.7, 4.7, 4.7], [0.0, 0.05, 0.0, 0.3]], F)
    out["clamp"] = (clamp, np.array([[1.0, 2.0, 3.0, 4.0]], F), 0.1)
    # signed zeros: a lone -0.0 coordinate sums to +0.0
    zer = np.array([[-0.0, 0.0, -0.0, 1.0], [-0.0, -0.0, -0.0, -0.0], [0.0, 0.0, 0.0, 0.0]], F)
    out["zeros"] = (zer, np.array([[-0.0, -0.0, -0.0, -0.0]], F), 0.5)
    # two clusters 500 apart at dl = 0.001: keys past 2^32 (57 key bits)
    far = (rng.random((3, 400)) * 0.01).astype(F)
    far[:, 200:] += F(500.0)
    out["keys64"] = (far[:, rng.permutation(400)], rng.standard_normal((1, 400)).astype(F), 0.001)
    # cells of 1 .. 73 points: the sum takes batches of 32, then of 8, then
    # single points (73 = 2 x 32 + 8 + 1)
    sizes = [8, 9, 32, 33, 64, 1, 7, 31, 40, 41, 73]
    cells = np.repeat(np.arange(len(sizes)), sizes)
    xyz = np.stack([cells + 0.1 + 0.8 * rng.random(cells.size), 0.5 * np.ones(cells.size),
                    0.5 * np.ones(cells.size)]).astype(F)
    perm = rng.permutation(cells.size)
    out["batches"] = (xyz[:, perm], rng.standard_normal((2, cells.size)).astype(F), 1.0)
    return out


def assert_same(got, exp, what=""):
    """exact equality, bit for bit, of every output (floats compared as their
    bit patterns: -0.0 is not +0.0)"""
    for k in ("status", "count", "dims", "cell_of", "cell_count"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(exp[k])), (what, k)
    for k in ("origin", "xyz", "features"):
        if exp[k] is None:
            assert got[k] is None, (what, k)
            continue
        g = np.ascontiguousarray(got[k], F).view(np.uint32)
        e = np.ascontiguousarray(exp[k], F).view(np.uint32)
        assert g.shape == e.shape, (what, k)
        bad = np.argwhere(g != e)
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist())
