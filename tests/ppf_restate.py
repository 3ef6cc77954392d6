"""Float64 restatement of the point-pair features, the comparison helper and
the input families of the PPF tests (test_ppf_cpu.py, test_gpu_ppf.py).

The two references below are plain numpy float64 written from the model's
definition (pvcnn_classify.py:252-269 and spherical_ppf/ppf.cu:28-90); they
share no code with include/pcr_math.h or oracle/np_restate.py.  They return
cosines, not angles: acos is ill-conditioned at +-1, so the kernels' angles are
compared as cos(angle).
"""
import functools

import numpy as np

import oracle
from clouds import edge_clouds_for_knn, gaussian_clouds

COS_TOL = 2e-6   # tests/test_oracle_kat.py: |cos(angle) - cos_f64|
DN_RTOL = 1e-6   # tests/test_oracle_kat.py: |d|, relative
REL1_EXCLUDED_CAP = 0.005


# ------------------------------------------------------------ references
def local_ppf_f64(points, normals, centers, cnormals, idx, kmajor, relative):
    """-> [b, 4, u, m] float64: clamp(pn . d/|d|), clamp(cn . d/|d|),
    clamp(pn . cn), |d| with d = 2c - p when `relative`, else c - p.  Indices
    < 0 or >= n read neighbour 0.  Undefined elements (0 / 0, NaN inputs) are
    NaN."""
    P, Pn, C, Cn = (np.asarray(a, dtype=np.float64) for a in (points, normals, centers, cnormals))
    ids = np.asarray(idx).astype(np.int64)
    if not kmajor:
        ids = ids.transpose(0, 2, 1)  # [b, u, m]
    n = P.shape[2]
    ids = np.where((ids < 0) | (ids >= n), 0, ids)
    out = np.empty((P.shape[0], 4) + ids.shape[1:], np.float64)
    with np.errstate(all="ignore"):
        for b in range(P.shape[0]):
            p, pn = P[b][:, ids[b]], Pn[b][:, ids[b]]  # [3, u, m]
            c, cn = C[b][:, None, :], Cn[b][:, None, :]
            d = 2.0 * c - p if relative else c - p
            dn = np.sqrt((d * d).sum(axis=0))
            u = d / dn
            out[b, 0] = np.clip((pn * u).sum(axis=0), -1.0, 1.0)
            out[b, 1] = np.clip((cn * u).sum(axis=0), -1.0, 1.0)
            out[b, 2] = np.clip((pn * cn).sum(axis=0), -1.0, 1.0)
            out[b, 3] = dn
    return out


def global_ppf_f64(coords, center, normals, cnormals):
    """-> (ref [b, 4, n] float64, zero_row [b, n]): clamp(d^ . cn^),
    clamp(d^ . n^), clamp(cn^ . n^), max(|d|, 1e-20) with d = centre - point,
    d^ = d / max(|d|, 1e-20) and each normal divided by its length.  A row
    with either normal of length <= 1e-10 is the zero row (flagged; its ref
    entries are 0).  ppf.cu clamps with max(min(x, 1), -1), and CUDA's min /
    max return the other operand of a NaN: an undefined cosine reads as 1
    (angle 0) and an undefined |d| as 1e-20, so this reference is defined
    everywhere."""

    def clamp(x):
        return np.fmax(np.fmin(x, 1.0), -1.0)

    X, C, Nn, Cn = (np.asarray(a, dtype=np.float64) for a in (coords, center, normals, cnormals))
    with np.errstate(all="ignore"):
        d = C - X
        dn = np.fmax(np.sqrt((d * d).sum(axis=1)), 1e-20)  # a NaN length clamps too
        d = d / dn[:, None]
        l1 = np.sqrt((Cn * Cn).sum(axis=1))
        l2 = np.sqrt((Nn * Nn).sum(axis=1))
        zero = (l1 <= 1e-10) | (l2 <= 1e-10)
        cn, nn = Cn / l1[:, None], Nn / l2[:, None]
        ref = np.stack([clamp((d * cn).sum(axis=1)), clamp((d * nn).sum(axis=1)),
                        clamp((cn * nn).sum(axis=1)), dn], axis=1)
    ref[np.broadcast_to(zero[:, None, :], ref.shape)] = 0.0
    return ref, zero


# ------------------------------------------------------------ comparison
def unit_rows(nrm):
    """[b, n]: the normal is finite and of unit length (to fp32 rounding)."""
    v = np.asarray(nrm, dtype=np.float64)
    with np.errstate(all="ignore"):
        ln = np.sqrt((v * v).sum(axis=1))
    return np.isfinite(v).all(axis=1) & (np.abs(ln - 1.0) <= 1e-6)


# fp32 cannot hold every |d|^2 of the scaled clouds, and there the oracle
# itself (fp32 by definition) leaves the bounds: a square below 2^-126 is
# denormal, so each of the three roundings of x*x + y*y + z*z may be off by
# 2^-150 absolute instead of 2^-24 relative.  |d| then carries up to
# 1.5 * 2^-150 / |d|^2 + 2.5 * 2^-24 relative: 5.1e-7 at |d| = 2^-64, inside
# the 1e-6 bound, and 1.6e-6 at 2^-65, outside it.  At the top the sum of
# squares must stay below fp32's largest number, just under 2^128.  Pairs
# whose float64 |d| lies outside [DN_LO, DN_HI) are "out of range": they are
# still compared bit for bit with the oracle, not with float64, and their
# share is returned, capped (range_cap) and asserted like the undefined share.
DN_LO, DN_HI = 2.0 ** -64, 2.0 ** 64 * (1.0 - 2.0 ** -23)


def compare_local(out, ref, p_unit, c_unit, idx, kmajor):
    """Kernel / oracle local PPF `out` [b, 4, u, m] against local_ppf_f64's
    `ref`.  An element is excluded where the reference is undefined (NaN), and
    there `out` must be NaN too; a pair is out of range where fp32 cannot hold
    |d|^2 (above).  The bounds apply to every other element whose normals are
    unit and finite (p_unit [b, n], c_unit [b, m]).  -> dict, per cloud:
    `excluded` and `out_of_range` pair shares, `eligible` [b, 4] elements with
    unit normals, `bounded` [b, 4] elements held to the bounds; and the worst
    errors `cos`, `dn`."""
    out = np.asarray(out)
    assert out.shape == ref.shape and out.dtype == np.float32
    undef = np.isnan(ref)
    assert np.isnan(out[undef]).all(), "finite output where float64 is undefined"
    ids = np.asarray(idx).astype(np.int64)
    if not kmajor:
        ids = ids.transpose(0, 2, 1)
    n = p_unit.shape[1]
    ids = np.where((ids < 0) | (ids >= n), 0, ids)
    pu = np.stack([p_unit[b][ids[b]] for b in range(ids.shape[0])])  # [b, u, m]
    cu = np.broadcast_to(c_unit[:, None, :], pu.shape)
    dn = ref[:, 3]
    with np.errstate(invalid="ignore"):
        ranged = (dn >= DN_LO) & (dn < DN_HI)
        off_range = ~ranged & (dn > 0)  # |d| = 0 or NaN is undefined, not out of range
    assert (out[:, 3][dn == 0] == 0).all(), "|d| = 0 in float64 but not in the output"
    ones = np.ones_like(pu)
    elig = np.stack([pu, cu, pu & cu, ones], axis=1)
    use = elig & np.stack([ranged, ranged, ones, ranged], axis=1) & ~undef
    assert not np.isnan(out[use]).any(), "NaN output where float64 is defined"
    with np.errstate(all="ignore"):
        cerr = np.abs(np.cos(out[:, :3].astype(np.float64)) - ref[:, :3])
        derr = np.abs(out[:, 3].astype(np.float64) - dn) / dn
    cmax = float(cerr[use[:, :3]].max()) if use[:, :3].any() else 0.0
    dmax = float(derr[use[:, 3]].max()) if use[:, 3].any() else 0.0
    assert cmax <= COS_TOL, "cosine off by %.3g" % cmax
    assert dmax <= DN_RTOL, "|d| off by %.3g relative" % dmax
    return {"excluded": undef.any(axis=1).mean(axis=(1, 2)),
            "out_of_range": off_range.mean(axis=(1, 2)),
            "eligible": elig.sum(axis=(2, 3)), "bounded": use.sum(axis=(2, 3)),
            "pairs": pu[0].size, "cos": cmax, "dn": dmax}


def assert_coverage(fig, excluded_cap, range_cap):
    """The caps hold per cloud, and every channel of every cloud keeps its
    eligible elements under the bounds, less at most the capped shares."""
    assert (fig["excluded"] <= excluded_cap + 1e-12).all(), "excluded share %s above cap %s" % (
        fig["excluded"], excluded_cap)
    assert (fig["out_of_range"] <= range_cap + 1e-12).all(), (
        "out-of-range share %s above cap %s" % (fig["out_of_range"], range_cap))
    lost = (np.asarray(excluded_cap) + range_cap) * fig["pairs"]
    need = fig["eligible"] - np.broadcast_to(lost, fig["eligible"].shape[:1])[:, None]
    assert (fig["bounded"] >= need).all(), "bounded %s of eligible %s" % (
        fig["bounded"].tolist(), fig["eligible"].tolist())


def compare_global(out, ref, zero):
    """Kernel / oracle global PPF `out` [b, 4, n] against global_ppf_f64: a
    flagged row must be the all-zero row, an undefined element NaN, the rest
    within the bounds.  -> (max cosine error, max relative |d| error, number
    of bounded elements)."""
    out = np.asarray(out)
    assert out.shape == ref.shape and out.dtype == np.float32
    zr = np.broadcast_to(zero[:, None, :], out.shape)
    assert (out[zr] == 0).all(), "a row with a ~0 normal is not the zero row"
    undef = np.isnan(ref)
    assert np.isnan(out[undef]).all(), "finite output where float64 is undefined"
    use = ~undef & ~zr
    assert not np.isnan(out[use]).any(), "NaN output where float64 is defined"
    with np.errstate(all="ignore"):
        cerr = np.abs(np.cos(out[:, :3].astype(np.float64)) - ref[:, :3])
        derr = np.abs(out[:, 3].astype(np.float64) - ref[:, 3]) / ref[:, 3]
    cmax = float(cerr[use[:, :3]].max()) if use[:, :3].any() else 0.0
    dmax = float(derr[use[:, 3]].max()) if use[:, 3].any() else 0.0
    assert cmax <= COS_TOL, "cosine off by %.3g" % cmax
    assert dmax <= DN_RTOL, "|d| off by %.3g relative" % dmax
    return cmax, dmax, int(use.sum())


def excluded_cap(xyz, nrm, ids, unfilled, relative):
    """Per cloud, a cap on the share of pairs the float64 reference leaves
    undefined, from the inputs alone.  relative = 1: 0.005 for the inputs of
    these tests (d = 2c - p vanishes on lattices only).  relative = 0:
    d = c - p vanishes for the self pair and for every neighbour that
    duplicates the centre, at most min(k, copies) slots per point -- 1 / k
    plus the cloud's duplicate-pair share; plus the unfilled slots (`unfilled`
    [b, k, n], they read point 0) of the copies of point 0; plus the pairs
    whose centre or neighbour has a non-finite coordinate or normal."""
    xyz, nrm = np.asarray(xyz), np.asarray(nrm)
    b, k, n = ids.shape
    if relative:
        return np.full(b, REL1_EXCLUDED_CAP)
    cap = np.zeros(b)
    for i in range(b):
        pts = xyz[i].T
        _, inv, cnt = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
        copies = np.minimum(k, cnt[inv.ravel()])
        like0 = (pts == pts[0]).all(axis=1)
        bad = ~(np.isfinite(xyz[i]).all(axis=0) & np.isfinite(nrm[i]).all(axis=0))
        nb = np.where((ids[i] < 0) | (ids[i] >= n), 0, ids[i])
        touched = bad[None, :] | bad[nb]
        cap[i] = (copies.sum() + unfilled[i][:, like0].sum() + touched.sum()) / (k * n)
    return cap


def range_cap(name, n, k):
    """Cap on a cloud's share of out-of-range pairs (DN_LO, DN_HI), from the
    inputs' construction.  Gaussian clouds times 2^e, e <= -59: |d| < 2^-64
    needs another point (the neighbour p, or 2c - p of it) within r =
    2^(-64 - e) of a point; a unit Gaussian cloud of n points has on average
    n (4 pi)^-3/2 points per unit volume around one of its own, so
    n (4 pi)^-3/2 (4/3) pi r^3 such pairs per point are expected, of k: three
    times that, plus 16 pairs for the small counts.  Every other case: 0 --
    the lattices' nonzero |d| is at least their pitch, 2^-63 or more, and
    |d| >= 2^64 at 2^60 needs |2c - p| >= 16 in a unit Gaussian cloud."""
    if name[0] != "A":
        return 0.0
    e = int(name.rsplit("e", 1)[1])
    if e > -59:
        return 0.0
    r = 2.0 ** (-64 - e)
    return 3.0 * n * (4 * np.pi) ** -1.5 * (4.0 / 3.0) * np.pi * r ** 3 / k + 16.0 / (n * k)


def unsafe_pairs(xyz, idx, relative):
    """[b, k, n] bool: the pair leaves the shared-reciprocal path of
    ppf_local_dev -- a nonzero component of d, or |d|, outside [2^-60, 2^60]
    (non-finite included), d in fp32 as the kernel forms it."""
    xyz = np.asarray(xyz, dtype=np.float32)
    n = xyz.shape[2]
    ids = np.where((idx < 0) | (idx >= n), 0, idx)
    lo, hi = np.float32(2.0 ** -60), np.float32(2.0 ** 60)
    bad = np.zeros(ids.shape, bool)
    with np.errstate(all="ignore"):
        for b in range(xyz.shape[0]):
            c = xyz[b][:, None, :]
            p = xyz[b][:, ids[b]]
            d = c - (p - c) if relative else c - p
            a = np.abs(d)
            comp = ((a != 0) & ~((a >= lo) & (a <= hi))).any(axis=0)
            dn = np.sqrt((d.astype(np.float64) ** 2).sum(axis=0)).astype(np.float32)
            bad[b] = comp | ~((dn >= lo) & (dn <= hi))
    return bad


# --------------------------------------------------- sorted-path input cases
# (pcr_knn_prepare + pcr_knn_select_ppf).  Every case is (xyz, normals, k);
# expected ids / PPF come from the oracle, once per process.
SCALES = (-61, -60, -59, 58, 59, 60)
K = 32


def _pow2(e):
    return np.float32(2.0 ** e)


def family_a(n, e):
    """Gaussian clouds times 2^e (exact), unit normals."""
    xyz, nrm, _ = gaussian_clouds(2, n, seed=n + 100 + e)
    return np.ascontiguousarray(xyz * _pow2(e)), nrm, K


def family_b(e):
    """Lattice clouds times 2^e: coordinates are multiples of 2^(e-2), so the
    components of d land on, just inside and just outside 2^-60, with exact
    zeros and p == 2c."""
    xyz = edge_clouds_for_knn(2, 516, seed=5) * _pow2(e)
    return np.ascontiguousarray(xyz), gaussian_clouds(2, 516, seed=55)[1], K


def family_c():
    """Gaussian clouds at scale 1 whose first 64 points are a 4 x 4 x 4
    lattice of pitch 2^-62: the cluster's 32 nearest neighbours are each other
    (d in multiples of 2^-62, mostly outside the range), every other query is
    deep inside it, in one launch."""
    xyz, nrm, _ = gaussian_clouds(2, 1024, seed=64)
    g = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij")).reshape(3, 64)
    for b in range(2):
        xyz[b, :, :64] = g[:, np.random.default_rng(b).permutation(64)] * 2.0 ** -62
    return np.ascontiguousarray(xyz.astype(np.float32)), nrm, K


PLANT = {"zero": slice(100, 104), "nan": 110, "inf": 111, "tiny": slice(120, 124),
         "huge": slice(124, 128), "seam": slice(200, 232)}
SEAM_COS = (1.0, -1.0, 0.5, -0.5)  # eight points each, in this order


def family_normals(n, relative):
    """Three Gaussian clouds: unit normals; unit normals with planted rows
    (PLANT); np.roll normals.  The seam rows take the unit d of the point's
    slot-1 neighbour (float64, rounded): +d, -d and d mixed with an orthogonal
    unit vector to a float64 cosine of exactly 0.5, then -0.5, so slot 1's
    centre-normal cosine sits at +-1 and at the acos seam."""
    xyz, nrm, _ = gaussian_clouds(3, n, seed=n + 7)
    nrm[1, :, PLANT["zero"]] = 0.0
    nrm[1, 0, PLANT["nan"]] = np.nan
    nrm[1, 2, PLANT["inf"]] = np.inf
    nrm[1, :, PLANT["tiny"]] *= np.float32(1e-20)
    nrm[1, :, PLANT["huge"]] *= np.float32(1e20)
    _, ids = oracle.knn_dir(xyz[1:2], xyz[1:2], 2)
    s = PLANT["seam"]
    for t, i in enumerate(range(s.start, s.stop)):
        c = xyz[1, :, i].astype(np.float64)
        p = xyz[1, :, ids[0, 1, i]].astype(np.float64)
        d = 2.0 * c - p if relative else c - p
        d /= np.linalg.norm(d)
        o = np.cross(d, np.eye(3)[np.argmin(np.abs(d))])
        o /= np.linalg.norm(o)
        cs = SEAM_COS[t // 8]
        nrm[1, :, i] = cs * d + np.sqrt(1.0 - cs * cs) * o
    nrm[2] = np.roll(xyz[2], 1, axis=0)
    return xyz, np.ascontiguousarray(nrm), K


SIZES = (4, 5, 512, 513, 516, 1020, 1028, 2045, 2048)


def family_size(b, n, k):
    xyz, nrm, _ = gaussian_clouds(b, n, seed=3 * n + k)
    return xyz, nrm, k


def _sorted_cases():
    cases = {}
    for e in (0,) + SCALES:
        for n in (1024, 1023):
            cases["A-n%d-e%d" % (n, e)] = functools.partial(family_a, n, e)
        cases["B-e%d" % e] = functools.partial(family_b, e)
    cases["C"] = family_c
    for n in SIZES:
        for k in (32, 31):
            cases["size-n%d-k%d" % (n, k)] = functools.partial(family_size, 2, n, k)
    cases["size-b3-n516-k7"] = functools.partial(family_size, 3, 516, 7)
    for n in (1024, 516):
        cases["align-n%d" % n] = functools.partial(family_size, 2, n, 32)
    return cases


SORTED_CASES = _sorted_cases()
SCALE_CASES = [c for c in SORTED_CASES if c[0] in "ABC"]
SIZE_CASES = [c for c in SORTED_CASES if c.startswith("size-")]
NORMAL_SIZES = (1024, 1001)


@functools.lru_cache(maxsize=None)
def sorted_case(name, relative=1):
    """-> (xyz, normals, k, oracle ids, oracle PPF), read-only."""
    if name.startswith("normals-n"):
        xyz, nrm, k = family_normals(int(name[9:]), relative)
    else:
        xyz, nrm, k = SORTED_CASES[name]()
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    nrm = np.ascontiguousarray(nrm, dtype=np.float32)
    _, ids = oracle.knn_dir(xyz, xyz, k)
    ppf = oracle.local_ppf(xyz, nrm, xyz, nrm, ids, kmajor=True, relative=bool(relative))
    for a in (xyz, nrm, ids, ppf):
        a.setflags(write=False)
    return xyz, nrm, k, ids, ppf


@functools.lru_cache(maxsize=None)
def sorted_unfilled(name, relative=1):
    """[b, k, n] bool: the oracle's KNN left the slot unfilled (10000, 0)."""
    xyz, _, k, _, _ = sorted_case(name, relative)
    d, _ = oracle.knn_dir(xyz, xyz, k)
    return d >= 10000


def check_sorted_case_f64(name, relative, out=None):
    """The case's oracle PPF (or `out`, a kernel's) against float64; asserts
    the caps on the undefined and the out-of-range share and the coverage of
    every channel of every cloud.  -> compare_local's figures."""
    xyz, nrm, k, ids, ppf = sorted_case(name, relative)
    ref = local_ppf_f64(xyz, nrm, xyz, nrm, ids, True, relative)
    u = unit_rows(nrm)
    fig = compare_local(ppf if out is None else out, ref, u, u, ids, True)
    fig["excluded_cap"] = excluded_cap(xyz, nrm, ids, sorted_unfilled(name, relative), relative)
    fig["range_cap"] = range_cap(name, xyz.shape[2], k)
    assert_coverage(fig, fig["excluded_cap"], fig["range_cap"])
    return fig


# ------------------------------------------------ explicit-index input cases
LOCAL_SHAPES = ((300, 300, 13), (2048, 2048, 9), (2049, 2049, 8), (700, 257, 20), (257, 700, 20))


@functools.lru_cache(maxsize=None)
def local_case(n, m, u, kmajor):
    """-> (points, normals, centres, centre normals, idx): Gaussian clouds
    (the centres are the points when n == m), idx from the oracle's KNN, or
    its ball query for (257, 700), in the asked layout, with out-of-range ids
    planted at the head, one centre's whole row at -1 and the last centre's
    last slot at n."""
    pts, nrm, _ = gaussian_clouds(2, n, seed=n + u)
    if n == m:
        ctr, cnrm = pts, nrm
    else:
        ctr, cnrm, _ = gaussian_clouds(2, m, seed=m + u + 1)
    if (n, m) == (257, 700):
        ids = oracle.ball_query(ctr, pts, 0.6, u).transpose(0, 2, 1)  # [b, u, m]
    else:
        _, ids = oracle.knn_dir(ctr, pts, u)
    ids = np.array(ids, dtype=np.int32)
    bad = (-1, n, n + 5, 2 ** 31 - 1, -2 ** 31)
    for b in range(2):
        ids[b, 0, :5] = bad
        ids[b, u - 1, 5:10] = bad[::-1]
        ids[b, :, 7 + 100 * b] = -1
        ids[b, u - 1, m - 1] = n
    if not kmajor:
        ids = ids.transpose(0, 2, 1)
    ids = np.ascontiguousarray(ids)
    for a in (pts, nrm, ctr, cnrm, ids):
        a.setflags(write=False)
    return pts, nrm, ctr, cnrm, ids


@functools.lru_cache(maxsize=None)
def local_expected(n, m, u, kmajor, relative):
    pts, nrm, ctr, cnrm, ids = local_case(n, m, u, kmajor)
    out = oracle.local_ppf(pts, nrm, ctr, cnrm, ids, kmajor=kmajor, relative=bool(relative))
    out.setflags(write=False)
    return out


GLOBAL_SIZES = (1, 255, 257, 1000)
G_PLANT = ("n_below", "n_above", "cn_below", "cn_above", "coincide", "near", "nan_xyz", "nan_nrm",
           "short", "long")


def _unit(rng, b, n):
    v = rng.standard_normal((b, 3, n))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def global_case(n):
    """-> (coords, centre, normals, centre normals, oracle output, planted
    columns): Gaussian points against per-point Gaussian centres, unit
    normals, with planted columns (n = 1 is one plain pair per cloud): normal
    lengths 0.9e-10 / 1.1e-10 on either side of the zero-row threshold for
    each of the two normals, a point on its centre and one 1e-30 from it
    (under the 1e-20 clamp), a NaN coordinate, a NaN normal, normals of length
    1e-5 and 1e5."""
    rng = np.random.default_rng(n + 11)
    xyz = rng.standard_normal((3, 3, n)).astype(np.float32)
    ctr = rng.standard_normal((3, 3, n)).astype(np.float32)
    nrm, cnrm = _unit(rng, 3, n), _unit(rng, 3, n)
    if n == 1:
        return xyz, ctr, nrm, cnrm, oracle.spherical_ppf_forward(xyz, ctr, nrm, cnrm), {}
    col = {name: 17 * i + 3 for i, name in enumerate(G_PLANT)}  # all below 255
    nrm[:, :, col["n_below"]] *= np.float32(0.9e-10)
    nrm[:, :, col["n_above"]] *= np.float32(1.1e-10)
    cnrm[:, :, col["cn_below"]] *= np.float32(0.9e-10)
    cnrm[:, :, col["cn_above"]] *= np.float32(1.1e-10)
    ctr[:, :, col["coincide"]] = xyz[:, :, col["coincide"]]
    ctr[:, :, col["near"]] = 0.0
    xyz[:, :, col["near"]] = (1e-30, 0.0, 0.0)
    xyz[:, 1, col["nan_xyz"]] = np.nan
    cnrm[:, 2, col["nan_nrm"]] = np.nan
    nrm[:, :, col["short"]] *= np.float32(1e-5)
    cnrm[:, :, col["long"]] *= np.float32(1e5)
    out = oracle.spherical_ppf_forward(xyz, ctr, nrm, cnrm)
    for a in (xyz, ctr, nrm, cnrm, out):
        a.setflags(write=False)
    return xyz, ctr, nrm, cnrm, out, col
