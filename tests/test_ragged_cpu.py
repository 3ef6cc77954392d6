"""CPU: the ragged ops' contracts without a GPU -- the list
normals' restatement (tests/ragged_restate.py) on known answers and against
the radius-search oracle, the ragged restatements of the matching, ICP and
FGR, and the argument checks of the new C entry points through the ABI."""
import os
import re

import numpy as np
import pytest

import hybrid_restate as hr
import ragged_restate as rr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pcr_normals_from_neighbors", "pcr_mutual_nn_match_ragged",
         "pcr_icp_point_to_point_ragged", "pcr_fgr_ragged")


# ------------------------------------------------- list normals: known answers
def lattice_patch(z=2.0, side=7, spacing=0.1):
    g = (np.arange(side) - side // 2) * spacing
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(side * side, z)]).astype(F)[None]


@pytest.mark.parametrize("z", [2.0, -2.0])
def test_planar_lattice_gives_the_axis_facing_the_origin(z):
    xyz = lattice_patch(z)
    _, idx, cnt, _ = hr.search(xyz, 0.25, 32)
    nrm, got_cnt = rr.list_normals(xyz, idx)
    assert np.array_equal(got_cnt, cnt) and cnt.min() >= 3
    exp = np.zeros_like(nrm)
    exp[:, 2] = -np.sign(z)  # towards the origin
    assert np.array_equal(nrm, exp)  # exactly the axis (a flipped zero is -0.0)


def test_short_and_empty_rows():
    xyz = lattice_patch()
    n = xyz.shape[2]
    idx = np.full((1, 4, n), -1, np.int32)
    idx[0, 0, 0], idx[0, 1, 0] = 0, 1  # a row of 2
    nrm, cnt = rr.list_normals(xyz, idx)
    assert cnt[0, 0] == 2 and (cnt[0, 1:] == 0).all()
    exp = np.zeros_like(nrm)
    exp[:, 2] = 1.0
    rr.assert_same_bits(nrm, exp, "(0, 0, 1) below three neighbours")


def test_bad_slots_are_skipped_in_place():
    """-1 and an index >= n between valid slots change nothing: the same
    cumulants, bit for bit, as the row without them"""
    rng = np.random.default_rng(5)
    xyz = (rng.normal(size=(1, 3, 40)) + np.array([0, 0, 4.0])[None, :, None]).astype(F)
    n = xyz.shape[2]
    clean = np.stack([rng.permutation(n)[:6] for _ in range(n)], axis=1)[None].astype(np.int32)
    salted = np.full((1, 10, n), -1, np.int32)
    salted[0, [0, 2, 3, 6, 8, 9]] = clean[0]
    salted[0, 1], salted[0, 4], salted[0, 5] = -1, n, 2 ** 31 - 1
    salted[0, 7] = -2 ** 31
    a, ca = rr.list_normals(xyz, clean)
    b, cb = rr.list_normals(xyz, salted)
    assert np.array_equal(ca, cb) and (ca == 6).all()
    rr.assert_same_bits(rr.cumulants(xyz, salted)[0], rr.cumulants(xyz, clean)[0], "cumulants")
    rr.assert_same_bits(b, a, "normals")


# measured on this fixture: the largest angle between the two is 0 rad -- the
# two fp64 summation orders differ below what the rounding of the unit normal
# to float keeps, on every one of the 800 points; the bound is 10 x that
ORACLE_ANGLE_BOUND = 0.0


def test_list_normals_against_the_radius_oracle():
    """every point's row holds all the points within the radius (within <= k)
    and none sits near the boundary, so the neighbour sets are those of
    oracle.estimate_normals; the two sum in different orders: compare angles"""
    import oracle
    rng = np.random.default_rng(17)
    xyz = (rng.uniform(-0.5, 0.5, size=(2, 3, 400)) + np.array([0, 0, 3.0])[None, :, None])
    xyz = xyz.astype(F)
    radius, k = 0.22, 128
    dist, idx, cnt, within = hr.search(xyz, radius, k)
    assert within.max() <= k
    r2 = float(F(radius) * F(radius))
    assert np.abs(dist[np.isfinite(dist)].astype(np.float64) - r2).min() > 1e-6 * r2
    onrm, ocnt = oracle.estimate_normals(xyz, float(F(radius)))
    nrm, got_cnt = rr.list_normals(xyz, idx)
    assert np.array_equal(got_cnt, ocnt) and np.array_equal(got_cnt, cnt)
    assert (cnt >= 3).mean() > 0.9
    a, b = nrm.astype(np.float64), onrm.astype(np.float64)
    cross = np.linalg.norm(np.cross(a, b, axis=1), axis=1)
    angle = np.arctan2(cross, (a * b).sum(axis=1))
    print("largest angle to the oracle: %.3g rad" % angle.max())
    assert angle.max() <= ORACLE_ANGLE_BOUND


# ----------------------------------------------- the ragged restatements
def test_ragged_matching_restatement_is_the_trimmed_pair_plus_fills():
    import oracle
    rng = np.random.default_rng(3)
    f1 = rng.normal(size=(3, 20, 5)).astype(F)
    f2 = rng.normal(size=(3, 17, 5)).astype(F)
    full = rr.match(f1, f2, None, None)
    for g, e in zip(full, oracle.mutual_nn_keys(f1, f2)):
        rr.assert_same_bits(g, e, "full counts")
    c1, c2 = np.array([20, 7, 0], np.int32), np.array([17, 1, 9], np.int32)
    f1n = f1.copy()
    f1n[1, 7:] = np.nan
    got = rr.match(f1n, f2, c1, c2)
    assert (got[0][1, 7:] == -1).all() and (got[0][1, :7] == 0).all()
    assert (got[1][1, 1:] == -1).all() and 0 <= got[1][1, 0] < 7
    assert (got[0][2] == -1).all() and (got[1][2] == -1).all() and got[4][2] == 0
    assert (got[5][1, 7:] == -1).all() and (got[6][2] == -1).all()
    cm = rr.match(f1n.transpose(0, 2, 1), f2.transpose(0, 2, 1), c1, c2, channel_major=True)
    for g, e in zip(cm, got):
        rr.assert_same_bits(g, e, "channel-major")


def test_ragged_icp_restatement_rules():
    import icp_restate as ir
    x1, x2, _ = ir.make_batch(7, 3, 40, 50)
    c1, c2 = np.array([40, 0, 25], np.int32), np.array([50, 30, 0], np.int32)
    x1p = x1.copy()
    x1p[2, :, 25:] = np.nan
    init = np.stack([np.eye(4)] * 3)
    init[1, :3, 3] = (0.1, 0.2, 0.3)
    got = rr.icp(x1p, x2, c1, c2, init, max_iters=20)
    exp0 = ir.icp_pair(x1[0], x2[0], init[0], max_iters=20)
    rr.assert_same_bits(got["transform"][0], exp0["transform"], "full pair")
    assert np.array_equal(got["transform"][1], init[1]) and got["status"][1] == 1
    assert got["iterations"][1] == 0 and got["fitness"][1] == 0 and got["num_corr"][1] == 0
    assert (got["corr"][1] == -1).all() and (got["corr"][2] == -1).all()
    assert got["status"][2] == 1 and got["num_corr"][2] == 0


def test_ragged_fgr_restatement_ignores_the_pads():
    import fgr_restate as fr
    x1, x2, idx1, idx2, count = fr.make_batch(9, 2, 60, 60)[:5]
    c1, c2 = np.array([60, 60], np.int32), np.array([60, 60], np.int32)
    full = rr.fgr(x1, x2, idx1, idx2, count, c1, c2, max_tuples=0)
    # the same clouds inside wider, zero-padded strides
    w1 = np.zeros((2, 3, 90), F)
    w2 = np.zeros((2, 3, 75), F)
    w1[:, :, :60], w2[:, :, :60] = x1, x2
    i1 = np.full((2, 90), -1, np.int32)
    i2 = np.full((2, 90), -1, np.int32)
    i1[:, :60], i2[:, :60] = idx1, idx2
    wide = rr.fgr(w1, w2, i1, i2, count, c1, c2, max_tuples=0)
    for a, b in zip(full, wide):
        rr.assert_same_bits(a["transform"], b["transform"], "fgr transform")
        assert a["status"] == b["status"] == 0


# ------------------------------------------------------------------- ABI
def test_header_library_and_signatures_have_the_entry_points():
    from pcr_amd import _lib
    text = open(os.path.join(ROOT, "include", "pcr_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text)
        assert hasattr(_lib.load(), name)
        assert name in _lib.SIGNATURES
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"normals_nbr_kernel" in data and b"RaggedCounts" in data


ONE = 0x1000  # a dummy pointer: the calls below are refused before any use


def test_normals_argument_checks_need_no_gpu():
    from pcr_amd import _lib
    lib = _lib.load()

    def call(b=2, n=100, k=16, xyz=ONE, idx=ONE, out=ONE, cnt=ONE):
        return lib.pcr_normals_from_neighbors(xyz, idx, b, n, k, out, cnt, None)
    assert call(b=-1) == -1 and call(n=0) == -1 and call(n=-1) == -1
    assert call(k=0) == -1 and call(k=129) == -1
    assert b"k (" in lib.pcr_last_error()
    assert call(b=1 << 12, n=1 << 13, k=64) == -1  # b * k * n reaches 2^31
    assert call(b=0) == 0 and call(b=0, k=0) == -1
    for key in ("xyz", "idx", "out"):
        assert call(**{key: None}) == -1, key
    assert b"null" in lib.pcr_last_error()


def test_matching_argument_checks_need_no_gpu():
    from pcr_amd import _lib
    lib = _lib.load()
    names = ("f1", "f2", "corr12", "corr21", "idx1", "idx2", "count", "ws")

    def call(p=2, n1=100, n2=90, c=8, cm=0, ws_bytes=1 << 30, counts1=ONE, counts2=ONE, **kw):
        a = dict({key: ONE for key in names}, **kw)
        return lib.pcr_mutual_nn_match_ragged(
            a["f1"], a["f2"], p, n1, n2, c, counts1, counts2, cm, a["corr12"], a["corr21"],
            a["idx1"], a["idx2"], a["count"], a["ws"], ws_bytes, None)
    assert call(p=-1) == -1 and call(n1=0) == -1 and call(n2=0) == -1 and call(c=0) == -1
    assert call(p=65536) == -1
    assert call(p=0) == 0 and call(p=0, cm=1) == 0 and call(p=0, n1=0) == -1
    for key in names:
        assert call(**{key: None}) == -1, key
    need = lib.pcr_mutual_nn_workspace_size(2, 100, 90)
    assert call(ws_bytes=need - 1) == -1
    assert b"workspace" in lib.pcr_last_error() and b"ragged" in lib.pcr_last_error()


def test_icp_argument_checks_need_no_gpu():
    from pcr_amd import _lib
    lib = _lib.load()
    names = ("xyz1", "xyz2", "transform", "corr", "num_corr", "fitness", "rmse", "iterations",
             "status")

    def call(p=2, n1=100, n2=90, max_dist=0.2, max_iters=10, rf=1e-6, rr_=1e-6, **kw):
        a = dict({key: ONE for key in names}, **kw)
        return lib.pcr_icp_point_to_point_ragged(
            a["xyz1"], a["xyz2"], p, n1, n2, ONE, ONE, None, max_dist, max_iters, rf, rr_,
            a["transform"], a["corr"], a["num_corr"], a["fitness"], a["rmse"], a["iterations"],
            a["status"], None)
    assert call(p=-1) == -1 and call(n1=0) == -1 and call(n2=0) == -1
    assert call(max_dist=0.0) == -1 and call(max_iters=-1) == -1 and call(max_iters=100001) == -1
    assert call(rf=-1.0) == -1 and call(rr_=float("nan")) == -1
    assert call(p=0) == 0 and call(p=0, n1=0) == -1
    for key in names:
        assert call(**{key: None}) == -1, key
    assert b"null" in lib.pcr_last_error()


def test_fgr_argument_checks_need_no_gpu():
    from pcr_amd import _lib
    lib = _lib.load()
    names = ("xyz1", "xyz2", "idx1", "idx2", "count", "transform", "slots", "num_corr",
             "num_trials", "mu", "status", "ws")

    def call(p=2, n1=100, n2=90, dist=0.08, iters=64, div=1.4, scale=0.95, max_tuples=100,
             trials=100, ws_bytes=1 << 30, **kw):
        a = dict({key: ONE for key in names}, **kw)
        return lib.pcr_fgr_ragged(
            a["xyz1"], a["xyz2"], p, n1, n2, ONE, ONE, a["idx1"], a["idx2"], a["count"], dist,
            iters, div, 1, scale, max_tuples, trials, 0, 0, a["transform"], a["slots"],
            a["num_corr"], a["num_trials"], a["mu"], a["status"], a["ws"], ws_bytes, None)
    assert call(p=-1) == -1 and call(n1=0) == -1 and call(n2=0) == -1
    assert call(iters=-1) == -1 and call(div=1.0) == -1 and call(scale=1.0) == -1
    assert call(max_tuples=-1) == -1 and call(trials=-1) == -1 and call(dist=-1.0) == -1
    assert call(p=0) == 0 and call(p=0, n1=0) == -1
    for key in names:
        assert call(**{key: None}) == -1, key
    need = lib.pcr_fgr_workspace_size(2, 100, 100)
    assert call(ws_bytes=need - 1) == -1
    assert b"workspace" in lib.pcr_last_error()


def test_wrappers_reject_bad_counts_and_cpu_tensors():
    import torch
    from pcr_amd import ops, registration
    x = torch.zeros((2, 3, 16))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.normals_from_neighbors(x, torch.zeros((2, 4, 16), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.estimate_normals_hybrid(x, 0.1)
    with pytest.raises(RuntimeError, match="search='grid'"):
        registration.fpfh_pairs(x, x, x, x, 0.1, counts1=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="equal, non-zero"):
        registration.scan_pairs([], [], 0.1)
