"""Restatements of the ragged ops' contracts, on the CPU.

list_normals   pcr_normals_from_neighbors: the nine cumulants in numpy (fp64
               products of the widened coordinates, summed from 0.0 in
               ascending slot, a slot outside [0, n) skipped in place), then
               pcr_estimate_normal of include/pcr_math.h itself through a
               small C program (gcc -O1 -ffp-contract=off), as
               test_fpfh_cpu.py runs include/pcr_fpfh.h.
match / icp / fgr
               the ragged contract is "the dense op on the pair trimmed to its
               counts, plus a fixed fill", so these are the existing
               restatements (oracle.mutual_nn_keys, icp_restate, fgr_restate)
               on the trimmed pair plus the fills.
scan_pair      the synthetic surface scans of the chain test.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "pcr_math.h"
/* stdin: int m, then m records {double cum[9]; int cnt; float p[3]}  ->
 * stdout: m x float[3] */
int main(void) {
  int m, i;
  if (fread(&m, 4, 1, stdin) != 1) return 1;
  for (i = 0; i < m; i++) {
    double cum[9];
    int cnt;
    float p[3], out[3];
    if (fread(cum, 8, 9, stdin) != 9 || fread(&cnt, 4, 1, stdin) != 1 ||
        fread(p, 4, 3, stdin) != 3)
      return 2;
    pcr_estimate_normal(cum, cnt, p[0], p[1], p[2], out);
    fwrite(out, 4, 3, stdout);
  }
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def normal_exe():
    d = tempfile.mkdtemp(prefix="ragged_restate_")
    src = os.path.join(d, "normal_host.c")
    with open(src, "w") as f:
        f.write(PROGRAM)
    out = os.path.join(d, "normal_host")
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-I", INCLUDE, src, "-o", out,
                           "-lm"])
    return out


def cumulants(xyz, idx):
    """xyz [b, 3, n] fp32, idx [b, k, n] int -> cum [b, n, 9] fp64, cnt [b, n]"""
    xyz = np.asarray(xyz, F)
    idx = np.asarray(idx, np.int64)
    b, _, n = xyz.shape
    k = idx.shape[1]
    cum = np.zeros((b, n, 9), np.float64)
    cnt = np.zeros((b, n), np.int32)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for q in range(b):
        p64 = xyz[q].astype(np.float64)
        for s in range(k):
            j = idx[q, s]
            ok = (j >= 0) & (j < n)
            v = p64[:, j[ok]]
            for d in range(3):
                cum[q, ok, d] += v[d]
            for a, (d, e) in enumerate(pairs):
                cum[q, ok, 3 + a] += v[d] * v[e]
            cnt[q, ok] += 1
    return cum, cnt


def list_normals(xyz, idx):
    """-> normals [b, 3, n] fp32, nbr_count [b, n] int32"""
    xyz = np.asarray(xyz, F)
    b, _, n = xyz.shape
    cum, cnt = cumulants(xyz, idx)
    rec = np.zeros(b * n, np.dtype([("cum", "<f8", 9), ("cnt", "<i4"), ("p", "<f4", 3)]))
    rec["cum"] = cum.reshape(-1, 9)
    rec["cnt"] = cnt.reshape(-1)
    rec["p"] = xyz.transpose(0, 2, 1).reshape(-1, 3)
    raw = subprocess.run([normal_exe()], input=np.int32(b * n).tobytes() + rec.tobytes(),
                         stdout=subprocess.PIPE, check=True).stdout
    out = np.frombuffer(raw, F).reshape(b, n, 3).transpose(0, 2, 1)
    return np.ascontiguousarray(out), cnt


def assert_same_bits(got, exp, what=""):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, \
        "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, exp.shape, exp.dtype)
    if got.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        got, exp = got.view(u), exp.view(u)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, "%s: %d of %d differ, first at %s: %r vs %r" % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def valid(counts, q, n):
    return n if counts is None else int(min(max(int(counts[q]), 0), n))


# ------------------------------------------------------------- matching
ONES = np.int64(-1)  # the all-ones key


def match(f1, f2, counts1, counts2, channel_major=False):
    """-> corr12, corr21, idx1, idx2, count, rowbest, colbest of the ragged
    matching: oracle.mutual_nn_keys on each trimmed pair, -1 / all-ones past
    the counts"""
    import oracle
    f1, f2 = np.asarray(f1, F), np.asarray(f2, F)
    if channel_major:
        f1, f2 = f1.transpose(0, 2, 1), f2.transpose(0, 2, 1)
    p, n1, _ = f1.shape
    n2 = f2.shape[1]
    corr12 = np.full((p, n1), -1, np.int32)
    corr21 = np.full((p, n2), -1, np.int32)
    idx1, idx2 = np.full((p, n1), -1, np.int32), np.full((p, n1), -1, np.int32)
    count = np.zeros(p, np.int32)
    rb, cb = np.full((p, n1), ONES, np.int64), np.full((p, n2), ONES, np.int64)
    for q in range(p):
        v1, v2 = valid(counts1, q, n1), valid(counts2, q, n2)
        if v1 == 0 or v2 == 0:
            continue
        g = oracle.mutual_nn_keys(np.ascontiguousarray(f1[q:q + 1, :v1]),
                                  np.ascontiguousarray(f2[q:q + 1, :v2]))
        corr12[q, :v1], corr21[q, :v2] = g[0][0], g[1][0]
        idx1[q, :v1], idx2[q, :v1], count[q] = g[2][0], g[3][0], g[4][0]
        rb[q, :v1], cb[q, :v2] = g[5][0], g[6][0]
    return corr12, corr21, idx1, idx2, count, rb, cb


# ------------------------------------------------------------------ ICP
def icp(xyz1, xyz2, counts1, counts2, init=None, **kw):
    """icp_restate.icp_pair on each trimmed pair; corr -1 past v1; an empty
    source returns the init with status 1; an empty target is the dense rule
    with nothing within reach"""
    import icp_restate as ir
    p, _, n1 = xyz1.shape
    n2 = xyz2.shape[2]
    out = dict(transform=np.zeros((p, 4, 4)), corr=np.full((p, n1), -1, np.int32),
               num_corr=np.zeros(p, np.int32), fitness=np.zeros(p), rmse=np.zeros(p),
               iterations=np.zeros(p, np.int32), status=np.zeros(p, np.int32))
    margin = np.inf
    for q in range(p):
        v1, v2 = valid(counts1, q, n1), valid(counts2, q, n2)
        t0 = np.eye(4) if init is None else np.asarray(init[q], np.float64)
        if v1 == 0:
            tr = np.eye(4)
            tr[:3] = t0[:3]
            out["transform"][q], out["status"][q] = tr, 1
            continue
        if v2 == 0:
            # no target: M = 0 at the first evaluation
            tr = np.eye(4)
            tr[:3] = t0[:3]
            out["transform"][q] = tr
            out["status"][q] = 2 if kw.get("max_iters", 200) == 0 else 1
            continue
        r = ir.icp_pair(xyz1[q][:, :v1], xyz2[q][:, :v2], t0, **kw)
        margin = min(margin, r["conv_margin"])
        out["corr"][q, :v1] = r["corr"]
        for k in ("transform", "num_corr", "fitness", "rmse", "iterations", "status"):
            out[k][q] = r[k]
    out["conv_margin"] = margin
    return out


# ------------------------------------------------------------------ FGR
def fgr(xyz1, xyz2, idx1, idx2, count, counts1, counts2, **kw):
    """fgr_restate.fgr_pair on each trimmed pair (with the pair's own index q,
    which seeds its tuple test)"""
    import fgr_restate as fr
    p, _, n1 = xyz1.shape
    n2 = xyz2.shape[2]
    res = []
    for q in range(p):
        v1, v2 = valid(counts1, q, n1), valid(counts2, q, n2)
        res.append(fr.fgr_pair(xyz1[q][:, :v1], xyz2[q][:, :v2], idx1[q], idx2[q], int(count[q]),
                               q, **kw))
    return res


# ---------------------------------------------------- the chain's fixture
def surface(rng, n):
    """n points of a bumpy height field over [-1, 1]^2, lifted away from the
    origin so that the normals' orientation is unambiguous: [3, n] fp32"""
    u, v = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    z = (0.35 * np.exp(-((u - 0.4) ** 2 + (v + 0.3) ** 2) / 0.08)
         - 0.30 * np.exp(-((u + 0.5) ** 2 + (v - 0.45) ** 2) / 0.05)
         + 0.25 * np.exp(-((u + 0.3) ** 2 + (v + 0.6) ** 2) / 0.03)
         + 0.20 * np.exp(-((u - 0.6) ** 2 + (v - 0.6) ** 2) / 0.02)
         + 0.15 * np.sin(2.3 * u) * np.cos(1.7 * v) + 0.1 * u * v)
    return np.stack([u, v, z + 3.0]).astype(F)


def rotation(rng, degrees):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(degrees)
    kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * kx @ kx


def scan_pair(seed, n1, n2, degrees=25.0, tnorm=0.4):
    """-> scan1 [3, n1], scan2 [3, n2], gt [4, 4]: scan2 is another sampling
    of the same surface (its own points, its own size and order), moved by
    gt and rounded to fp32"""
    rng = np.random.default_rng(seed)
    s1 = surface(rng, n1)
    s2 = surface(rng, n2)
    gt = np.eye(4)
    gt[:3, :3] = rotation(rng, degrees)
    t = rng.normal(size=3)
    gt[:3, 3] = tnorm * t / np.linalg.norm(t)
    s2 = (gt[:3, :3] @ s2.astype(np.float64) + gt[:3, 3:4]).astype(F)
    return s1, s2, gt
