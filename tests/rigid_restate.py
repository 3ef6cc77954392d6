"""numpy / fp64 restatement of the rigid-transform estimation contract
(the kernel is csrc/rigid.hip, its scalar math
include/pcr_rigid.h).  Deliberately another algorithm where the contract
allows one: the least-squares solve is the SVD Kabsch, the kernel's is Horn's
quaternion method; residuals are evaluated in fp64 from the fp32-rounded
transform, the kernel's in an fp32 fmaf chain.  The integer sampler and the
fp64 edge-length check are restated operation for operation.  Everything
consumes the fp32-rounded inputs the GPU gets."""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """uint32 mixer on python ints or uint64 arrays holding uint32 values"""
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & U32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & U32
    x = x ^ (x >> np.uint64(16))
    return x


def draw(seed, q, h, j):
    h = np.asarray(h, dtype=np.uint64)
    s = mix(np.uint64(seed) ^ np.uint64(0x9E3779B9))
    s = mix((s + np.uint64(q)) & U32)
    return mix((s + np.uint64(3) * h + np.uint64(j)) & U32)


def triples(seed, q, h, m):
    """[len(h), 3] distinct slots of [0, m)"""
    h = np.atleast_1d(np.asarray(h, dtype=np.uint64))
    a = (draw(seed, q, h, 0) % np.uint64(m)).astype(np.int64)
    b = (draw(seed, q, h, 1) % np.uint64(m - 1)).astype(np.int64)
    c = (draw(seed, q, h, 2) % np.uint64(m - 2)).astype(np.int64)
    b = b + (b >= a)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    c = c + (c >= lo)
    c = c + (c >= hi)
    return np.stack((a, b, c), axis=1)


def kabsch(a, b):
    """least-squares R, t with b ~ R a + t, det R = +1; a, b [m, 3] fp64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    hm = (a - ca).T @ (b - cb)
    u, _, vt = np.linalg.svd(hm)
    d = 1.0 if np.linalg.det(vt.T @ u.T) >= 0 else -1.0
    r = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    return r, cb - r @ ca


def cov_singular_values(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.svd((a - a.mean(axis=0)).T @ (b - b.mean(axis=0)), compute_uv=False)


def edge_ok(a, b, rho):
    """a, b [..., 3, 3] ([slot][xyz]) fp32 -> bool [...]; fp64, in the header's
    operation order"""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    r = np.float64(np.float32(rho))
    ok = np.ones(a.shape[:-2], dtype=bool)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        da, db = a[..., i, :] - a[..., j, :], b[..., i, :] - b[..., j, :]
        la = np.sqrt(da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1] + da[..., 2] * da[..., 2])
        lb = np.sqrt(db[..., 0] * db[..., 0] + db[..., 1] * db[..., 1] + db[..., 2] * db[..., 2])
        ok &= (la > 0) & (lb > 0) & ~(la < r * lb) & ~(lb < r * la)
    return ok


def residuals(r, t, a, b):
    """|R32 a + t32 - b| in fp64 with R, t rounded to fp32; a, b [m, 3]"""
    r32 = np.asarray(r).astype(np.float32).astype(np.float64)
    t32 = np.asarray(t).astype(np.float32).astype(np.float64)
    return np.linalg.norm(a @ r32.T + t32 - b, axis=1)


def tau_of(inlier_dist):
    """the threshold on the residual: sqrt of the fp32 product tau * tau"""
    t = np.float32(inlier_dist)
    return float(np.sqrt(np.float64(t * t)))


def ransac_pair(xyz1, xyz2, idx1, idx2, m, q, hyps, inlier_dist, edge_ratio, refine_iters, seed,
                shift=0.0):
    """One pair.  xyz1 [3, n1], xyz2 [3, n2] fp32; idx rows [n1].  `shift` is
    added to the threshold (the band tests).  Returns a dict; `margin` is the
    least | residual - threshold | over every residual that decided a score
    or a mask."""
    n1 = xyz1.shape[1]
    out = dict(transform=np.eye(4), inliers=np.zeros(n1, np.int32), num_inliers=0, best_hyp=-1,
               scores=np.full(hyps, -1, np.int32), status=0, margin=np.inf)
    if m < 3:
        out["status"] = 1
        return out
    a32 = np.ascontiguousarray(xyz1[:, idx1[:m]].T).astype(np.float32)
    b32 = np.ascontiguousarray(xyz2[:, idx2[:m]].T).astype(np.float32)
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    thr = tau_of(inlier_dist) + shift
    tr = triples(seed, q, np.arange(hyps), m)
    ok = edge_ok(a32[tr], b32[tr], edge_ratio)
    margin = np.inf
    for h in np.nonzero(ok)[0]:
        r, t = kabsch(a[tr[h]], b[tr[h]])
        res = residuals(r, t, a, b)
        margin = min(margin, np.abs(res - thr).min())
        out["scores"][h] = int((res <= thr).sum())
    if not ok.any():
        out["status"] = 2
        return out
    bh = int(np.argmax(out["scores"]))  # first of the maxima: the lowest h
    r, t = kabsch(a[tr[bh]], b[tr[bh]])
    for _ in range(refine_iters):
        res = residuals(r, t, a, b)
        margin = min(margin, np.abs(res - thr).min())
        mask = res <= thr
        if mask.sum() < 3:
            break
        r, t = kabsch(a[mask], b[mask])
    res = residuals(r, t, a, b)
    margin = min(margin, np.abs(res - thr).min())
    mask = res <= thr
    out["transform"][:3, :3] = r
    out["transform"][:3, 3] = t
    out["inliers"][:m] = mask
    out["num_inliers"] = int(mask.sum())
    out["best_hyp"] = bh
    out["margin"] = float(margin)
    return out


def ransac(xyz1, xyz2, idx1, idx2, count, hyps, inlier_dist, edge_ratio, refine_iters, seed,
           shift=0.0):
    """The batch: stacked per-pair results, `margin` the least over the pairs."""
    res = [ransac_pair(xyz1[q], xyz2[q], idx1[q], idx2[q], int(count[q]), q, hyps, inlier_dist,
                       edge_ratio, refine_iters, seed, shift) for q in range(len(count))]
    keys = ("transform", "inliers", "num_inliers", "best_hyp", "scores", "status")
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in keys}
    out["margin"] = min(r["margin"] for r in res)
    return out


def rre_rte(gt, est):
    """RE_TE_one_pair (datasets/deepgmr_mn40.py:152-164), batched: degrees of
    acos(clamp((tr(Rgt^T Rest) - 1) / 2, -1, 1)) and |t_gt - t_est|"""
    gt, est = np.asarray(gt, np.float64), np.asarray(est, np.float64)
    tr = np.einsum("bij,bij->b", gt[:, :3, :3], est[:, :3, :3])
    rre = np.degrees(np.arccos(np.clip((tr - 1.0) / 2.0, -1.0, 1.0)))
    rte = np.linalg.norm(gt[:, :3, 3] - est[:, :3, 3], axis=1)
    return rre, rte
