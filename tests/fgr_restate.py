"""numpy / fp64 restatement of the Fast Global Registration contract
(the kernels are csrc/fgr.hip, their scalar math
include/pcr_fgr.h and the sampler and edge check of include/pcr_rigid.h).
The tuple test is restated operation for operation (tests/rigid_restate.py:
integer sampler, fp64 edge lengths), vectorised over chunks of trials, and so
is the order of the centroids' sums (the only sums a decision hangs on: the
scale becomes mu with absolute_scale).  The loop is deliberately another
computation where the contract allows one: the normal equations are summed
from the explicit 3 x 6 Jacobian rows (28 sums; the kernel forms A and g from
16 moment sums), in numpy's order, ascending or descending (`order`), and the
step is np.linalg.solve (the kernel's is a Cholesky factorisation)."""
import numpy as np

from icp_restate import ball, motion
from rigid_restate import edge_ok, rre_rte, triples  # noqa: F401 (rre_rte: for the tests)

F32 = np.float32
THREADS = 512  # PCR_FGR_THREADS
MIN_CORR = 10
CHUNK = 4096
DEFAULTS = dict(max_corr_dist=0.08, iterations=64, division_factor=1.4, decrease_mu=True,
                tuple_scale=0.95, max_tuples=1000, trials_per_corr=100, absolute_scale=False,
                seed=0)
KEYS = ("transform", "slots", "num_corr", "num_trials", "mu", "status")


def ordered_sum(x):
    """pcr_fgr_sum: partial j takes i = j, j + THREADS, ... ascending; each 64
    consecutive partials meet in the xor butterfly; the results in order."""
    x = np.asarray(x, F32).astype(np.float64)
    rounds = -(-len(x) // THREADS)
    pad = np.zeros(max(rounds, 1) * THREADS)
    pad[:len(x)] = x
    part = np.zeros(THREADS)
    for r in range(rounds):
        part = part + pad[r * THREADS:(r + 1) * THREADS]
    v = part.reshape(-1, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    s = v[0, 0]
    for w in range(1, len(v)):
        s = s + v[w, 0]
    return s


def centroid(xyz):
    """xyz [3, n] fp32 -> fp64 [3]"""
    return np.array([ordered_sum(xyz[d]) for d in range(3)]) / np.float64(xyz.shape[1])


def norms(xyz, m):
    """pcr_fgr_norm of every point, [n]"""
    d = np.asarray(xyz, F32).astype(np.float64) - m[:, None]
    return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def tuple_test(a32, b32, m, q, tuple_scale, max_tuples, trials_per_corr, seed):
    """-> L (slots, int64), num_trials"""
    if max_tuples == 0:
        return np.arange(m, dtype=np.int64), 0
    trials = trials_per_corr * m
    kept, total = [], 0
    if m >= 3:
        for h0 in range(0, trials, CHUNK):
            h = np.arange(h0, min(h0 + CHUNK, trials))
            tr = triples(seed, q, h, m)
            ok = edge_ok(a32[tr], b32[tr], tuple_scale)
            take = min(int(ok.sum()), max_tuples - total)
            kept.append(tr[ok][:take])
            total += take
            if total >= max_tuples:
                return np.concatenate(kept).reshape(-1), int(h[ok][take - 1]) + 1
    if kept:
        return np.concatenate(kept).reshape(-1), trials
    return np.zeros(0, np.int64), trials


def euler(d):
    """Rz(d2) Ry(d1) Rx(d0)"""
    sa, ca, sb, cb, sc, cc = np.sin(d[0]), np.cos(d[0]), np.sin(d[1]), np.cos(d[1]), \
        np.sin(d[2]), np.cos(d[2])
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return rz @ ry @ rx


def fgr_pair(xyz1, xyz2, idx1, idx2, m, q, order=1, **kw):
    """One pair.  xyz1 [3, n1], xyz2 [3, n2] fp32; idx rows [n1]; m = count.
    order: +1 / -1, the direction of the loop's sums."""
    kw = dict(DEFAULTS, **kw)
    xyz1, xyz2 = np.asarray(xyz1, F32), np.asarray(xyz2, F32)
    n1, n2 = xyz1.shape[1], xyz2.shape[1]
    m = min(max(int(m), 0), n1)
    i1 = np.clip(np.asarray(idx1[:m], np.int64), 0, n1 - 1)
    i2 = np.clip(np.asarray(idx2[:m], np.int64), 0, n2 - 1)
    a32 = np.ascontiguousarray(xyz1[:, i1].T)
    b32 = np.ascontiguousarray(xyz2[:, i2].T)
    max_tuples = kw["max_tuples"]
    with np.errstate(all="ignore"):
        lst, num_trials = tuple_test(a32, b32, m, q, kw["tuple_scale"], max_tuples,
                                     kw["trials_per_corr"], kw["seed"])
    k = len(lst)
    slots = np.full(3 * max_tuples if max_tuples else n1, -1, np.int32)
    slots[:k] = lst
    out = dict(transform=np.eye(4), slots=slots, num_corr=k, num_trials=num_trials, mu=0.0,
               status=0)
    if k < MIN_CORR:
        out["status"] = 1
        return out
    with np.errstate(all="ignore"):
        m1, m2 = centroid(xyz1), centroid(xyz2)
        s = np.concatenate((norms(xyz1, m1), norms(xyz2, m2))).max()  # a NaN stays
    if not (s > 0 and np.isfinite(s)):
        out["status"] = 2
        return out
    d, mu = (1.0, float(s)) if kw["absolute_scale"] else (float(s), 1.0)
    p = (a32.astype(np.float64)[lst] - m1) / d
    q0 = (b32.astype(np.float64)[lst] - m2) / d
    r_, t_ = np.eye(3), np.zeros(3)
    jac = np.zeros((k, 3, 6))
    jac[:, 0, 3] = jac[:, 1, 4] = jac[:, 2, 5] = -1.0
    for it in range(kw["iterations"]):
        qq = q0 @ r_.T + t_
        res = p - qq
        w = mu / ((res * res).sum(axis=1) + mu)
        w = w * w
        jac[:, 0, 1], jac[:, 0, 2] = -qq[:, 2], qq[:, 1]
        jac[:, 1, 0], jac[:, 1, 2] = qq[:, 2], -qq[:, 0]
        jac[:, 2, 0], jac[:, 2, 1] = -qq[:, 1], qq[:, 0]
        ta = w[:, None, None] * np.einsum("cki,ckj->cij", jac, jac)
        tg = w[:, None] * np.einsum("cki,ck->ci", jac, res)
        amat, g = ta[::order].sum(axis=0), tg[::order].sum(axis=0)
        try:
            if not np.isfinite(amat).all():
                raise np.linalg.LinAlgError
            np.linalg.cholesky(amat)
        except np.linalg.LinAlgError:
            out["status"] = 3
            break
        delta = -np.linalg.solve(amat, g)
        rd = euler(delta[:3])
        r_, t_ = rd @ r_, rd @ t_ + delta[3:]
        if kw["decrease_mu"] and it % 4 == 0 and mu > kw["max_corr_dist"]:
            mu /= kw["division_factor"]
    out["transform"][:3, :3] = r_.T
    out["transform"][:3, 3] = m2 - r_.T @ (d * t_ + m1)
    out["mu"] = mu
    return out


def fgr(xyz1, xyz2, idx1, idx2, count, order=1, **kw):
    """The batch: stacked per-pair results."""
    res = [fgr_pair(xyz1[q], xyz2[q], idx1[q], idx2[q], int(count[q]), q, order, **kw)
           for q in range(len(count))]
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in KEYS}
    for k in ("num_corr", "num_trials", "status"):
        out[k] = out[k].astype(np.int32)
    return out


def order_gap(xyz1, xyz2, idx1, idx2, count, **kw):
    """The restatement with its sums ascending and descending: (the ascending
    result, the largest difference of the two transforms).  The tests'
    condition for the 1e-8 bound: a gap <= 1e-11 and equal statuses."""
    up = fgr(xyz1, xyz2, idx1, idx2, count, 1, **kw)
    down = fgr(xyz1, xyz2, idx1, idx2, count, -1, **kw)
    assert np.array_equal(up["status"], down["status"])
    return up, float(np.abs(up["transform"] - down["transform"]).max())


# ------------------------------------------------------------ synthetic pairs
def make_pair(rng, n1, n2, wrong=0.0, m=None, degrees=40.0, tnorm=0.5):
    """Source points in the unit ball (rounded to fp32); the target is a
    permuted superset (n2 >= n1) moved by R a + t and rounded to fp32.  Slot s
    < m pairs source s with its counterpart, a fraction `wrong` of the slots
    with a random target instead.  -> xyz1 [3, n1], xyz2 [3, n2], idx1, idx2
    [n1] (-1 past m), m, gt [4, 4]"""
    a = ball(rng, n1).astype(F32)
    gt = motion(rng, degrees, tnorm)
    pts = np.concatenate((a.astype(np.float64), ball(rng, n2 - n1)))
    perm = rng.permutation(n2)
    tgt = (pts @ gt[:3, :3].T + gt[:3, 3])[perm]
    pos = np.empty(n2, np.int64)
    pos[perm] = np.arange(n2)
    m = n1 if m is None else m
    idx1, idx2 = np.full(n1, -1, np.int32), np.full(n1, -1, np.int32)
    idx1[:m] = np.arange(m)
    idx2[:m] = pos[:m]
    bad = rng.permutation(m)[:int(wrong * m)]
    idx2[bad] = rng.integers(0, n2, len(bad))
    return (np.ascontiguousarray(a.T), np.ascontiguousarray(tgt.T.astype(F32)), idx1, idx2, m, gt)


def make_batch(seed, p, n1, n2, **kw):
    """-> xyz1 [p, 3, n1], xyz2 [p, 3, n2], idx1, idx2 [p, n1], count [p] int32, gt [p, 4, 4]"""
    rng = np.random.default_rng(seed)
    pairs = [make_pair(rng, n1, n2, **kw) for _ in range(p)]
    out = [np.stack([pr[k] for pr in pairs]) for k in range(6)]
    out[4] = out[4].astype(np.int32)
    return tuple(out)
