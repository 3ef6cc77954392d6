"""numpy model of knn_wsel_kernel's threshold passes (csrc/knn_wsel.hip, step
2) over the bench's clouds: the mean number of count passes per query under
two policies for a query's first threshold.

  own     the product's: the threshold the wave's previous query ended with
          (12 waves take the block's 64 queries one at a time, so ~12 Morton
          positions back); a wave's first query starts from its distance to
          the far corner of its block's box;
  shared  a per-block array of final thresholds: a wave starts from the
          nearest query below its own that has already finished, else as
          `own`.

The 12 waves of a block are simulated as an event queue: the next query goes
to the wave that is free first, a query costs BASE + PASS cycles per pass
(DESIGN.md 4.3's phase clocks), and `finished` means finished before the
reader starts.  The pass loop is the kernel's: count(d <= t) against the
window [k, 64], the t^1.5 step towards (k + 64) / 2 for three passes, then
bisection of the float bits, bracketed.  Clouds are sorted like knn_sort.hip:
the top 12 bits of the 30-bit Morton code in the cloud's box, input order
inside a cell.
usage: python scripts/wsel_seed_model.py [clouds [n [k [waves]]]]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clouds import gaussian_clouds  # noqa: E402

TMAX = 0x461C3FFF
BASE, PASS = 2900, 1000  # cycles per query outside / per pass (4.3)


def spread10(v):
    v = v & 0x3FF
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def morton_order(p):
    """p [3, n] -> the sort's order (coarse: 16^3 cells, stable inside)."""
    lo, hi = p.min(axis=1, keepdims=True), p.max(axis=1, keepdims=True)
    q = np.clip(((p - lo) * (np.float32(1023.0) / (hi - lo))).astype(np.int64), 0, 1023)
    code = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2)
    return np.argsort(code >> 18, kind="stable")


def bits(f):
    return int(np.float32(f).view(np.int32))


def passes_from(dsorted, k, tb):
    """The kernel's pass loop on one query's ascending distance bits; returns
    (passes, final threshold bits)."""
    tgt = 0.5 * (k + 64)
    lo, hi = -1, 0x7F800000
    npass = 0
    while True:
        cnt = int(np.searchsorted(dsorted, tb, side="right"))
        npass += 1
        if k <= cnt <= 64:
            return npass, tb
        if cnt < k:
            lo = tb
            if tb >= TMAX:
                return npass, tb
        else:
            hi = tb
        if hi - lo <= 1:
            return npass, tb  # ties: the exact path, no more count passes
        if npass <= 3:
            f = float(np.int32(tb).view(np.float32)) * (tgt / max(cnt, 1)) ** (2.0 / 3.0)
            nb = bits(f) if f < 1e30 else TMAX
        else:
            nb = lo + ((hi - lo) >> 1)
        nb = min(nb, TMAX)
        if nb <= lo or nb >= hi:
            nb = lo + ((hi - lo) >> 1)
        tb = nb


def block_passes(dbits, pts, k, waves, shared):
    """One 64-query block: dbits [64][n] ascending distance bits per query,
    pts [64, 3] the block's points.  Returns the passes of each query."""
    nq = dbits.shape[0]
    free = np.zeros(waves)          # when each wave is free
    own = [None] * waves            # its previous final threshold
    done_at = np.full(nq, np.inf)
    final = np.zeros(nq, dtype=np.int64)
    out = np.zeros(nq, dtype=np.int64)
    bmin, bmax = pts.min(axis=0), pts.max(axis=0)
    for qi in range(nq):
        w = int(np.argmin(free))
        t0 = free[w]
        seed = own[w]
        if shared:
            fin = np.nonzero(done_at[:qi] <= t0)[0]
            if fin.size:
                seed = final[fin[-1]]
        if seed is None:
            g = np.maximum(np.abs(pts[qi] - bmin), np.abs(pts[qi] - bmax)).astype(np.float32)
            u = np.float32(g[0] * g[0]) + np.float32(g[1] * g[1]) + np.float32(g[2] * g[2])
            seed = bits(u) if (nq >= k and u < 10000.0) else TMAX
        out[qi], final[qi] = passes_from(dbits[qi], k, int(seed))
        own[w] = final[qi]
        free[w] = t0 + BASE + PASS * out[qi]
        done_at[qi] = free[w]
    return out


def main():
    a = [int(v) for v in sys.argv[1:]]
    b, n, k, waves = (a + [32, 1024, 32, 12][len(a):])[:4]
    xyz = gaussian_clouds(b, n, seed=0)[0]
    tot = {False: 0, True: 0}
    nqs = 0
    for c in range(b):
        p = xyz[c][:, morton_order(xyz[c])].T.astype(np.float32)  # [n, 3] sorted
        for q0 in range(0, n, 64):
            blk = p[q0:q0 + 64]
            d = blk[:, None, :] - p[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
            db = np.sort(d2.astype(np.float32).view(np.int32).astype(np.int64), axis=1)
            for shared in (False, True):
                tot[shared] += int(block_passes(db, blk, k, waves, shared).sum())
            nqs += blk.shape[0]
    print("b=%d n=%d k=%d waves=%d: passes per query own %.3f  shared %.3f  (gain %.3f)" % (
        b, n, k, waves, tot[False] / nqs, tot[True] / nqs, (tot[False] - tot[True]) / nqs))


if __name__ == "__main__":
    main()
