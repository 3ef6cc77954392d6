"""HIP-event time per call of the TEASER-style robust registration (pcr_teaser,
DESIGN.md 4.8d) at the c4 shape -- 128 pairs per GPU x 1024 correspondences --
with 55 % and 90 % of the matches wrong and with every match correct (the
clique is all 1024 slots: the worst case of the rotation stage), noise-free
and with the inliers moved by up to the noise bound (the GNC loop then runs),
every slot a seed (seeds = 0) against 16 seeds.  The correct matches are the
first slots of every pair, so the stages come apart by differences of calls:
  solve   the call with inlier_selection off and count = the number of
          correct slots: the clique's points (but for a chance member or two),
          no graph and no search;
  graph   the call with seeds = 1 (one walk: the same clique) minus the solve;
  clique  the full call minus the call with seeds = 1;
  an iteration of the rotation: (max_iters = 11 minus max_iters = 1) / 10 of
  the solve call on the noisy pairs.
Diagnostic, not the bench.

  python scripts/teaser_probe.py [pairs] [points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "point-cloud-registration-based-on-rotation-invariant-feature_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
from pcr_amd import ops  # noqa: E402
from pcr_amd.registration import rre_rte  # noqa: E402

p, n = (int(a) for a in (sys.argv[1:3] + ["128", "1024"][len(sys.argv) - 1:]))
NOISE_BOUND = 0.02
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)


def timed(fn, warm=3, it=50):
    """median and minimum of `it` single calls, each between two HIP events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(it):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def ball(shape_p, shape_n):
    x = torch.randn((shape_p, 3, shape_n), device=dev, generator=gen)
    return x / x.norm(dim=1, keepdim=True) * \
        torch.rand((shape_p, 1, shape_n), device=dev, generator=gen) ** (1 / 3)


xyz1 = ball(p, n).contiguous()
rot, _ = torch.linalg.qr(torch.randn((p, 3, 3), device=dev, generator=gen, dtype=torch.float64))
rot = rot * torch.sign(torch.linalg.det(rot))[:, None, None]
shift = torch.rand((p, 3, 1), device=dev, generator=gen, dtype=torch.float64) - 0.5
moved = rot @ xyz1.double() + shift
idx = torch.arange(n, device=dev, dtype=torch.int32).repeat(p, 1).contiguous()
count = torch.full((p,), n, dtype=torch.int32, device=dev)
gt = torch.eye(4, device=dev, dtype=torch.float64).repeat(p, 1, 1)
gt[:, :3, :3], gt[:, :3, 3:] = rot, shift


def targets(wrong, noise):
    """the first (1 - wrong) n slots keep their target (moved by up to `noise`),
    the others get a random point of the unit cube"""
    good = n - int(wrong * n)
    x = (moved + noise * ball(p, n).double()).float()
    x[:, :, good:] = torch.rand((p, 3, n - good), device=dev, generator=gen) * 2 - 1
    return x.contiguous(), good


def report(name, wrong, noise):
    xyz2, good = targets(wrong, noise)

    def call(cnt=count, **kw):
        return ops.teaser(xyz1, xyz2, idx, idx, cnt, noise_bound=NOISE_BOUND, **kw)
    out = call()
    torch.cuda.synchronize()
    rre, rte = rre_rte(gt, out[0])
    size, its = out[2], out[5]
    print("%s: p=%d n=%d, %d correct slots per pair; clique min %d max %d, inliers min %d max %d, "
          "iterations min %d max %d, status 0 on %d / %d, RRE median %.3g max %.3g degrees, RTE "
          "median %.3g max %.3g" % (
              name, p, n, good, size.min().item(), size.max().item(), out[4].min().item(),
              out[4].max().item(), its.min().item(), its.max().item(),
              int((out[6] == 0).sum().item()), p, rre.median().item(), rre.max().item(),
              rte.median().item(), rte.max().item()))
    first = torch.full_like(count, good)
    full, low = timed(call)
    few, _ = timed(lambda: call(seeds=16))
    one, _ = timed(lambda: call(seeds=1))
    same = all(torch.equal(a, b) for a, b in zip(call(seeds=1)[1:3], out[1:3]))
    solve, _ = timed(lambda: call(first, inlier_selection=False))
    print("  ops.teaser: median %.3f ms  min %.3f ms;  seeds = 16: %.3f ms;  seeds = 1: %.3f ms "
          "(the same cliques: %s);  solve alone %.3f ms  ->  graph %.3f ms, clique %.3f ms "
          "(16 seeds: %.3f ms), solve %.3f ms" % (full, low, few, one, same, solve, one - solve,
                                                  full - one, few - one, solve))
    if its.min().item() >= 11:
        a, _ = timed(lambda: call(first, inlier_selection=False, max_iters=11))
        b, _ = timed(lambda: call(first, inlier_selection=False, max_iters=1))
        print("  rotation: %.1f us per iteration (max_iters 11: %.3f ms, 1: %.3f ms); the rest of "
              "the solve (first solve, largest residual, vote) %.3f ms" % (
                  (a - b) / 10 * 1e3, a, b, b))


for wrong in (0.55, 0.9, 0.0):
    report("%d %% wrong, noise-free" % round(100 * wrong), wrong, 0.0)
    report("%d %% wrong, inliers moved by up to the noise bound" % round(100 * wrong), wrong,
           NOISE_BOUND)
