"""HIP-event time per call of the point-to-point ICP (pcr_icp_point_to_point,
DESIGN.md 4.8b) at the c4 shape -- 128 pairs per GPU x 1024 x 1024 points,
max_dist 0.2, 200 iterations allowed, Open3D's default criteria -- once as a
solver from the identity on 5 degree pairs, once as the refinement of
pcr_rigid_ransac's transform on pairs with 55 % of the targets replaced.
Per-iteration time is (full call - pure evaluation) / iterations of the
slowest pair; the bound is 9 fp32 VALU operations per (source, target) pair at
128 lanes per clock and CU, 2.4 GHz, one CU per pair.  Diagnostic, not the
bench.

  python scripts/icp_probe.py [pairs] [points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "point-cloud-registration-based-on-rotation-invariant-feature_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
from pcr_amd import ops  # noqa: E402

p, n = (int(a) for a in (sys.argv[1:3] + ["128", "1024"][len(sys.argv) - 1:]))
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)


def timed(fn, warm=5, it=50):
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


def ball():
    x = torch.randn((p, 3, n), device=dev, generator=gen)
    return x / x.norm(dim=1, keepdim=True) * torch.rand((p, 1, n), device=dev,
                                                        generator=gen) ** (1 / 3)


def rotations(degrees):
    ax = torch.randn((p, 3), device=dev, generator=gen, dtype=torch.float64)
    ax = ax / ax.norm(dim=1, keepdim=True)
    k = torch.zeros((p, 3, 3), device=dev, dtype=torch.float64)
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    th = torch.deg2rad(torch.tensor(float(degrees), dtype=torch.float64, device=dev))
    return torch.eye(3, device=dev, dtype=torch.float64) + torch.sin(th) * k + \
        (1 - torch.cos(th)) * (k @ k)


def report(name, xyz1, xyz2, init, rot):
    out = ops.icp(xyz1, xyz2, init)
    torch.cuda.synchronize()
    its = out[5]
    err = (out[0][:, :3, :3] - rot).abs().amax().item()
    print("%s: p=%d n=%d, iterations min %d median %d max %d, status 0 on %d / %d, "
          "max |R - R_gt| %.2g" % (name, p, n, its.min().item(), its.median().item(),
                                   its.max().item(), int((out[6] == 0).sum().item()), p, err))
    full, low = timed(lambda: ops.icp(xyz1, xyz2, init))
    ev, _ = timed(lambda: ops.icp(xyz1, xyz2, init, max_iters=0))
    mx = max(int(its.max().item()), 1)
    per = (full - ev) / mx * 1e3
    bound = n * n * 9 / 128 / 2.4e3  # us per evaluation of one pair on one CU
    print("  ops.icp: median %.3f ms  min %.3f ms;  pure evaluation %.3f ms;  %.1f us per "
          "iteration (scan + solve)" % (full, low, ev, per))
    print("  fp32 VALU bound %.1f us per evaluation: the evaluation runs at %.0f %% of it, an "
          "iteration at %.0f %%" % (bound, 100 * bound / (ev * 1e3), 100 * bound / per))


# solver: 5 degree pairs, |t| = 0.03, the target a permuted moved copy
xyz1 = ball().contiguous()
rot = rotations(5.0)
shift = torch.randn((p, 3, 1), device=dev, generator=gen, dtype=torch.float64)
shift = shift / shift.norm(dim=1, keepdim=True) * 0.03
perm = torch.argsort(torch.rand((p, n), device=dev, generator=gen), dim=1)
moved = (rot @ xyz1.double() + shift).float()
xyz2 = torch.gather(moved, 2, perm[:, None, :].expand(p, 3, n)).contiguous()
report("from the identity, 5 degrees", xyz1, xyz2, None, rot)

# refinement: any rotation, 55 % of the targets replaced, RANSAC first
rot, _ = torch.linalg.qr(torch.randn((p, 3, 3), device=dev, generator=gen, dtype=torch.float64))
rot = rot * torch.sign(torch.linalg.det(rot))[:, None, None]
shift = torch.rand((p, 3, 1), device=dev, generator=gen, dtype=torch.float64) - 0.5
xyz2 = (rot @ xyz1.double() + shift).float()
bad = torch.rand((p, 1, n), device=dev, generator=gen) < 0.55
xyz2 = torch.where(bad, torch.rand((p, 3, n), device=dev, generator=gen) * 2 - 1, xyz2).contiguous()
idx = torch.arange(n, device=dev, dtype=torch.int32).repeat(p, 1).contiguous()
count = torch.full((p,), n, dtype=torch.int32, device=dev)
est = ops.rigid_ransac(xyz1, xyz2, idx, idx, count, hyps=1000, inlier_dist=0.02, edge_ratio=0.9,
                       refine_iters=2, seed=1)[0]
report("refinement of rigid_ransac", xyz1, xyz2, est, rot)
