"""HIP-event time per call of the Fast Global Registration (pcr_fgr, DESIGN.md
4.8c) at the c4 shape -- 128 pairs per GPU x 1024 correspondences, 55 % of
them wrong, the defaults (tuple test up to 1000 triples = 3000 correspondences,
64 iterations).  The tuple stage is the call with iterations = 0 (tuple kernel,
centroids, scale, staging); the loop is the rest, per iteration (full call -
that) / 64.  The same for max_tuples = 0 (the 1024 slots as they are), and for
16 slots per pair, where an iteration is all block sum and solve: the part of
an iteration that does not shrink with the list.  Diagnostic, not the bench.

  python scripts/fgr_probe.py [pairs] [points]
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
ITERS = 64
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


# any rotation, 55 % of the targets replaced: slot s pairs point s with point s
x = torch.randn((p, 3, n), device=dev, generator=gen)
xyz1 = (x / x.norm(dim=1, keepdim=True) *
        torch.rand((p, 1, n), device=dev, generator=gen) ** (1 / 3)).contiguous()
rot, _ = torch.linalg.qr(torch.randn((p, 3, 3), device=dev, generator=gen, dtype=torch.float64))
rot = rot * torch.sign(torch.linalg.det(rot))[:, None, None]
shift = torch.rand((p, 3, 1), device=dev, generator=gen, dtype=torch.float64) - 0.5
xyz2 = (rot @ xyz1.double() + shift).float()
bad = torch.rand((p, 1, n), device=dev, generator=gen) < 0.55
xyz2 = torch.where(bad, torch.rand((p, 3, n), device=dev, generator=gen) * 2 - 1, xyz2).contiguous()
idx = torch.arange(n, device=dev, dtype=torch.int32).repeat(p, 1).contiguous()
count = torch.full((p,), n, dtype=torch.int32, device=dev)
gt = torch.eye(4, device=dev, dtype=torch.float64).repeat(p, 1, 1)
gt[:, :3, :3], gt[:, :3, 3:] = rot, shift


def report(name, cnt, **kw):
    out = ops.fgr(xyz1, xyz2, idx, idx, cnt, **kw)
    torch.cuda.synchronize()
    rre, rte = rre_rte(gt, out[0])
    print("%s: p=%d n=%d, correspondences min %d max %d, trials min %d max %d, status 0 on %d / "
          "%d, RRE median %.3g max %.3g degrees, RTE median %.3g max %.3g" % (
              name, p, n, out[2].min().item(), out[2].max().item(), out[3].min().item(),
              out[3].max().item(), int((out[5] == 0).sum().item()), p, rre.median().item(),
              rre.max().item(), rte.median().item(), rte.max().item()))
    full, low = timed(lambda: ops.fgr(xyz1, xyz2, idx, idx, cnt, **kw))
    head, _ = timed(lambda: ops.fgr(xyz1, xyz2, idx, idx, cnt, iterations=0, **kw))
    print("  ops.fgr: median %.3f ms  min %.3f ms;  tuple stage (iterations = 0) %.3f ms;  loop "
          "%.3f ms = %.1f us per iteration" % (full, low, head, full - head,
                                               (full - head) / ITERS * 1e3))
    return (full - head) / ITERS * 1e3


a = report("defaults (tuple test)", count)
b = report("max_tuples = 0", count, max_tuples=0)
c = report("16 slots, max_tuples = 0", torch.full_like(count, 16), max_tuples=0)
print("block sum + solve %.1f us per iteration: %.0f %% of an iteration over 3000 correspondences, "
      "%.0f %% over %d" % (c, 100 * c / a, 100 * c / b, n))
