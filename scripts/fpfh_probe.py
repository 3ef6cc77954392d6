"""HIP-event time per call of the FPFH descriptors (ops.fpfh_from_neighbors,
DESIGN.md 4.8f) at 128 clouds x 1024 points with k = 32 and k = 100 and at
8 clouds x 16,384 points with k = 100, on an ellipsoid with analytic normals and a radius that admits about as many neighbours as the lists hold
(the worst case: nearly every slot is a pair).  Next to each, on the same GPU:
the KNN that makes the lists, both together (ops.fpfh), and the mutual-NN
matching of the first half of the clouds against the second at C = 33.  The
FPFH stage's gather is 33 * 4 bytes per neighbour, out of L2; the SPFH stage's
32 bytes per neighbour.  Per-kernel times come from a kernel trace of the
`calls` mode.  Diagnostic, not the bench.

  python scripts/fpfh_probe.py
  python scripts/fpfh_probe.py calls B N K    # 20 calls of one shape, for
                                              # rocprofv3 --kernel-trace --stats
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "point-cloud-registration-based-on-rotation-invariant-feature_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
from pcr_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)
AXES = torch.tensor([1.0, 0.8, 0.6], device=dev).view(1, 3, 1)
# radius per (n, k): about k neighbours inside it at n points on this surface
RADIUS = {(1024, 32): 0.36, (1024, 100): 0.62, (16384, 100): 0.155}


def timed(fn, warm=3, it=20):
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


def clouds(b, n):
    """points of the ellipsoid x^2 + (y / 0.8)^2 + (z / 0.6)^2 = 1 and its normals"""
    u = torch.randn((b, 3, n), device=dev, generator=gen)
    u = u / u.norm(dim=1, keepdim=True)
    xyz = (u * AXES).contiguous()
    nrm = u / AXES
    return xyz, (nrm / nrm.norm(dim=1, keepdim=True)).contiguous()


def case(b, n, k):
    radius = RADIUS[(n, k)]
    xyz, nrm = clouds(b, n)
    dist, _, idx, _ = ops.knn_forward_cuda(xyz, xyz, k)
    feat, cnt = ops.fpfh_from_neighbors(xyz, nrm, idx, dist, radius, return_counts=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(feat).all())
    m = float(cnt.float().mean())
    op, op_low = timed(lambda: ops.fpfh_from_neighbors(xyz, nrm, idx, dist, radius))
    knn, knn_low = timed(lambda: ops.knn_forward_cuda(xyz, xyz, k))
    both, both_low = timed(lambda: ops.fpfh(xyz, nrm, radius, k))
    p = b // 2
    mat, mat_low = timed(lambda: ops.mutual_nn_match(feat[:p], feat[p:], channel_major=True))
    print("b=%d n=%d k=%d r=%.3g: neighbours per point mean %.1f min %d max %d" % (
        b, n, k, radius, m, int(cnt.min()), int(cnt.max())))
    print("    fpfh_from_neighbors median %.3f ms min %.3f ms (%.1f MB of SPFH rows gathered, "
          "%.1f MB of packed points)" % (op, op_low, b * n * m * 132 / 1e6, b * n * m * 32 / 1e6))
    print("    knn_forward_cuda median %.3f ms min %.3f ms; ops.fpfh (both) median %.3f ms min "
          "%.3f ms" % (knn, knn_low, both, both_low))
    print("    mutual_nn_match of %d pairs at C = 33: median %.3f ms min %.3f ms" % (
        p, mat, mat_low))


if len(sys.argv) > 1 and sys.argv[1] == "calls":
    b_, n_, k_ = (int(a) for a in sys.argv[2:5])
    xyz_, nrm_ = clouds(b_, n_)
    dist_, _, idx_, _ = ops.knn_forward_cuda(xyz_, xyz_, k_)
    for _ in range(20):
        ops.fpfh_from_neighbors(xyz_, nrm_, idx_, dist_, RADIUS[(n_, k_)])
    torch.cuda.synchronize()
    sys.exit(0)

print("device: %s" % torch.cuda.get_device_name(0))
case(128, 1024, 32)
case(128, 1024, 100)
case(8, 16384, 100)
