"""HIP-event time per call of the hybrid (radius + max_nn) neighbour search
(ops.hybrid_search) and, in the same run on the same clouds,
of the KNN it replaces as FPFH's search (ops.knn_forward_cuda(xyz, xyz, k)):
the shapes, ellipsoid clouds and radii of scripts/fpfh_probe.py -- 128 clouds
x 1024 points with k = 32 and k = 100, 8 clouds x 16,384 points with k = 100.
Next to each: ops.fpfh with both searches (checked bit-identical first), and
how many points lie within the radius (the search's work).  Last, one ragged
batch: raw scans through ops.grid_subsample, its counts into the search and
into ops.fpfh(search="grid").  Diagnostic, not the bench.

  python scripts/hybrid_probe.py
  python scripts/hybrid_probe.py calls B N K    # 20 calls of one shape, for
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
    dist, idx, cnt, within = ops.hybrid_search(xyz, radius, k, return_within=True)
    kd, _, ki, _ = ops.knn_forward_cuda(xyz, xyz, k)
    filled = torch.arange(k, device=dev).view(1, k, 1) < cnt.unsqueeze(1)
    same = bool((idx[filled] == ki[filled]).all()) and \
        bool((dist[filled].view(torch.int32) == kd[filled].view(torch.int32)).all())
    f_grid = ops.fpfh(xyz, nrm, radius, k, search="grid")
    f_knn = ops.fpfh(xyz, nrm, radius, k, search="knn")
    same_f = bool((f_grid.view(torch.int32) == f_knn.view(torch.int32)).all())
    torch.cuda.synchronize()
    hyb, hyb_low = timed(lambda: ops.hybrid_search(xyz, radius, k))
    knn, knn_low = timed(lambda: ops.knn_forward_cuda(xyz, xyz, k))
    fg, fg_low = timed(lambda: ops.fpfh(xyz, nrm, radius, k, search="grid"))
    fk, fk_low = timed(lambda: ops.fpfh(xyz, nrm, radius, k, search="knn"))
    w = within.float()
    print("b=%d n=%d k=%d r=%.3g: within the radius mean %.1f min %d max %d; rows cut by max_nn "
          "%.1f %%" % (b, n, k, radius, float(w.mean()), int(within.min()), int(within.max()),
                       100.0 * float((within > k).float().mean())))
    print("    rows equal the KNN's in every filled slot: %s; fpfh grid == fpfh knn bit for bit: "
          "%s" % (same, same_f))
    print("    hybrid_search median %.3f ms min %.3f ms; knn_forward_cuda median %.3f ms min "
          "%.3f ms (x %.1f)" % (hyb, hyb_low, knn, knn_low, knn / hyb))
    print("    ops.fpfh search=grid median %.3f ms min %.3f ms; search=knn median %.3f ms min "
          "%.3f ms" % (fg, fg_low, fk, fk_low))
    assert same and same_f


def ragged(b, n, cell, radius, k):
    """raw scans (the ellipsoid with 1 % noise, each cloud cropped to a
    different share) -> grid_subsample -> counts -> the search and FPFH"""
    xyz, nrm = clouds(b, n)
    xyz = (xyz + 0.01 * torch.randn(xyz.shape, device=dev, generator=gen)).contiguous()
    raw = torch.tensor([n - (q * n) // (2 * b) for q in range(b)], dtype=torch.int32, device=dev)
    sub = ops.grid_subsample(xyz, cell, features=nrm, counts=raw)
    counts = sub["count"]
    sxyz = sub["xyz"]
    snrm = sub["features"]
    snrm = (snrm / snrm.norm(dim=1, keepdim=True).clamp_min(1e-20)).contiguous()
    dist, idx, cnt, within = ops.hybrid_search(sxyz, radius, k, counts, return_within=True)
    feat = ops.fpfh(sxyz, snrm, radius, k, search="grid", counts=counts)
    torch.cuda.synchronize()
    valid = torch.arange(n, device=dev).view(1, n) < counts.view(b, 1)
    assert bool((cnt[~valid] == 0).all()) and bool((feat.transpose(1, 2)[~valid] == 0).all())
    assert int(idx.max()) < int(counts.max()) and bool(torch.isfinite(feat).all())
    hyb, hyb_low = timed(lambda: ops.hybrid_search(sxyz, radius, k, counts))
    fg, fg_low = timed(lambda: ops.fpfh(sxyz, snrm, radius, k, search="grid", counts=counts))
    sub_ms, sub_low = timed(lambda: ops.grid_subsample(xyz, cell, features=nrm, counts=raw))
    print("ragged: b=%d raw points %d .. %d, cell %.3g -> counts %d .. %d of n=%d; r=%.3g k=%d: "
          "within the radius mean %.1f max %d" % (
              b, int(raw.min()), int(raw.max()), cell, int(counts.min()), int(counts.max()), n,
              radius, k, float(within[valid].float().mean()), int(within.max())))
    print("    grid_subsample median %.3f ms min %.3f ms; hybrid_search median %.3f ms min %.3f "
          "ms; ops.fpfh search=grid median %.3f ms min %.3f ms" % (
              sub_ms, sub_low, hyb, hyb_low, fg, fg_low))


if len(sys.argv) > 1 and sys.argv[1] == "calls":
    b_, n_, k_ = (int(a) for a in sys.argv[2:5])
    xyz_, _ = clouds(b_, n_)
    for _ in range(20):
        ops.hybrid_search(xyz_, RADIUS[(n_, k_)], k_)
    torch.cuda.synchronize()
    sys.exit(0)

print("device: %s" % torch.cuda.get_device_name(0))
case(128, 1024, 32)
case(128, 1024, 100)
case(8, 16384, 100)
ragged(8, 16384, 0.04, 0.2, 100)
