"""HIP-event time per call of the point-to-plane ICP (pcr_icp_point_to_plane,
DESIGN.md 4.8i) beside the point-to-point one (4.8b) in the same run, on pairs
of two independent samplings of one ellipsoid (semi-axes 1 / 0.8 / 0.6, 5
degrees and |t| = 0.03 apart, analytic target normals), max_dist 0.2, 200
iterations allowed, Open3D's default criteria:
  dense   128 pairs per GPU x 1024 x 1024 points;
  ragged  the same strides with counts drawn from [n / 2, n];
then registration.scan_pairs with both refinements on one set of raw scan
pairs.  Per-iteration time is (full call - pure evaluation) / iterations of
the slowest pair; the bound is 9 fp32 VALU operations per (source, target)
pair at 128 lanes per clock and CU, 2.4 GHz, one CU per pair.  Diagnostic, not
the bench.

  python scripts/icp_plane_probe.py [pairs] [points]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "point-cloud-registration-based-on-rotation-invariant-feature_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
from pcr_amd import ops, registration  # noqa: E402

p, n = (int(a) for a in (sys.argv[1:3] + ["128", "1024"][len(sys.argv) - 1:]))
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)
AXES = torch.tensor([1.0, 0.8, 0.6], device=dev, dtype=torch.float64)[None, :, None]


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


def ellipsoid(count):
    """[p, 3, count] fp64 points and their unit normals"""
    u = torch.randn((p, 3, count), device=dev, generator=gen, dtype=torch.float64)
    x = u / u.norm(dim=1, keepdim=True) * AXES
    nrm = x / (AXES * AXES)
    return x, nrm / nrm.norm(dim=1, keepdim=True)


def rotations(degrees):
    ax = torch.randn((p, 3), device=dev, generator=gen, dtype=torch.float64)
    ax = ax / ax.norm(dim=1, keepdim=True)
    k = torch.zeros((p, 3, 3), device=dev, dtype=torch.float64)
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    th = torch.deg2rad(torch.tensor(float(degrees), dtype=torch.float64, device=dev))
    return torch.eye(3, device=dev, dtype=torch.float64) + torch.sin(th) * k + \
        (1 - torch.cos(th)) * (k @ k)


def report(name, xyz1, xyz2, nrm2, gt, **counts):
    bound = n * n * 9 / 128 / 2.4e3  # us per evaluation of one full pair on one CU
    print("%s: p=%d n=%d" % (name, p, n))
    for est, kw in (("point_to_point", {}),
                    ("point_to_plane", dict(estimation="point_to_plane", normals2=nrm2))):
        kw = dict(kw, **counts)
        out = ops.icp(xyz1, xyz2, **kw)
        torch.cuda.synchronize()
        its = out[5]
        err = (out[0][:, :3] - gt).abs().amax(dim=(1, 2))
        full, low = timed(lambda: ops.icp(xyz1, xyz2, **kw))
        ev, _ = timed(lambda: ops.icp(xyz1, xyz2, max_iters=0, **kw))
        mx = max(int(its.max().item()), 1)
        per = (full - ev) / mx * 1e3
        print("  %s: iterations min %d median %d max %d, status 0 on %d / %d, transform error "
              "median %.2g max %.2g" % (est, its.min().item(), its.median().item(), mx,
                                        int((out[6] == 0).sum().item()), p,
                                        err.median().item(), err.max().item()))
        print("    median %.3f ms  min %.3f ms;  pure evaluation %.3f ms;  %.1f us per iteration"
              ";  fp32 VALU bound %.1f us: an iteration runs at %.0f %% of it"
              % (full, low, ev, per, bound, 100 * bound / per))


src, _ = ellipsoid(n)
tgt, tn = ellipsoid(n)
rot = rotations(5.0)
shift = torch.randn((p, 3, 1), device=dev, generator=gen, dtype=torch.float64)
shift = shift / shift.norm(dim=1, keepdim=True) * 0.03
gt = torch.cat((rot, shift), dim=2)
xyz1 = src.float().contiguous()
xyz2 = (rot @ tgt + shift).float().contiguous()
nrm2 = (rot @ tn).float().contiguous()
report("dense, two samplings of an ellipsoid", xyz1, xyz2, nrm2, gt)
c1 = torch.randint(n // 2, n + 1, (p,), device=dev, generator=gen, dtype=torch.int32)
c2 = torch.randint(n // 2, n + 1, (p,), device=dev, generator=gen, dtype=torch.int32)
report("ragged, counts in [n / 2, n]", xyz1, xyz2, nrm2, gt, counts1=c1, counts2=c2)


# ---- scan_pairs with both refinements on one set of raw scan pairs
def surface(count, g):
    """a bumpy height field over [-1, 1]^2, lifted away from the origin"""
    u = torch.rand(count, device=dev, generator=g, dtype=torch.float64) * 2 - 1
    v = torch.rand(count, device=dev, generator=g, dtype=torch.float64) * 2 - 1
    z = (0.35 * torch.exp(-((u - 0.4) ** 2 + (v + 0.3) ** 2) / 0.08)
         - 0.30 * torch.exp(-((u + 0.5) ** 2 + (v - 0.45) ** 2) / 0.05)
         + 0.25 * torch.exp(-((u + 0.3) ** 2 + (v + 0.6) ** 2) / 0.03)
         + 0.15 * torch.sin(2.3 * u) * torch.cos(1.7 * v) + 0.1 * u * v)
    return torch.stack((u, v, z + 3.0))


sp = min(p, 16)
sizes = torch.randint(6000, 12001, (2 * sp,), generator=torch.Generator().manual_seed(1)).tolist()
rot = rotations(25.0)[:sp]
scans1, scans2, gts = [], [], []
for q in range(sp):
    t = torch.randn((3, 1), device=dev, generator=gen, dtype=torch.float64)
    t = 0.4 * t / t.norm()
    scans1.append(surface(sizes[2 * q], gen).float().contiguous())
    scans2.append((rot[q] @ surface(sizes[2 * q + 1], gen) + t).float().contiguous())
    g4 = torch.eye(4, device=dev, dtype=torch.float64)
    g4[:3, :3], g4[:3, 3:] = rot[q], t
    gts.append(g4)
gts = torch.stack(gts)
print("scan_pairs: %d pairs of %d .. %d raw points, cell 0.05" % (sp, min(sizes), max(sizes)))
for est in ("point_to_point", "point_to_plane"):
    icp = dict(estimation=est)
    out = registration.scan_pairs(scans1, scans2, 0.05, icp=icp)
    torch.cuda.synchronize()
    full, low = timed(lambda: registration.scan_pairs(scans1, scans2, 0.05, icp=icp), 3, 20)
    none, _ = timed(lambda: registration.scan_pairs(scans1, scans2, 0.05), 3, 20)
    its = out["icp_iterations"]
    rm = torch.stack([registration.alignment_rmse(
        out["xyz1"][q:q + 1, :, :int(out["counts1"][q])].contiguous(), gts[q:q + 1],
        out["icp_transform"][q:q + 1])[0] for q in range(sp)])
    print("  %s: chain median %.3f ms (min %.3f; without the refinement %.3f), subsampled to "
          "%d .. %d points, iterations median %d max %d, icp_status 0 on %d / %d, alignment rmse "
          "median %.3g max %.3g" % (est, full, low, none, int(out["counts1"].min()),
                                    int(out["counts1"].max()), its.median().item(),
                                    its.max().item(), int((out["icp_status"] == 0).sum().item()),
                                    sp, rm.median().item(), rm.max().item()))
