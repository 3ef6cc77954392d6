"""HIP-event time per call of the ragged ops, each beside its
dense twin in the same run on the same tensors:

  * ops.mutual_nn_match, ops.icp and ops.fgr at 128 pairs x 1024 points --
    dense, ragged with full counts (the same work through the ragged
    instantiation), ragged with counts drawn from 50-100 % of n;
  * ops.estimate_normals_hybrid (hybrid_search + normals_from_neighbors, and
    the latter alone) beside the brute-force ops.estimate_normals at 128 x 1024
    and 8 x 16,384 points;
  * registration.scan_pairs on 8 pairs of 65,536-point scans.

Timing: warm-up calls, then single calls between two HIP events; median and
minimum.  Diagnostic, not the bench.

  python scripts/ragged_probe.py
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "point-cloud-registration-based-on-rotation-invariant-feature_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
from pcr_amd import ops, registration  # noqa: E402

dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)
AXES = torch.tensor([1.0, 0.8, 0.6], device=dev).view(1, 3, 1)


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


def ellipsoid(b, n, shift=0.0):
    """points of x^2 + (y / 0.8)^2 + (z / 0.6)^2 = 1, moved along z"""
    u = torch.randn((b, 3, n), device=dev, generator=gen)
    u = u / u.norm(dim=1, keepdim=True)
    xyz = u * AXES
    xyz[:, 2] += shift
    return xyz.contiguous()


def motion(p, degrees, tnorm):
    """[p, 4, 4] fp64: a rotation about a random axis and a translation"""
    ax = torch.randn((p, 3), device=dev, generator=gen, dtype=torch.float64)
    ax = ax / ax.norm(dim=1, keepdim=True)
    k = torch.zeros((p, 3, 3), device=dev, dtype=torch.float64)
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0] = -ax[:, 2], ax[:, 1], ax[:, 2]
    k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -ax[:, 0], -ax[:, 1], ax[:, 0]
    a = math.radians(degrees)
    t = torch.eye(4, device=dev, dtype=torch.float64).repeat(p, 1, 1)
    t[:, :3, :3] += math.sin(a) * k + (1 - math.cos(a)) * (k @ k)
    d = torch.randn((p, 3), device=dev, generator=gen, dtype=torch.float64)
    t[:, :3, 3] = tnorm * d / d.norm(dim=1, keepdim=True)
    return t


def report(name, rows):
    print("%s:" % name)
    for label, (med, low) in rows:
        print("    %-34s median %.3f ms min %.3f ms" % (label, med, low))


def twins(p, n):
    full = torch.full((p,), n, dtype=torch.int32, device=dev)
    part = torch.randint(n // 2, n + 1, (p,), device=dev, generator=gen).to(torch.int32)
    print("128 x 1024 twins: partial counts %d .. %d, mean %.0f" % (
        int(part.min()), int(part.max()), float(part.float().mean())))
    f1 = torch.randn((p, 33, n), device=dev, generator=gen)
    f2 = (f1 + 0.05 * torch.randn((p, 33, n), device=dev, generator=gen)).contiguous()
    ws = torch.empty(2 * p * n * 8 + 512, dtype=torch.uint8, device=dev)

    def match(c1, c2):
        return lambda: ops.mutual_nn_match(f1, f2, channel_major=True, workspace=ws,
                                           counts1=c1, counts2=c2)
    d = ops.mutual_nn_match(f1, f2, channel_major=True)
    r = ops.mutual_nn_match(f1, f2, channel_major=True, counts1=full, counts2=full)
    assert all(bool((a == b).all()) for a, b in zip(d, r))
    report("mutual_nn_match, c = 33 channel-major", [
        ("dense", timed(match(None, None))), ("ragged, full counts", timed(match(full, full))),
        ("ragged, 50-100 % counts", timed(match(part, part)))])

    x1 = ellipsoid(p, n)
    gt = motion(p, 4.0, 0.03)
    x2 = registration.apply_transform(x1, gt).float().contiguous()

    def icp(c1, c2):
        return lambda: ops.icp(x1, x2, max_iters=30, counts1=c1, counts2=c2)
    d, r = ops.icp(x1, x2, max_iters=30), ops.icp(x1, x2, max_iters=30, counts1=full, counts2=full)
    assert all(bool((a.view(torch.uint8) == b.view(torch.uint8)).all()) for a, b in zip(d, r))
    print("    icp iterations (dense): mean %.1f" % float(d[5].float().mean()))
    report("icp, max_iters = 30", [
        ("dense", timed(icp(None, None))), ("ragged, full counts", timed(icp(full, full))),
        ("ragged, 50-100 % counts", timed(icp(part, part)))])

    idx = torch.arange(n, dtype=torch.int32, device=dev).repeat(p, 1).contiguous()
    gt = motion(p, 40.0, 0.5)
    y2 = registration.apply_transform(x1, gt).float().contiguous()

    def fgr(cnt, c1, c2):
        return lambda: ops.fgr(x1, y2, idx, idx, cnt, counts1=c1, counts2=c2)
    d, r = ops.fgr(x1, y2, idx, idx, full), ops.fgr(x1, y2, idx, idx, full, counts1=full,
                                                    counts2=full)
    assert all(bool((a.view(torch.uint8) == b.view(torch.uint8)).all()) for a, b in zip(d, r))
    report("fgr, defaults (tuple test, 64 iterations)", [
        ("dense", timed(fgr(full, None, None))),
        ("ragged, full counts", timed(fgr(full, full, full))),
        ("ragged, 50-100 % counts", timed(fgr(part, part, part)))])


def normals(b, n, radius, k=30):
    xyz = ellipsoid(b, n, shift=3.0)
    _, idx, cnt, within = ops.hybrid_search(xyz, radius, k, return_within=True)
    brute = ops.estimate_normals(xyz, radius)
    lists = ops.normals_from_neighbors(xyz, idx)
    cos = (brute * lists).sum(dim=1)
    uncut = within <= k
    print("normals b=%d n=%d r=%.3g k=%d: within the radius mean %.1f, rows cut by max_nn "
          "%.1f %%; smallest cosine to the brute-force normal where the row is whole: %.9f"
          % (b, n, radius, k, float(within.float().mean()),
             100.0 * float((~uncut).float().mean()),
             float(cos[uncut].min()) if bool(uncut.any()) else float("nan")))
    report("    per call", [
        ("estimate_normals (brute force)", timed(lambda: ops.estimate_normals(xyz, radius))),
        ("estimate_normals_hybrid", timed(lambda: ops.estimate_normals_hybrid(xyz, radius, k))),
        ("hybrid_search alone", timed(lambda: ops.hybrid_search(xyz, radius, k))),
        ("normals_from_neighbors alone", timed(lambda: ops.normals_from_neighbors(xyz, idx)))])


def scans(p, n, cell):
    s1, s2 = [], []
    gt = motion(p, 30.0, 0.4)
    for q in range(p):
        m1 = n - 4096 * q
        m2 = n - 4096 * ((q + 3) % p)
        a = ellipsoid(1, m1, shift=3.0)[0]
        b = ellipsoid(1, m2, shift=3.0)[0]
        # not a solid of revolution: a bump, so that the pose is determined
        for x in (a, b):
            x[2] += 0.25 * torch.exp(-((x[0] - 0.5) ** 2 + (x[1] - 0.2) ** 2) / 0.05)
        b = registration.apply_transform(b[None], gt[q:q + 1])[0].float()
        s1.append(a.contiguous())
        s2.append(b.contiguous())
    out = registration.scan_pairs(s1, s2, cell, icp={})
    torch.cuda.synchronize()
    x1 = out["xyz1"]
    valid = torch.arange(x1.shape[2], device=dev)[None] < out["counts1"][:, None]
    moved = (registration.apply_transform(x1, out["icp_transform"]) -
             registration.apply_transform(x1, gt)).norm(dim=1)
    rmse = (moved * valid).sum(dim=1) / out["counts1"]
    print("scan_pairs: %d pairs of %d .. %d raw points, cell %.3g -> counts %d .. %d (stride %d); "
          "mutual matches %d .. %d; reg_status %s; alignment rmse over the valid points %.4f .. "
          "%.4f" % (p, min(s.shape[1] for s in s1 + s2), n, cell,
                    int(torch.minimum(out["counts1"], out["counts2"]).min()),
                    int(torch.maximum(out["counts1"], out["counts2"]).max()), x1.shape[2],
                    int(out["count"].min()), int(out["count"].max()),
                    out["reg_status"].tolist(), float(rmse.min()), float(rmse.max())))
    report("    per call", [("scan_pairs, ransac + icp",
                             timed(lambda: registration.scan_pairs(s1, s2, cell, icp={}),
                                   warm=1, it=5))])


def main():
    print("device:", torch.cuda.get_device_name(0))
    twins(128, 1024)
    normals(128, 1024, 0.36)
    normals(8, 16384, 0.09)
    scans(8, 65536, 0.04)


if __name__ == "__main__":
    main()
