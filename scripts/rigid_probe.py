"""HIP-event time per call of the rigid-transform estimation (pcr_rigid_ransac,
DESIGN.md 4.8a) at the c4 shape -- 128 pairs per GPU x 1024 correspondences x
1000 hypotheses, tau = 0.02, rho = 0.9, two refits, 55 % wrong matches -- next
to the matching that feeds it (pcr_mutual_nn_match_cm, 128 pairs x 1024 points,
C = 64).  Diagnostic, not the bench.

  python scripts/rigid_probe.py [pairs] [correspondences] [hyps]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "point-cloud-registration-based-on-rotation-invariant-feature_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
from pcr_amd import _lib, ops  # noqa: E402
from pcr_amd.ops import _ptr  # noqa: E402

p, n, hyps = (int(a) for a in (sys.argv[1:4] + ["128", "1024", "1000"][len(sys.argv) - 1:]))
dev = torch.device("cuda:0")
lib = _lib.load()
gen = torch.Generator(device=dev).manual_seed(0)
stream = torch.cuda.current_stream().cuda_stream


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


# pairs: source points in the unit ball, targets = R a + t, 55 % of them replaced
xyz1 = torch.randn((p, 3, n), device=dev, generator=gen)
xyz1 = xyz1 / xyz1.norm(dim=1, keepdim=True) * torch.rand((p, 1, n), device=dev,
                                                         generator=gen) ** (1 / 3)
rot, _ = torch.linalg.qr(torch.randn((p, 3, 3), device=dev, generator=gen))
rot = rot * torch.sign(torch.linalg.det(rot))[:, None, None]
shift = torch.rand((p, 3, 1), device=dev, generator=gen) - 0.5
xyz2 = rot @ xyz1 + shift
bad = torch.rand((p, 1, n), device=dev, generator=gen) < 0.55
xyz2 = torch.where(bad, torch.rand((p, 3, n), device=dev, generator=gen) * 2 - 1, xyz2).contiguous()
idx = torch.arange(n, device=dev, dtype=torch.int32).repeat(p, 1).contiguous()
count = torch.full((p,), n, dtype=torch.int32, device=dev)
ws = torch.empty(max(256, lib.pcr_rigid_ransac_workspace_size(p, n, hyps)), dtype=torch.uint8,
                 device=dev)
kw = dict(hyps=hyps, inlier_dist=0.02, edge_ratio=0.9, refine_iters=2, seed=1, workspace=ws)

out = ops.rigid_ransac(xyz1, xyz2, idx, idx, count, return_scores=True, **kw)
torch.cuda.synchronize()
err = (out[0][:, :3, :3] - rot.double()).abs().amax().item()
print("p=%d m=%d hyps=%d: %.1f%% of the hypotheses pass the edge check, status ok %d / %d, "
      "max |R - R_gt| %.2g" % (p, n, hyps, 100.0 * (out[5] >= 0).double().mean().item(),
                               int((out[4] == 0).sum().item()), p, err))
med, low = timed(lambda: ops.rigid_ransac(xyz1, xyz2, idx, idx, count, **kw))
print("rigid_ransac (ops, allocates its outputs): median %.3f ms  min %.3f ms" % (med, low))

i32 = dict(dtype=torch.int32, device=dev)
tr = torch.empty((p, 4, 4), dtype=torch.float64, device=dev)
inl = torch.empty((p, n), **i32)
num, best, status = (torch.empty((p,), **i32) for _ in range(3))


def raw(scores=None):
    _lib.check(lib.pcr_rigid_ransac(
        _ptr(xyz1), _ptr(xyz2), p, n, n, _ptr(idx), _ptr(idx), _ptr(count), hyps, 0.02, 0.9, 2, 1,
        _ptr(tr), _ptr(inl), _ptr(num), _ptr(best), scores, _ptr(status), _ptr(ws), ws.numel(),
        stream), "rigid_ransac")


med, low = timed(raw)
print("pcr_rigid_ransac (C ABI): median %.3f ms  min %.3f ms  (%.0f pairs/s)"
      % (med, low, p / (med * 1e-3)))

c = 64
f1 = torch.randn((p, c, n), device=dev, generator=gen)
f2 = torch.randn((p, c, n), device=dev, generator=gen)
outs = [torch.empty((p, n), **i32) for _ in range(4)] + [torch.empty((p,), **i32)]
mws = torch.empty(lib.pcr_mutual_nn_workspace_size(p, n, n), dtype=torch.uint8, device=dev)
med, low = timed(lambda: _lib.check(lib.pcr_mutual_nn_match_cm(
    _ptr(f1), _ptr(f2), p, n, n, c, *[_ptr(o) for o in outs], _ptr(mws), mws.numel(), stream),
    "match"))
print("pcr_mutual_nn_match_cm (C = %d): median %.3f ms  min %.3f ms" % (c, med, low))
