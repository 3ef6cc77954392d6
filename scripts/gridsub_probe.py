"""HIP-event time per call of the grid subsampling (ops.grid_subsample,
DESIGN.md 4.8e) on raw-scan shapes -- 8 clouds x 65,536 points at cell sizes
that leave about 1k, 4k and 16k cells, and 128 clouds x 4096 points -- without
features and with 32 feature channels.  Next to each, on the same GPU:
ops.furthest_point_sampling to the same output count (the only other reducer
here; it returns indices and averages nothing), and a torch composition
(per cloud: torch.unique(return_inverse=True) of the cell keys + index_add_,
whose float atomics do not fix the order of the sums).  The fraction of the
8 TB/s roofline is for the algorithmic bytes: (12 + 4 c) n in, the same out,
and 8 n for cell_of and cell_count, per cloud.  Diagnostic, not the bench.

  python scripts/gridsub_probe.py
  python scripts/gridsub_probe.py calls B N C CELL   # 20 calls of one shape and nothing else,
                                                     # for rocprofv3 --kernel-trace --stats
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
HBM = 8.0e12  # bytes per second, the datasheet figure


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


def torch_composition(xyz, cell, feat):
    """the same cells with stock torch ops, cloud by cloud"""
    outs = []
    for q in range(xyz.shape[0]):
        p = xyz[q]
        origin = torch.floor(p.min(dim=1, keepdim=True).values * (1.0 / cell)) * cell
        ijk = torch.clamp(torch.floor((p - origin) / cell), min=0).long()
        dims = ijk.max(dim=1).values + 1
        key = ijk[0] + dims[0] * (ijk[1] + dims[1] * ijk[2])
        uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
        rows = p if feat is None else torch.cat([p, feat[q]])
        acc = torch.zeros((rows.shape[0], uniq.numel()), device=dev)
        acc.index_add_(1, inv, rows)
        outs.append(acc / cnt)
    return outs


def case(b, n, cell, c):
    xyz = torch.rand((b, 3, n), device=dev, generator=gen).contiguous()
    feat = torch.randn((b, c, n), device=dev, generator=gen).contiguous() if c else None
    out = ops.grid_subsample(xyz, cell, feat)
    torch.cuda.synchronize()
    assert int((out["status"] != 0).sum()) == 0
    cells = out["count"]
    m = int(cells.max())
    ref = torch_composition(xyz, cell, feat)
    # the composition's sums are unordered, and torch's own rounding of the
    # quotient can put a point next to a face into the neighbouring cell:
    # close on the clouds where the cell counts agree, not equal
    same = [q for q in range(b) if ref[q].shape[1] == int(cells[q])]
    err = max([float((ref[q][:3] - out["xyz"][q, :, :int(cells[q])]).abs().max()) for q in same] +
              [0.0])
    med, low = timed(lambda: ops.grid_subsample(xyz, cell, feat))
    bytes_ = b * n * (2 * (12 + 4 * c) + 8)
    print("b=%d n=%d c=%d cell=%.4g: cells min %d max %d; ops.grid_subsample median %.3f ms min "
          "%.3f ms; %.1f MB algorithmic = %.2f %% of 8 TB/s at the median" % (
              b, n, c, cell, int(cells.min()), m, med, low, bytes_ / 1e6,
              100.0 * bytes_ / (med * 1e-3) / HBM))
    tmed, tlow = timed(lambda: torch_composition(xyz, cell, feat), warm=1, it=5)
    print("    torch unique + index_add_: median %.3f ms min %.3f ms (max |xyz difference| %.2g on "
          "the %d of %d clouds with the same number of cells)" % (tmed, tlow, err, len(same), b))
    if c == 0:
        fmed, flow = timed(lambda: ops.furthest_point_sampling(xyz, m), warm=1, it=3)
        print("    furthest_point_sampling to %d points: median %.3f ms min %.3f ms" % (
            m, fmed, flow))


if len(sys.argv) > 1 and sys.argv[1] == "calls":
    b_, n_, c_ = (int(a) for a in sys.argv[2:5])
    xyz_ = torch.rand((b_, 3, n_), device=dev, generator=gen).contiguous()
    feat_ = torch.randn((b_, c_, n_), device=dev, generator=gen).contiguous() if c_ else None
    for _ in range(20):
        ops.grid_subsample(xyz_, float(sys.argv[5]), feat_)
    torch.cuda.synchronize()
    sys.exit(0)

print("device: %s" % torch.cuda.get_device_name(0))
for c in (0, 32):
    for cell in (0.1, 1.0 / 16, 0.04):
        case(8, 65536, cell, c)
    case(128, 4096, 0.1, c)
