#!/usr/bin/env python3
"""bench.py -- north-star metric of BASELINE.json:
point-clouds/sec (1024 pts, k=32) PPF + sph-vox forward at 1/2/4/8 MI355X.

Workloads (one "step" = one pass of the hot path over one batch of synthetic
clouds already resident in HBM):

  extract (default, BASELINE c2) -- the sph-dg extractor forward
      (pcr_amd.extractor.SphExtractor): self-KNN k=32 + local PPF, spherical
      normalisation + voxelisation (dense [B,C,r^3] grid, ind, cnt),
      spherical devoxelisation of that grid and the per-cloud descriptor;
      32 clouds x 1024 points, r=32, C=64 per GPU.
  pairs (BASELINE c4) -- registration pairs: the same forward over 128
      source + 128 target clouds per GPU, on-rank mutual-NN matching of each
      pair's devox features, descriptor all-gather across ranks.
  c3 (BASELINE c3) -- the path's share of the classify train step: 256 x
      2048 points, extractor forward + spherical devox backward + spherical
      vox backward (the gradient chain the reference runs with atomics).
  c5 (BASELINE c5) -- dense-scan stress: 8 x 65,536 points, k=64, r=64:
      KNN + local PPF, normalisation, sph voxelize, sph devoxelize.

Multi-GPU: one process per GPU (torch.distributed, RCCL), weak scaling:
every rank runs its own batch; the only collective is the per-call
descriptor all-gather (pcr_amd.distributed.DescriptorPipeline, side
stream), for extract / pairs.  `--gpus N` without torchrun's environment
starts N ranks itself (torch.distributed.run as a child process; this
parent never touches the GPU) and fails when fewer than N GPUs are visible.

Prints ONE JSON line (rank 0).  `roofline` is step level: the workload's
algorithmic bytes (DESIGN.md 4 for the backward terms) over
ms_per_step against the 8 TB/s HBM peak.

A plain run does what that line's `value` / `ms_per_step` need: set-up, the
settle calls, the warm-up and the timed steps.  `--full` adds the rest: the
output check before the warm-up (`outputs_verified`), `roofline.kernel`,
which prices the dominant kernel from its in-step duration (HIP events on
the stream it runs on), and `cpu_baseline`, which times the CPU restatement
(oracle/, the "port") on a bounded sample of the same workload on the host
cores.  `--dump-outputs DIR` writes the last timed step's outputs as .npy.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "point-cloud-registration-based-on-rotation-invariant-feature_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md chip table)
VALU_PEAK_TFLOPS = 157.3   # MI355X fp32 vector peak (packed FMA), SURVEY.md 8d
METRIC = "point-clouds/sec (1024 pts, k=32) PPF+sph-vox forward"
DUMP_BYTES = 60 * 1000 * 1000  # --dump-outputs writes at most this much array data

DEFAULTS = {  # workload: (clouds per GPU, points, k, r, channels)
    "extract": (32, 1024, 32, 32, 64),
    "pairs": (256, 1024, 32, 32, 64),
    "c3": (256, 2048, 32, 32, 64),
    "c5": (8, 65536, 64, 64, 64),
}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps (default 200 extract / pairs, 20 c3, 10 c5)")
    ap.add_argument("--warmup", type=int, default=None,
                    help="untimed warm-up steps (default 40 extract / pairs, 3 c3 / c5)")
    ap.add_argument("--workload", choices=tuple(DEFAULTS), default="extract")
    ap.add_argument("--batch", type=int, default=None, help="clouds per GPU")
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--res", type=int, default=None)
    ap.add_argument("--channels", type=int, default=None)
    ap.add_argument("--kernel-iters", type=int, default=50, help="(kept for old command lines)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--schedule", type=int, choices=(6, 7), default=None,
                    help="pcr_extractor_run schedule (include/pcr_amd.h): 6 = two "
                         "independent pipelines per chain (voxel chain on s_vox / origin, KNN "
                         "chain on s_nbr / s_pre by step parity), no cross-queue events, 7 = as 6 "
                         "with three voxel queues (s_vox / origin / s_pre) and one KNN queue; default 6")
    ap.add_argument("--no-kernel-timing", action="store_true",
                    help="diagnostic: no timing events around the dominant kernel")
    ap.add_argument("--settle-ms", type=float, default=50.0,
                    help="untimed calls of the timed call's shape (min(steps, "
                         "steps-per-launch) steps each, synchronized) for at least this long "
                         "after the output check and before the warm-up: a short timed region "
                         "right after the GPU idled measures its ramp, not the steady state "
                         "(DESIGN.md 4.9, scripts/first_call_probe.py); 0 = off")
    ap.add_argument("--no-verify", action="store_true",
                    help="diagnostic: skip the output check before the warm-up")
    ap.add_argument("--c3-schedule", choices=("pipelined", "pipelined-nbr", "serial"),
                    default="pipelined",
                    help="c3: pipelined = each batch's KNN + local PPF and its voxel head "
                         "(prep + means + devox) on side streams one batch ahead, overlapping "
                         "the previous step's grid stream and backwards "
                         "(SphExtractor.pipelined_steps(voxel_ahead=True)); pipelined-nbr = "
                         "only the KNN + PPF ahead (round 5's schedule); serial = forward "
                         "(joined), then the backwards")
    ap.add_argument("--cu-split", type=float, default=0.0,
                    help="extract diagnostic: the KNN queues on this fraction of the CUs, the "
                         "voxel queues (s_vox and the caller's stream) on the rest (CU-masked "
                         "HIP streams); 0 = off")
    ap.add_argument("--c3-cu-split", type=float, default=0.0,
                    help="c3 diagnostic: run the neighbour stream on this fraction of the CUs "
                         "and the caller's chain on the rest (CU-masked HIP streams); 0 = off")
    ap.add_argument("--steps-per-launch", type=int, default=200,
                    help="most pipelined steps per native runner call (extract / pairs); "
                         "--steps and --warmup are split into calls of at most this many "
                         "(each call ends in a join of the runner's queues, so its pipeline "
                         "drains: 200 steps as one call 442-447k against 427-431k clouds/s "
                         "as five of 40, profiles/r06_steps_per_launch.log)")
    ap.add_argument("--batches", type=int, default=None,
                    help="distinct input batches cycled through the timed steps (extract / "
                         "pairs: the runner's batch ring, each batch with its own output set; "
                         "default 20 extract, 8 pairs, 4 c3)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the output check "
                         "before the warm-up, the timing events around the dominant kernel "
                         "(roofline.kernel, roofline.traffic) and the CPU baseline after the "
                         "timed steps (each can still be switched off with its --no-* flag); "
                         "without --full a run sets up, settles, warms up, times the steps "
                         "and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last timed step "
                         "(the arrays a caller of the timed path receives) as DIR/<name>.npy, "
                         "float32 (float64 where an integer output does not fit float32); an "
                         "output of more than DUMP_BYTES / 8 / (number of outputs) elements is "
                         "written as a fixed, seeded sample of that many of its elements")
    args = ap.parse_args(argv)
    if not args.full:
        args.no_verify = args.no_kernel_timing = args.no_cpu_baseline = True
    b, n, k, r, c = DEFAULTS[args.workload]
    args.batch = b if args.batch is None else args.batch
    args.points = n if args.points is None else args.points
    args.k = k if args.k is None else args.k
    args.res = r if args.res is None else args.res
    args.channels = c if args.channels is None else args.channels
    heavy = args.workload in ("c3", "c5")
    if args.steps is None:
        args.steps = {"c3": 20, "c5": 10}.get(args.workload, 200)
    if args.warmup is None:
        args.warmup = 3 if heavy else 40
    if args.batches is None:
        args.batches = {"pairs": 8, "c3": 4}.get(args.workload, 20)
    if args.schedule is None:
        # extract: 381-395k with 6 against 305-319k with 7 (one KNN queue
        # is then the critical chain).  pairs: 7 while the matching was six
        # launches (250.5k vs 234.3k in round 4); with the norms in the tile
        # kernel 6 is ahead, 316.7-321.8k vs 313.4-314.9k (three interleaved
        # rounds, profiles/r06_pairs_schedule.log)
        args.schedule = 6
    if args.batches < 1:
        ap.error("--batches must be >= 1")
    if args.schedule >= 6 and args.batches < args.schedule - 4 and \
            args.workload in ("extract", "pairs"):
        ap.error("--schedule %d needs --batches >= %d (consecutive steps write distinct sets)"
                 % (args.schedule, args.schedule - 4))
    if args.workload == "pairs" and args.batch % 2:
        ap.error("--workload pairs needs an even --batch (source + target clouds)")
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    return args


# ------------------------------------------------------------ rank launch
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args, argv):
    """--gpus N outside torchrun: start N ranks with torch.distributed.run as
    a child process and return its exit code.  Only torch.cuda.device_count()
    is called here (it does not initialise the GPU on this image)."""
    visible = torch.cuda.device_count()
    if visible < args.gpus:
        print("bench: --gpus %d needs %d GPUs, but %d %s visible to this process"
              % (args.gpus, args.gpus, visible, "is" if visible == 1 else "are"),
              file=sys.stderr, flush=True)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node=%d" % args.gpus, "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


# ------------------------------------------------------------ inputs
def synthetic_inputs(b, n, c, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    xyz = torch.randn((b, 3, n), generator=g, device=device)
    xyz = (xyz - xyz.mean(dim=2, keepdim=True)).contiguous()
    nrm = torch.randn((b, 3, n), generator=g, device=device)
    nrm = (nrm / nrm.norm(dim=1, keepdim=True)).contiguous()
    feat = (torch.rand((b, c, n), generator=g, device=device) * 2 - 1).contiguous()
    return xyz, nrm, feat


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return ""


def usable_cores():
    """Threads this process can really run: its CPU affinity, capped by the
    cgroup CPU quota when one is set (a container's share of the host)."""
    aff = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
        if q != "max":
            quota = max(1, int(-(-int(q) // int(p))))
            if quota < aff:
                return quota, "affinity %d CPUs, cgroup quota %d" % (aff, quota)
    except (OSError, ValueError):
        pass
    return aff, "affinity %d CPUs" % aff


def _rate(one_batch, clouds_per_batch, seconds, threads):
    """Clouds per second of one_batch() repeated for about `seconds`."""
    import oracle
    oracle.set_num_threads(threads)
    one_batch()  # warm (page-in, thread pool)
    done, t0 = 0, time.perf_counter()
    while True:
        one_batch()
        done += clouds_per_batch
        el = time.perf_counter() - t0
        if el >= seconds:
            return done / el, done, el


def cpu_baseline(args):
    """The CPU restatement (oracle/pcr_oracle.c, OpenMP across clouds) on a
    bounded sample of the workload, once on one thread and once on every
    core this process may run on; the all-core figure is `value`."""
    import numpy as np
    import oracle
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from clouds import gaussian_clouds
    n, c, k, r, wl = args.points, args.channels, args.k, args.res, args.workload
    cores, why = usable_cores()
    if wl == "c5":
        # the oracle's reference KNN is O(N^2) per cloud (~50 s for one
        # 65,536-point cloud on one core): the sample is every stage of the
        # step for the whole batch, except that the KNN runs for a fixed
        # subset of Q query points per cloud against the whole cloud; its
        # time is scaled by N / Q (every query scans all N candidates)
        b, q = args.batch, 1024
        xyz, nrm, feat = gaussian_clouds(b, n, seed=0, c=c)
        sub = np.ascontiguousarray(xyz[:, :, :q])

        def timed(threads):
            oracle.set_num_threads(threads)
            t0 = time.perf_counter()
            _, ki = oracle.knn_dir(sub, xyz, k)
            t_knn = (time.perf_counter() - t0) * (n / q)
            t0 = time.perf_counter()
            oracle.local_ppf(xyz, nrm, sub, np.ascontiguousarray(nrm[:, :, :q]), ki,
                             kmajor=True, relative=True)
            t_ppf = (time.perf_counter() - t0) * (n / q)
            t0 = time.perf_counter()
            nc = oracle.normalize_sph(xyz)
            grid, ind, _ = oracle.spherical_avg_voxelize_forward(feat, nc, r)
            oracle.spherical_trilinear_devoxelize_forward(r, nc, grid, ind)
            return t_knn + t_ppf + (time.perf_counter() - t0)

        t1 = timed(1)  # one thread runs the clouds one after another
        tn = timed(cores)
        return {"value": b / tn, "unit": "point-clouds/sec", "cores": cores, "kind": "port",
                "single_thread": {"value": b / t1, "cores": 1},
                "sample": "the whole c5 step for %d clouds (N=%d, k=%d, r=%d, C=%d) except "
                          "that KNN + local PPF ran for %d of the %d query points per cloud "
                          "(each query scans all N candidates) and were scaled by N/%d; "
                          "oracle/pcr_oracle.c, OpenMP over clouds, %s; %s"
                          % (b, n, k, r, c, q, n, q, cpu_model(), why)}
    b = min(args.batch, 32 if wl != "c3" else 8)
    xyz, nrm, feat = gaussian_clouds(b, n, seed=0, c=c)
    gy = np.random.default_rng(1).standard_normal((b, c, n)).astype(np.float32)

    def one_batch():
        _, ki = oracle.knn_dir(xyz, xyz, k)
        oracle.local_ppf(xyz, nrm, xyz, nrm, ki, kmajor=True, relative=True)
        nc = oracle.normalize_sph(xyz)
        grid, ind, cnt = oracle.spherical_avg_voxelize_forward(feat, nc, r)
        dv, di, dw = oracle.spherical_trilinear_devoxelize_forward(r, nc, grid, ind)
        dv.max(axis=2)
        if wl == "pairs":
            f = dv.transpose(0, 2, 1)
            oracle.mutual_nn(np.ascontiguousarray(f[:b // 2]), np.ascontiguousarray(f[b // 2:]))
        if wl == "c3":
            gg = oracle.devoxelize_backward(gy, di, dw, r, spherical=True)
            oracle.avg_voxelize_backward(gg, ind, cnt)

    r1, d1, e1 = _rate(one_batch, b, args.cpu_seconds / 2, 1)
    rn, dn, en = _rate(one_batch, b, args.cpu_seconds, cores)
    return {"value": rn, "unit": "point-clouds/sec", "cores": cores, "kind": "port",
            "single_thread": {"value": r1, "cores": 1},
            "sample": "batches of %d clouds (N=%d, k=%d, r=%d, C=%d%s): %d clouds in %.1f s on "
                      "1 thread, %d clouds in %.1f s on %d threads; oracle/pcr_oracle.c, "
                      "OpenMP over clouds, %s; %s"
                      % (b, n, k, r, c, ", forward + devox / vox backward" if wl == "c3" else "",
                         d1, e1, dn, en, cores, cpu_model(), why)}


# ------------------------------------------------------------ workloads
class ExtractWorkload:
    """BASELINE c2 (extract) / c4 (pairs): the native runner enqueues up to
    S pipelined steps per call over a ring of R distinct synthetic batches
    (step s reads batch (s mod R) and writes that batch's own output set, as
    the reference's loaders hand a fresh batch to every iteration:
    datasets/deepgmr_mn40.py:71-97); each call's descriptors are
    all-gathered across ranks by the product pipeline (pcr_amd.distributed)."""

    def __init__(self, args, dev, rank, world):
        from pcr_amd.extractor import SphExtractor, algorithmic_bytes_per_cloud, \
            stream_kernel_bytes_per_cloud
        self.args, self.dev, self.world = args, dev, world
        b, n, c, k, r = args.batch, args.points, args.channels, args.k, args.res
        self.b, self.c = b, c
        self.R = args.batches
        self.batches = [self._make_batch(args, dev, 1234 + 7919 * rank + i)
                        for i in range(self.R)]
        if args.workload == "pairs":
            from pcr_amd.registration import PairExtractor
            self.ex = PairExtractor(b // 2, n, c, k, r, device=dev)
        else:
            self.ex = SphExtractor(b, n, c, k, r, device=dev)
        self.origin = None
        if args.cu_split > 0:
            sx = self.ex.ex if args.workload == "pairs" else self.ex
            sx.s_nbr, sx.s_pre, sx.s_vox, self.origin = cu_masked_streams(args.cu_split, dev, 2)
        self.S = max(1, args.steps_per_launch)
        self.next_set = 0
        self.desc_steps = {}
        self.pipe = None
        if world > 1:
            from pcr_amd.distributed import DescriptorPipeline
            self.pipe = DescriptorPipeline([b] * world, c, self.S, dev)
        self.step_bytes = algorithmic_bytes_per_cloud(n, k, r, c)["total"] * b
        if args.workload == "pairs":
            # matching: both clouds' [C, N] features read, corr12 / corr21 /
            # idx1 / idx2 written (4 x 4N), per pair
            self.step_bytes += (2 * 4 * c * n + 16 * n) * (b // 2)
        # the grid stream also writes devox + descriptor at c2-sized clouds
        # (pcr_extractor_voxel_stream_devox; pairs too since round 6)
        from pcr_amd import _lib
        self.stream_devox = bool(_lib.load().pcr_extractor_stream_devox_ok(n, c, r))
        self.kernel_bytes = stream_kernel_bytes_per_cloud(
            r, c, n if self.stream_devox else None) * b
        # grid launches bracketed with timing events in the timed call (each
        # event record on the grid queue costs ~3.5 us: 10 of 20 steps timed
        # made the driver's 20-step line 3.5% slower than untimed)
        self.KTIMED = 4

    @staticmethod
    def _make_batch(args, dev, seed):
        b, n, c = args.batch, args.points, args.channels
        xyz, nrm, feat = synthetic_inputs(b, n, c, dev, seed=seed)
        if args.workload == "pairs":
            # targets = sources rotated by a fixed rotation and permuted
            g = torch.Generator().manual_seed(seed)
            rot = torch.linalg.qr(torch.randn(3, 3, generator=g))[0].to(dev)
            perm = torch.randperm(n, generator=g).to(dev)
            p = b // 2
            xyz[p:] = torch.einsum("ij,bjn->bin", rot, xyz[:p])[:, :, perm]
            nrm[p:] = torch.einsum("ij,bjn->bin", rot, nrm[:p])[:, :, perm]
            feat[p:] = feat[:p][:, :, perm]
        return xyz.contiguous(), nrm.contiguous(), feat.contiguous()

    def chunks(self, total):
        from pcr_amd.distributed import step_chunks
        return step_chunks(total, self.S)

    def verify(self):
        """One runner call of R steps over the ring, every ring output
        poisoned first; then each step's outputs (knn_idx, local_ppf, ind,
        cnt, grid, devox, desc, and the pair matching) must equal one
        forward() of that step's batch."""
        args = self.args
        pairs = args.workload == "pairs"
        sx = self.ex.ex if pairs else self.ex
        ring = sx.ring_outputs(self.R, self.ex.pairs if pairs else 0)
        for o in ring:
            for t in o.values():
                t.view(-1).view(torch.uint8).fill_(0xFF)
        self.ex.run_ring(self.batches, self.R, 0, None, schedule=args.schedule)
        torch.cuda.synchronize(self.dev)
        keys = ("knn_idx", "local_ppf", "ind", "cnt", "grid", "devox", "desc")
        if pairs:
            keys += ("corr12", "corr21", "idx1", "idx2", "count")
        for i, (xyz, nrm, feat) in enumerate(self.batches):
            ref = self.ex.forward(xyz, nrm, feat)
            for key in keys:
                got = ring[i][key]
                if not torch.equal(got, ref[key]) and not torch.allclose(
                        got, ref[key], equal_nan=True):
                    raise SystemExit("bench: runner output %s of batch %d differs from the "
                                     "single-step path" % (key, i))
        return True

    def prepare_timing(self):
        if not self.args.no_kernel_timing:
            # the runner's timing events exist before the timed region
            # (creating them synchronises the device)
            self.ex.reserve_timing(self.KTIMED)

    def run(self, steps, timed):
        """`steps` steps over the batch ring, continuing the cycle across
        calls; timed: the last call brackets the grid kernel of KTIMED
        steps in its middle (pipeline full) with HIP events on its stream
        (in-step durations)."""
        from pcr_amd.distributed import run_pipelined
        ncalls = len(self.chunks(steps))

        def launch(i, m):
            if m not in self.desc_steps:
                self.desc_steps[m] = torch.empty((m, self.b, self.c), device=self.dev)
            tk = self.KTIMED if (timed and i == ncalls - 1 and
                                 not self.args.no_kernel_timing) else False
            self.ex.run_ring(self.batches, m, self.next_set, self.desc_steps[m],
                             schedule=self.args.schedule, timed=tk)
            self.next_set = (self.next_set + m) % self.R
            return self.desc_steps[m]

        if self.origin is None:
            return run_pipelined(steps, self.S, launch, self.pipe)
        self.origin.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.origin):
            out = run_pipelined(steps, self.S, launch, self.pipe)
        torch.cuda.current_stream(self.dev).wait_stream(self.origin)
        return out

    def last_outputs(self):
        """The ring set the last step wrote (run() leaves next_set one past it)."""
        pairs = self.args.workload == "pairs"
        sx = self.ex.ex if pairs else self.ex
        ring = sx.ring_outputs(self.R, self.ex.pairs if pairs else 0)
        return dict(ring[(self.next_set - 1) % self.R])

    def kernel_report(self):
        ms = self.ex.grid_kernel_times()
        avg = sum(ms) / len(ms) if ms else float("nan")
        gbs = self.kernel_bytes / (avg * 1e-3) / 1e9
        traffic = step_traffic = None
        a = self.args
        pmc_path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(pmc_path):
            try:
                with open(pmc_path) as f:
                    pm = json.load(f)
                if pm.get("config") == [a.batch, a.points, a.k, a.res, a.channels]:
                    traffic = pm.get("grid_kernel_hbm_bytes_per_launch")
                    step_traffic = pm.get("step_hbm_bytes")
            except (OSError, ValueError):
                pass
        return step_traffic, {
            "name": ("vox_stream_kernel (sph-vox dense grid + cnt from the voxel means, and "
                     "the sph devox + descriptor of the same means)" if self.stream_devox else
                     "vox_stream_kernel (sph-vox dense grid + cnt from the voxel means)"),
            "bound": "hbm", "avg_ms_in_step": round(avg, 5), "launches_timed": len(ms),
            "bytes_per_launch": self.kernel_bytes, "achieved": round(gbs, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
            "traffic": traffic}

    def config(self):
        a = self.args
        b, n, k, r, c = a.batch, a.points, a.k, a.res, a.channels
        wl = ("sph-dg extractor forward: self-KNN k=%d + local PPF + sph-vox r=%d^3 + "
              "sph-devox + descriptor" % (k, r)) if a.workload == "extract" else \
            ("registration pairs (BASELINE c4): extractor forward over %d source + %d "
             "target clouds (self-KNN k=%d + local PPF + sph-vox r=%d^3 + sph-devox + "
             "descriptor), mutual-NN matching of each pair's devox features on-rank, "
             "descriptor all-gather" % (b // 2, b // 2, k, r))
        return {"workload": wl, "clouds_per_gpu": b,
                "pairs_per_gpu": b // 2 if a.workload == "pairs" else None,
                "points": n, "k": k, "resolution": r, "channels": c,
                "global_batch": b * self.world,
                "parallelism": "dp%d (clouds sharded, descriptor all-gather)" % self.world,
                "schedule": a.schedule,
                "cu_split": a.cu_split or None,
                "runner_calls": [len(self.chunks(a.warmup)), len(self.chunks(a.steps))],
                "steps_per_launch": self.S,
                "distinct_batches": self.R}


class C3Workload:
    """BASELINE c3: the path's share of the classify train step at 256 x
    2048 points.  One step = the extractor forward (SphExtractor.forward)
    + the backward of the spherical devoxelisation (a synthetic upstream
    gradient [B, C, N] -> gradient grid [B, C, r^3]) + the backward of the
    spherical voxelisation of that gradient grid (-> [B, C, N]).  Conv3d /
    MLP layers between them are outside the path."""

    def __init__(self, args, dev, rank, world):
        from pcr_amd import ops
        from pcr_amd.extractor import SphExtractor, algorithmic_bytes_per_cloud
        self.ops = ops
        self.args, self.dev, self.world = args, dev, world
        b, n, c, k, r = args.batch, args.points, args.channels, args.k, args.res
        # a ring of R distinct batches (and upstream gradients): step s
        # trains on batch s % R, as the reference's loader hands every step a
        # new batch (train.py:138-153)
        self.R = args.batches
        self.batches = [synthetic_inputs(b, n, c, dev, seed=1234 + 7919 * rank + i)
                        for i in range(self.R)]
        g = torch.Generator(device=dev).manual_seed(99 + rank)
        self.gys = [torch.randn((b, c, n), generator=g, device=dev) for _ in range(self.R)]
        self.ex = SphExtractor(b, n, c, k, r, device=dev)
        self.main_stream = None
        if args.c3_cu_split > 0:
            nbr, main = cu_masked_streams(args.c3_cu_split, dev)
            self.ex.s_nbr = nbr
            self.main_stream = main
        fwd = algorithmic_bytes_per_cloud(n, k, r, c)["total"]
        # devox backward: upstream gradient 4CN + corner inds / wgts 64N in,
        # the dense gradient grid 4C r^3 out (written once); vox backward:
        # ind 4N + the counts of the points' voxels 4N + the gradient rows of
        # the occupied voxels (<= 4CN) in, grad_x 4CN out
        self.devox_bwd_bytes = (4 * c * n + 64 * n + 4 * c * r ** 3) * b
        vox_bwd = 8 * n + 8 * c * n
        self.step_bytes = fwd * b + self.devox_bwd_bytes + vox_bwd * b
        self.t = []
        # the timed call keeps its last step's outputs (references only) for
        # last_outputs(); other calls keep none, so they free theirs as before
        self.keep_last, self.last = False, None

    def _backward(self, s, out, ev=None):
        """Step s's backward share: devox backward of its synthetic upstream
        gradient, then voxelize backward of the gradient grid."""
        ops = self.ops
        if ev is not None:
            ev[0].record()
        gg = ops.spherical_trilinear_devoxelize_backward(self.gys[s % self.R], out["dinds"],
                                                         out["dwgts"], self.args.res)
        if ev is not None:
            ev[1].record()
        gx = ops.spherical_avg_voxelize_backward(gg, out["ind"], out["cnt"])
        return gg, gx

    def _serial(self, steps, timed, keep=None, first=0):
        for s in range(first, first + steps):
            out = self.ex.forward(*self.batches[s % self.R])
            res = self._backward(s, out, self.ev[s - first] if timed else None)
            if keep is not None:
                keep.append((out, res))
            if self.keep_last and s == first + steps - 1:
                self.last = (out, res)

    def _pipelined(self, steps, timed, keep=None):
        def consume(s, out):
            res = self._backward(s, out, self.ev[s] if timed else None)
            if keep is not None:
                keep.append(({kk: v.clone() for kk, v in out.items()}, res))
            if self.keep_last and s == steps - 1:
                self.last = (out, res)
        # prefetch: batch(s + 1) before step s's voxel side and consume; the
        # bench's batch tensors are read-only, so that is allowed.  The voxel
        # head (prep + means + devox) of batch s + 1 runs ahead on a side
        # stream too, unless --c3-schedule pipelined-nbr
        self.ex.pipelined_steps(steps, lambda s: self.batches[s % self.R], consume,
                                select_events=self.sev if timed else None, prefetch=True,
                                voxel_ahead=self.args.c3_schedule == "pipelined")

    def verify(self):
        """Three pipelined steps (batches 0, 1, 2 of the ring) vs the serial
        forward + backwards of the third: every forward output of the last
        step and both backward results must be identical (outputs poisoned
        first)."""
        if self.args.c3_schedule == "serial":
            return None
        ref = []
        self._serial(1, False, ref, first=2)
        ref = ({kk: v.clone() for kk, v in ref[0][0].items()}, [t.clone() for t in ref[0][1]])
        for t in [self.ex.local_ppf, self.ex.knn_idx, self.ex.grid, self.ex.devox, self.ex.ind,
                  self.ex.cnt] + [self.ex._ppf(1), self.ex._set(1)[4]]:
            t.view(-1).view(torch.uint8).fill_(0xFF)
        got = []
        self._pipelined(3, False, got)
        torch.cuda.synchronize(self.dev)
        out, res = got[-1]
        for key in ("knn_idx", "local_ppf", "ind", "cnt", "grid", "devox", "desc"):
            if not torch.equal(out[key], ref[0][key]) and not torch.allclose(
                    out[key], ref[0][key], equal_nan=True):
                raise SystemExit("bench: pipelined c3 output %s differs from the serial path"
                                 % key)
        # the backwards are atomics-free gathers: bit-identical run to run
        for name, a, b in zip(("devox backward", "vox backward"), res, ref[1]):
            if not torch.equal(a, b):
                raise SystemExit("bench: pipelined c3 %s differs from the serial path" % name)
        return True

    def prepare_timing(self):
        self.ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(self.args.steps)]
        # the KNN selection launch of every step, on the neighbour stream
        self.sev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    for _ in range(self.args.steps)]

    def run(self, steps, timed):
        # the extractor's stage kernels from Python (pipelined: the split
        # voxel stage -- means + devox, then the dense-grid stream -- on the
        # caller's stream, KNN + PPF one batch ahead on s_nbr)
        t = timed and not self.args.no_kernel_timing
        self.keep_last = timed
        if self.main_stream is not None:
            self.main_stream.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(self.main_stream):
                if self.args.c3_schedule == "serial":
                    self._serial(steps, t)
                else:
                    self._pipelined(steps, t)
            torch.cuda.current_stream(self.dev).wait_stream(self.main_stream)
        elif self.args.c3_schedule == "serial":
            self._serial(steps, t)
        else:
            self._pipelined(steps, t)
        self.keep_last = False
        self.timed_steps = steps if timed else 0
        return steps

    def last_outputs(self):
        """The last timed step's forward outputs and its two backward results."""
        out, (gg, gx) = self.last
        return dict(out, grad_grid=gg, grad_x=gx)

    def kernel_report(self):
        """The step's dominant kernel by in-step duration (HIP events on the
        stream each runs on): the KNN selection (VALU, priced at the
        brute-force-equivalent 9 N^2 fp32 operations per cloud, SURVEY.md
        8d) or the spherical devox backward (HBM); the other one is listed
        beside it."""
        a = self.args
        if a.no_kernel_timing:
            return None, None
        ms = [x.elapsed_time(y) for x, y in self.ev[:self.timed_steps]]
        avg = sum(ms) / len(ms) if ms else float("nan")
        gbs = self.devox_bwd_bytes / (avg * 1e-3) / 1e9
        devox = {
            "name": "spherical devoxelize backward (pcr_devoxelize_backward_ws: corner-set "
                    "order + gather, dense gradient grid written once)",
            "bound": "hbm", "avg_ms_in_step": round(avg, 5), "launches_timed": len(ms),
            "bytes_per_launch": self.devox_bwd_bytes, "achieved": round(gbs, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
            "traffic": None}
        sms = [x.elapsed_time(y) for x, y in self.sev[:self.timed_steps]]
        if c3_selection_timed(sms):
            savg = sum(sms) / len(sms)
            ops = 9.0 * a.points * a.points * a.batch
            tf = ops / (savg * 1e-3) / 1e12
            sel = {"name": "knn_select_kernel (threshold selection, k=%d, %d-point LDS-cached "
                           "candidates; pcr_knn_select_sorted)" % (a.k, a.points),
                   "bound": "valu", "avg_ms_in_step": round(savg, 5),
                   "launches_timed": len(sms), "fp32_ops_per_launch": ops,
                   "ops_model": "brute-force-equivalent 9 N^2 per cloud (SURVEY.md 8d)",
                   "achieved": round(tf, 3), "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                   "frac": round(tf / VALU_PEAK_TFLOPS, 4), "traffic": None}
            if savg >= avg:
                sel["other_kernels"] = [devox]
                return None, sel
            devox["other_kernels"] = [sel]
        return None, devox

    def config(self):
        a = self.args
        return {"workload": "BASELINE c3 train step, hot-path share: extractor forward "
                            "(self-KNN k=%d + local PPF + sph-vox r=%d^3 + sph-devox + "
                            "descriptor) + sph devox backward + sph vox backward"
                            % (a.k, a.res),
                "clouds_per_gpu": a.batch, "points": a.points, "k": a.k,
                "resolution": a.res, "channels": a.channels,
                "global_batch": a.batch * self.world,
                "parallelism": "dp%d (clouds sharded, no collective)" % self.world,
                "schedule": a.c3_schedule, "distinct_batches": self.R,
                "cu_split": a.c3_cu_split or None}


def c3_selection_timed(ms):
    """True when the selection events of the timed steps were recorded (the
    sorted-rows path ran; other shapes fall back without them)."""
    return bool(ms) and all(t > 0 for t in ms)


def cu_masked_streams(frac, dev, copies=1):
    """HIP streams on complementary CU masks (pcr_stream_create_cu_mask):
    `frac` of every 8 consecutive CU bits for the first `copies` streams, the
    rest for the next `copies`.  Returns torch ExternalStreams (diagnostic;
    the streams live for the process)."""
    import ctypes
    from pcr_amd import _lib
    lib = _lib.load()
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    words = (ncu + 31) // 32
    take = max(1, min(7, int(round(frac * 8))))
    a = (ctypes.c_uint32 * words)()
    bm = (ctypes.c_uint32 * words)()
    for cu in range(ncu):
        if cu % 8 < take:
            a[cu // 32] |= 1 << (cu % 32)
        else:
            bm[cu // 32] |= 1 << (cu % 32)
    out = []
    for mask in (a, bm):
        for _ in range(copies):
            st = ctypes.c_void_p()
            _lib.check(lib.pcr_stream_create_cu_mask(mask, words, ctypes.byref(st)),
                       "stream_create_cu_mask")
            out.append(torch.cuda.ExternalStream(st.value, device=dev))
    return out


class C5Workload:
    """BASELINE c5: 8 x 65,536 points, k=64, r=64 -- self-KNN + local PPF,
    spherical normalisation, voxelisation and devoxelisation, each through
    the torch-level op (ops.*): the neighbour branch on the current stream,
    the voxel branch on a side stream beside it."""

    def __init__(self, args, dev, rank, world):
        from pcr_amd import ops
        from pcr_amd.extractor import algorithmic_bytes_per_cloud
        self.ops = ops
        self.args, self.dev, self.world = args, dev, world
        b, n, c, k, r = args.batch, args.points, args.channels, args.k, args.res
        self.inputs = synthetic_inputs(b, n, c, dev, seed=1234 + rank)
        ab = algorithmic_bytes_per_cloud(n, k, r, c)
        self.step_bytes = ab["total"] * b
        # the KNN + local PPF launch: SURVEY.md 8d algorithmic bytes (inputs
        # read once, idx + ppf written once); the brute-force-equivalent
        # 9 N^2 fp32 ops per cloud are reported beside it, not as the bound:
        # the pruned selection does a small fraction of them
        self.knn_bytes = (ab["knn"] + ab["local_ppf"]) * b
        self.knn_ops = 9.0 * n * n * b
        self.side = torch.cuda.Stream(device=dev)

    def _step_outputs(self):
        ops, a = self.ops, self.args
        xyz, nrm, feat = self.inputs
        nc = ops.spherical_normalize(xyz)
        grid, ind, cnt = ops.spherical_avg_voxelize_forward(feat, nc, a.res)
        dv = ops.spherical_trilinear_devoxelize_forward(a.res, True, nc, grid, ind)
        idx, ppf, _ = ops.knn_local_ppf(xyz, nrm, a.k)
        return {"norm_coords": nc, "grid": grid, "ind": ind, "cnt": cnt, "devox": dv[0],
                "knn_idx": idx, "local_ppf": ppf}

    def verify(self):
        """The c5 step's outputs, checked on the GPU (the CPU oracle takes
        minutes at this size; tests/test_gpu_large.py holds the sampled
        oracle checks): two runs of the step are bit-identical; for 64
        sampled queries per cloud the k neighbours are the k nearest by a
        float64 brute force (each within 1e-5 relative of the float64 k-th
        distance, slot 0 at distance 0), their PPF distance channel is the
        float64 |2c - p| within 1e-5; every point with a voxel is counted in
        cnt, and the grid holds the float64 mean of its voxel's features
        within 1e-5 at 64 sampled occupied voxels per cloud."""
        a = self.args
        b, n, k, r3 = a.batch, a.points, a.k, a.res ** 3
        first = {kk: v.clone() for kk, v in self._step_outputs().items()}
        again = self._step_outputs()
        torch.cuda.synchronize(self.dev)
        for key, v in first.items():
            if not torch.equal(v.view(torch.int32), again[key].view(torch.int32)):
                raise SystemExit("bench: c5 output %s differs between two runs" % key)
        xyz, _, feat = self.inputs
        g = torch.Generator(device=self.dev).manual_seed(7)
        qi = torch.randint(0, n, (b, 64), generator=g, device=self.dev)
        idx, ppf = first["knn_idx"].long(), first["local_ppf"]
        for c in range(b):
            X = xyz[c].double()
            D = ((X[:, None, :] - X[:, qi[c]][:, :, None]) ** 2).sum(0)  # [64, n]
            kth = D.topk(k, largest=False).values[:, -1]
            sel = idx[c][:, qi[c]].t()  # [64, k]
            ds = D.gather(1, sel)
            dn = ppf[c, 3][:, qi[c]].t().double()
            # the PPF distance channel: |c - (p - c)| with the reference's
            # relative neighbour coordinates (pvcnn_classify.py:252-262)
            gq = 2.0 * X[:, qi[c]][:, :, None] - X[:, sel]  # [3, 64, k]
            de = (gq ** 2).sum(0).sqrt()
            checks = {
                "ids in range": bool(((sel >= 0) & (sel < n)).all()),
                "k nearest": bool((ds <= kth[:, None] * (1 + 1e-5) + 1e-12).all()),
                "slot 0 at distance 0": bool((ds[:, 0] == 0).all()),
                "ids distinct": bool((sel.sort(1).values.diff(dim=1) > 0).all()),
                "PPF distance": bool(((dn - de).abs() <= 1e-5 * de + 1e-6).all())}
            bad = [name for name, v in checks.items() if not v]
            if bad:
                raise SystemExit("bench: c5 KNN / PPF of cloud %d fail the float64 check: %s"
                                 % (c, ", ".join(bad)))
            ind, cnt = first["ind"][c].long(), first["cnt"][c].long()
            valid = ind >= 0
            if int(cnt.sum()) != int(valid.sum()) or not torch.equal(
                    torch.bincount(ind[valid], minlength=r3), cnt):
                raise SystemExit("bench: c5 cnt of cloud %d does not count ind" % c)
            occ = torch.nonzero(cnt > 0).flatten()
            vs = occ[torch.randint(0, occ.numel(), (64,), generator=g, device=self.dev)]
            for v in vs.tolist():
                pts = torch.nonzero(ind == v).flatten()
                mean = feat[c][:, pts].double().mean(1)
                got = first["grid"][c][:, v].double()
                if not bool(((got - mean).abs() <= 1e-5 * mean.abs() + 1e-6).all()):
                    raise SystemExit("bench: c5 grid voxel %d of cloud %d is not its mean"
                                     % (v, c))
        return True

    def prepare_timing(self):
        self.ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(self.args.steps)]

    def run(self, steps, timed):
        ops, a = self.ops, self.args
        xyz, nrm, feat = self.inputs
        cur = torch.cuda.current_stream(self.dev)
        for s in range(steps):
            # the voxel branch (normalise -> voxelize -> devoxelize) does not
            # depend on the neighbour branch (KNN + PPF): it runs on a side
            # stream beside it, so its HBM-bound sorted voxelisation overlaps
            # the latency-bound selection; joined before the next step
            self.side.wait_stream(cur)
            with torch.cuda.stream(self.side):
                nc = ops.spherical_normalize(xyz)
                grid, ind, cnt = ops.spherical_avg_voxelize_forward(feat, nc, a.res)
                dv = ops.spherical_trilinear_devoxelize_forward(a.res, True, nc, grid, ind)
            if timed and not a.no_kernel_timing:
                self.ev[s][0].record()
            nb = ops.knn_local_ppf(xyz, nrm, a.k)
            if timed and not a.no_kernel_timing:
                self.ev[s][1].record()
            cur.wait_stream(self.side)
            if timed and s == steps - 1:
                # references only, for last_outputs(); made on the side
                # stream, read after the synchronize that ends the timed region
                self.last = {"norm_coords": nc, "grid": grid, "ind": ind, "cnt": cnt,
                             "devox": dv[0], "dinds": dv[1], "dwgts": dv[2],
                             "knn_idx": nb[0], "local_ppf": nb[1]}
            del dv, nb  # every other step frees them here, as before
        self.timed_steps = steps if timed else 0
        return steps

    def last_outputs(self):
        return self.last

    def kernel_report(self):
        ms = [x.elapsed_time(y) for x, y in self.ev[:self.timed_steps]] \
            if not self.args.no_kernel_timing else []
        avg = sum(ms) / len(ms) if ms else float("nan")
        tf = self.knn_ops / (avg * 1e-3) / 1e12
        gbs = self.knn_bytes / (avg * 1e-3) / 1e9
        return None, {
            "name": "self-KNN k=%d + local PPF (Morton sort + threshold selection into "
                    "sorted-order keys + un-permuting PPF emit)" % self.args.k,
            "bound": "hbm", "avg_ms_in_step": round(avg, 4), "launches_timed": len(ms),
            "bytes_per_launch": self.knn_bytes, "achieved": round(gbs, 1),
            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
            "traffic": None,
            "brute_force_equivalent": {"fp32_ops_per_launch": self.knn_ops,
                                       "tflops": round(tf, 2)}}

    def config(self):
        a = self.args
        return {"workload": "BASELINE c5 dense-scan stress: self-KNN k=%d + local PPF + "
                            "sph normalise + sph-vox r=%d^3 + sph-devox" % (a.k, a.res),
                "clouds_per_gpu": a.batch, "points": a.points, "k": a.k,
                "resolution": a.res, "channels": a.channels,
                "global_batch": a.batch * self.world,
                "parallelism": "dp%d (clouds sharded, no collective)" % self.world}


WORKLOADS = {"extract": ExtractWorkload, "pairs": ExtractWorkload, "c3": C3Workload,
             "c5": C5Workload}


def settle_runs(wl, args, dev):
    """Untimed runner calls of the timed call's shape, each synchronized as
    the timed one is, for at least --settle-ms: after the output check the
    GPU has idled, and the first short calls after an idle run 3-5% slower
    than the same call repeated (20-step c2 calls: 1.55-1.64 ms for the
    first, 1.48-1.51 ms from the fourth on; an idle of 0.5 s brings the slow
    calls back; scripts/first_call_probe.py).  The W warm-up steps and the
    K timed steps are unchanged."""
    if args.settle_ms <= 0:
        return None
    m = min(args.steps, args.steps_per_launch) if args.workload in ("extract", "pairs") \
        else args.steps
    m = max(1, m)
    t0 = time.perf_counter()
    if args.no_verify:
        # no output check ran, so the process's first call pays the one-off
        # costs (code objects loaded, buffers made: ~13 ms against ~1.5 ms
        # for a 20-step c2 call); the call that sizes `calls` comes after it
        wl.run(m, timed=False)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
    wl.run(m, timed=False)
    torch.cuda.synchronize(dev)
    # the same number of calls on every rank (the calls all-gather)
    calls = max(1, math.ceil(args.settle_ms / ((time.perf_counter() - t0) * 1e3)))
    if dist.is_available() and dist.is_initialized():
        t = torch.tensor([calls], dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        calls = int(t.item())
    for _ in range(calls - 1):
        wl.run(m, timed=False)
        torch.cuda.synchronize(dev)
    return {"ms": round((time.perf_counter() - t0) * 1e3, 1), "calls": calls,
            "steps_per_call": m}


def dump_outputs(outputs, path):
    """Write {name: tensor} as path/<name>.npy, float32 (float64 for an
    integer tensor whose values do not all fit float32's 24 bits).  At most
    DUMP_BYTES in all: a tensor of more than cap = DUMP_BYTES / 8 / len(outputs)
    elements is written as its elements at cap flat positions drawn once
    from a fixed seed (the same positions for the same shape in every run)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    cap = DUMP_BYTES // 8 // max(1, len(outputs))
    for name in sorted(outputs):
        t = outputs[name].detach()
        if t.numel() > cap:
            pos = np.sort(np.random.default_rng(20240).integers(0, t.numel(), cap))
            t = t.reshape(-1)[torch.from_numpy(pos).to(t.device)]
        if t.is_floating_point() or t.numel() == 0 or int(t.abs().max()) < 1 << 24:
            t = t.to(torch.float32)
        else:
            t = t.to(torch.float64)
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args, argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print("bench: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world), file=sys.stderr)
        return 2
    if local_rank >= torch.cuda.device_count():
        print("bench: local rank %d has no GPU (%d visible)" % (local_rank,
                                                                 torch.cuda.device_count()),
              file=sys.stderr)
        return 2
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)

    wl = WORKLOADS[args.workload](args, dev, rank, world)
    wl.prepare_timing()
    # before the warm-up, outside the timed region: the outputs are checked
    # (extract / pairs: runner vs single-step path, every output poisoned
    # first), which also brings the GPU up to clock
    verified = False if args.no_verify else wl.verify()
    settle = settle_runs(wl, args, dev)
    wl.run(args.warmup, timed=False)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    calls = wl.run(args.steps, timed=True)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0 and args.dump_outputs:
        dump_outputs(wl.last_outputs(), args.dump_outputs)
    step_traffic, kernel = wl.kernel_report() if args.full else (None, None)
    value = args.batch * world * args.steps / elapsed
    # per rank: every rank moves its own HBM
    step_gbs = wl.step_bytes * args.steps / elapsed / 1e9
    if isinstance(kernel, dict) and kernel.get("bytes_per_launch") and \
            args.workload in ("extract", "pairs"):
        # one launch of the dominant kernel per step, two in flight under
        # the runner's schedules: its bytes over the step time is the rate
        # the step sustains for it (achieved / frac).  avg_ms_in_step is the
        # latency of one launch, which the overlap stretches: not a rate.
        agg = kernel["bytes_per_launch"] / (elapsed / args.steps) / 1e9
        kernel["achieved"] = round(agg, 1)
        kernel["frac"] = round(agg / HBM_PEAK_GBS, 4)
        kernel["level"] = "bytes_per_launch / ms_per_step (one launch per step)"
    result = {
        "metric": METRIC if args.workload in ("extract", "pairs") else
        "point-clouds/sec (%d pts, k=%d) %s" % (args.points, args.k,
                                                "forward+backward hot path (c3)"
                                                if args.workload == "c3" else
                                                "KNN+PPF+sph-vox+devox (c5)"),
        "value": round(value, 1),
        "unit": "point-clouds/sec",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic (seeded gaussian clouds, unit normals, U(-1,1) features)",
        "outputs_verified": verified,
        "settle": settle,
        "config": wl.config(),
        "roofline": {"bound": "hbm", "achieved": round(step_gbs, 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(step_gbs / HBM_PEAK_GBS, 4),
                     "traffic": step_traffic,
                     "level": "step: %d B/cloud x %d clouds per rank / ms_per_step"
                              % (wl.step_bytes // args.batch, args.batch),
                     "kernel": kernel},
    }
    if rank == 0 and not args.no_cpu_baseline:
        # after the timed region, on rank 0's host cores, at every N (the
        # other ranks wait at the barrier below)
        result["cpu_baseline"] = cpu_baseline(args)
    elif rank == 0:
        result["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
