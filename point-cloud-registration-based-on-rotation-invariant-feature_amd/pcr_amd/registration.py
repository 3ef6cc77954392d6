"""Registration pairs on one rank (BASELINE c4).

The reference's registration evaluation extracts per-point features of the
source and the target cloud of every pair (datasets/deepgmr_mn40.py:71-97:
feat1 = model(pc1), feat2 = model(pc2)) and matches them by mutual nearest
neighbours in feature space (:232-244, find_correspondence_one_pair).  Here
one step of a rank's shard of P pairs is:

  * the extractor forward (pcr_amd.extractor.SphExtractor, the north-star
    hot path) over a batch of 2P clouds -- sources in [0, P), targets in
    [P, 2P) -- so both clouds of a pair live on the same rank;
  * the mutual-NN matching of each source's devoxelised per-point features
    [C, N] against its target's (pcr_mutual_nn_match_cm, fp32 MFMA), which
    needs no exchange because the pair is local;
  * the per-cloud descriptors [2P, C] of the step, all-gathered across ranks
    (pcr_amd.distributed.gather_descriptors, RCCL over xGMI) -- the only
    collective.

The correspondences become a rigid transform per pair on the device too
(ops.rigid_ransac: a seeded RANSAC + least-squares refit):
PairExtractor.register, or register_pairs for features from elsewhere;
rre_rte and alignment_rmse are the reference's error meters.  ops.icp (the
reference's func='icp' solver) re-fits a transform over every
point within a distance: icp_pairs on its own, or `icp=` of register /
register_pairs as the refinement of the RANSAC estimate;
icp=dict(estimation="point_to_plane") refines along the target's normals
instead, which register, fpfh_pairs and scan_pairs fill in
from the normals they hold.  ops.fgr (the
reference's func='fgr' solver) is the other estimate from the
correspondences: fgr_pairs, or solver="fgr" of register / register_pairs.
ops.teaser (the reference's func='teaserpp' solver with a bounded clique
search) is the one meant for mostly wrong matches:
teaser_pairs, or solver="teaser".  fpfh_pairs needs no extractor and no
weights: it computes FPFH descriptors (ops.fpfh) from the
points and normals of both clouds and hands them to register_pairs.
scan_pairs starts one step earlier, from lists of raw scans of any sizes:
grid subsampling, normals from the hybrid search's rows, then fpfh_pairs on
the ragged clouds, whose counts (counts1 / counts2) the
matching, FGR and ICP take.

The native runner (pcr_extractor_run with match_pairs = P) enqueues the
matching on each step's voxel queue right after its devox (behind the grid
stream, which evaluates the devox at c2-sized clouds), so S steps of
extraction + matching cost one host call.
"""
import torch

from . import _lib, ops
from .extractor import SphExtractor


class PairMatch:
    """Output and workspace buffers of the per-step matching of P pairs of
    N-point clouds: corr12 / corr21 / idx1 / idx2 [P, N] int32, count [P]."""

    def __init__(self, pairs, npoints, device):
        self.pairs, self.n = int(pairs), int(npoints)
        i32 = dict(dtype=torch.int32, device=device)
        self.corr12 = torch.empty((pairs, npoints), **i32)
        self.corr21 = torch.empty((pairs, npoints), **i32)
        self.idx1 = torch.empty((pairs, npoints), **i32)
        self.idx2 = torch.empty((pairs, npoints), **i32)
        self.count = torch.empty((pairs,), **i32)
        need = _lib.load().pcr_mutual_nn_workspace_size(pairs, npoints, npoints)
        # three parts: the runner's schedules 6 / 7 match consecutive steps
        # on two / three queues at once, each in its own part
        part = (max(256, need) + 255) // 256 * 256
        self.ws = torch.empty(3 * part + 768, dtype=torch.uint8, device=device)

    def outputs(self):
        return {"corr12": self.corr12, "corr21": self.corr21, "idx1": self.idx1,
                "idx2": self.idx2, "count": self.count}


class PairExtractor:
    """Extraction + matching of a rank's P registration pairs per step."""

    def __init__(self, pairs, npoints, channels, k, resolution, device="cuda", relative=True):
        self.pairs = int(pairs)
        self.ex = SphExtractor(2 * pairs, npoints, channels, k, resolution, device=device,
                               relative=relative)
        self.match = PairMatch(pairs, npoints, self.ex.device)

    @staticmethod
    def pack(src, tgt):
        """[P, ...] sources and targets -> the [2P, ...] batch of one step."""
        return torch.cat((src, tgt), dim=0).contiguous()

    def forward(self, xyz, normals, features):
        """One step from Python: extractor forward, then the matching on the
        current stream.  Inputs are the packed [2P, ...] batch."""
        out = dict(self.ex.forward(xyz, normals, features))
        p = self.pairs
        dv = out["devox"]
        got = ops.mutual_nn_match(dv[:p], dv[p:], channel_major=True, workspace=self.match.ws)
        out.update(zip(("corr12", "corr21", "idx1", "idx2", "count"), got))
        return out

    def run_native(self, xyz, normals, features, steps, desc_steps=None, schedule=0,
                   timed=False):
        """`steps` serial steps of extraction + matching from one native
        runner call (schedule 0); the matching outputs of the last step stay
        in self.match."""
        out = dict(self.ex.run_native(xyz, normals, features, steps, desc_steps,
                                      schedule=schedule, timed=timed, match=self.match))
        out.update(self.match.outputs())
        return out

    def run_ring(self, batches, steps, set0=0, desc_steps=None, schedule=6, timed=False):
        """`steps` pipelined steps of extraction + matching over a batch ring
        of packed [2P, ...] batches (SphExtractor.run_ring): step s matches
        the pairs of batches[(set0 + s) % R] into that ring set's corr12 /
        corr21 / idx1 / idx2 / count."""
        return self.ex.run_ring(batches, steps, set0, desc_steps, schedule=schedule,
                                timed=timed, match=self.match)

    def grid_kernel_times(self):
        return self.ex.grid_kernel_times()

    def reserve_timing(self, timed_steps):
        self.ex.reserve_timing(timed_steps)

    def register(self, xyz, normals, features, icp=None, solver="ransac", **ransac):
        """forward, then the rigid transform of every pair from its
        correspondences (ops.rigid_ransac on the current stream; `ransac`:
        its keyword arguments): forward's keys plus transform [P, 4, 4] fp64
        (target ~ R source + t), inliers, num_inliers, best_hyp and
        reg_status.  icp: a dict of ops.icp keywords (may be empty) refines
        that transform by point-to-point ICP into the icp_* keys of
        register_pairs; with estimation="point_to_plane" and no normals2 in
        it, the targets' normals (normals[P:]) are the planes.  solver="fgr": ops.fgr instead (the keywords are
        its own), with the keys of fgr_pairs; solver="teaser": ops.teaser,
        with the keys of teaser_pairs."""
        out = self.forward(xyz, normals, features)
        p = self.pairs
        icp = _icp_with_normals(icp, normals[p:])
        if _solver(solver) != "ransac":
            solve = _fgr_solve if solver == "fgr" else _teaser_solve
            out.update(solve(xyz[:p], xyz[p:], out["idx1"], out["idx2"], out["count"], icp,
                             ransac))
            return out
        got = ops.rigid_ransac(xyz[:p], xyz[p:], out["idx1"], out["idx2"], out["count"], **ransac)
        out.update(zip(("transform", "inliers", "num_inliers", "best_hyp", "reg_status"), got))
        if icp is not None:
            out.update(_icp_refine(xyz[:p], xyz[p:], out["transform"], icp))
        return out


ICP_KEYS = ("transform", "corr", "num_corr", "fitness", "rmse", "iterations", "status")


def icp_pairs(xyz1, xyz2, init=None, counts1=None, counts2=None, **icp):
    """register_one_pair(func='icp') (utils/open3d_func.py:63-72), batched
    and on the device: xyz1 [p, 3, n1], xyz2 [p, 3, n2], init [p, 4, 4]
    float64 or None -> ops.icp's outputs as a dict (transform, corr, num_corr,
    fitness, rmse, iterations, status); `icp`: its keyword arguments, among
    them estimation="point_to_plane" with normals2 [p, 3, n2] (DESIGN.md
    4.8i).  counts1 / counts2 [p] int32: ragged pairs, as in ops.icp."""
    return dict(zip(ICP_KEYS, ops.icp(xyz1, xyz2, init, counts1=counts1, counts2=counts2, **icp)))


def _icp_refine(xyz1, xyz2, transform, icp, counts1=None, counts2=None):
    """ICP from `transform` (pairs whose RANSAC failed carry the identity)
    -> the icp_* keys; `icp` carries estimation / normals2 like any other
    ops.icp keyword"""
    got = ops.icp(xyz1, xyz2, transform, counts1=counts1, counts2=counts2, **icp)
    return {"icp_" + k: v for k, v in zip(ICP_KEYS, got)}


FGR_KEYS = ("transform", "slots", "num_corr", "num_trials", "mu", "reg_status")


def _icp_with_normals(icp, normals2):
    """`icp` with normals2 filled from the target normals the caller holds,
    when it asks for the point-to-plane step and brings none"""
    if icp is not None and icp.get("estimation") == "point_to_plane" and \
            icp.get("normals2") is None:
        icp = dict(icp, normals2=normals2)
    return icp


def _solver(solver):
    if solver not in ("ransac", "fgr", "teaser"):
        raise RuntimeError("unknown solver %r: expected 'ransac', 'fgr' or 'teaser'" % (solver,))
    return solver


def _fgr_solve(xyz1, xyz2, idx1, idx2, count, icp, fgr, counts1=None, counts2=None):
    """ops.fgr on a matching's output -> the FGR_KEYS, plus the icp_* keys"""
    out = dict(zip(FGR_KEYS, ops.fgr(xyz1, xyz2, idx1, idx2, count, counts1=counts1,
                                     counts2=counts2, **fgr)))
    if icp is not None:
        out.update(_icp_refine(xyz1, xyz2, out["transform"], icp, counts1, counts2))
    return out


def fgr_pairs(xyz1, xyz2, feat1, feat2, channel_major=False, icp=None, counts1=None,
              counts2=None, **fgr):
    """register_one_pair(func='fgr') (utils/open3d_func.py:34-75) after
    find_correspondence_one_pair, batched and on the device: the arguments of
    register_pairs -> a dict with the matching (idx1, idx2, count) and
    ops.fgr's outputs (transform, slots, num_corr, num_trials, mu,
    reg_status); `fgr`: its keyword arguments.  icp: a dict of ops.icp keywords
    (may be empty) refines the transform into the icp_* keys, as in
    register_pairs.  counts1 / counts2 [p] int32: ragged pairs, as in
    register_pairs."""
    _, _, idx1, idx2, count = ops.mutual_nn_match(feat1, feat2, channel_major=channel_major,
                                                  counts1=counts1, counts2=counts2)
    out = {"idx1": idx1, "idx2": idx2, "count": count}
    out.update(_fgr_solve(xyz1, xyz2, idx1, idx2, count, icp, fgr, counts1, counts2))
    return out


TEASER_KEYS = ("transform", "clique", "clique_size", "inliers", "num_inliers", "iterations",
               "reg_status")


def _teaser_solve(xyz1, xyz2, idx1, idx2, count, icp, teaser, counts1=None, counts2=None):
    """ops.teaser on a matching's output -> the TEASER_KEYS, plus the icp_* keys"""
    out = dict(zip(TEASER_KEYS, ops.teaser(xyz1, xyz2, idx1, idx2, count, **teaser)))
    if icp is not None:
        out.update(_icp_refine(xyz1, xyz2, out["transform"], icp, counts1, counts2))
    return out


def teaser_pairs(xyz1, xyz2, feat1, feat2, channel_major=False, icp=None, counts1=None,
                 counts2=None, **teaser):
    """register_one_pair(func='teaserpp')
    (datasets/modelnet40_registration.py:274-327) after
    find_correspondence_one_pair, batched and on the device: the arguments of
    register_pairs -> a dict with the matching (idx1, idx2, count) and
    ops.teaser's outputs (transform, clique, clique_size, inliers, num_inliers,
    iterations, reg_status); `teaser`: its keyword arguments.  icp: a dict of
    ops.icp keywords (may be empty) refines the transform into the icp_* keys,
    as in register_pairs.  counts1 / counts2 [p] int32: ragged pairs, as in
    register_pairs (the solver reads only the points the matching names)."""
    _, _, idx1, idx2, count = ops.mutual_nn_match(feat1, feat2, channel_major=channel_major,
                                                  counts1=counts1, counts2=counts2)
    out = {"idx1": idx1, "idx2": idx2, "count": count}
    out.update(_teaser_solve(xyz1, xyz2, idx1, idx2, count, icp, teaser, counts1, counts2))
    return out


def register_pairs(xyz1, xyz2, feat1, feat2, channel_major=False, icp=None, solver="ransac",
                   counts1=None, counts2=None, **ransac):
    """Pair in, transform out (datasets/deepgmr_mn40.py:165-244,
    find_correspondence_one_pair + register_one_pair(func='ransac'), batched
    and on the device): xyz1 [p, 3, n1], xyz2 [p, 3, n2] and per-point
    features [p, n, c] (channel_major: [p, c, n]) -> a dict with the matching
    (idx1, idx2, count) and ops.rigid_ransac's outputs (transform, inliers,
    num_inliers, best_hyp, reg_status; scores with return_scores).  The
    correspondence count never visits the host.  icp: a dict of ops.icp
    keywords (may be empty) refines the RANSAC transform by point-to-point
    ICP over every point; its outputs come as icp_transform, icp_corr,
    icp_num_corr, icp_fitness, icp_rmse, icp_iterations and icp_status, the
    other keys are unchanged (estimation="point_to_plane" and normals2 in the
    dict: the point-to-plane step).  solver="fgr": fgr_pairs with the same
    arguments (the keywords are ops.fgr's); solver="teaser": teaser_pairs (the
    keywords are ops.teaser's).  counts1 / counts2 [p] int32: ragged pairs
     -- pair q's clouds are the first counts1[q] / counts2[q]
    points; the matching names valid points only (RANSAC and TEASER read no
    others), and FGR and ICP take the counts themselves.  With both None the
    dense entry points run."""
    if _solver(solver) != "ransac":
        pairs = fgr_pairs if solver == "fgr" else teaser_pairs
        return pairs(xyz1, xyz2, feat1, feat2, channel_major=channel_major, icp=icp,
                     counts1=counts1, counts2=counts2, **ransac)
    _, _, idx1, idx2, count = ops.mutual_nn_match(feat1, feat2, channel_major=channel_major,
                                                  counts1=counts1, counts2=counts2)
    got = ops.rigid_ransac(xyz1, xyz2, idx1, idx2, count, **ransac)
    out = {"idx1": idx1, "idx2": idx2, "count": count}
    out.update(zip(("transform", "inliers", "num_inliers", "best_hyp", "reg_status", "scores"),
                   got))
    if icp is not None:
        out.update(_icp_refine(xyz1, xyz2, out["transform"], icp, counts1, counts2))
    return out


def apply_transform(xyz, transform):
    """R xyz + t of [p, 3, n] clouds under [p, 4, 4] transforms (the
    reference's apply_transform(pt1, est)), in the transforms' dtype."""
    x = xyz.to(transform.dtype)
    return transform[:, :3, :3] @ x + transform[:, :3, 3:4]


def rre_rte(gt, est):
    """RE_TE_one_pair (datasets/deepgmr_mn40.py:152-164), batched over
    [p, 4, 4] transforms: the rotation error in degrees,
    acos(clamp((tr(Rgt^T Rest) - 1) / 2, -1, 1)), and the norm of the
    translation difference."""
    gt, est = gt.to(torch.float64), est.to(torch.float64)
    tr = (gt[:, :3, :3] * est[:, :3, :3]).sum(dim=(1, 2))
    rre = torch.rad2deg(torch.acos(torch.clamp((tr - 1.0) / 2.0, -1.0, 1.0)))
    rte = torch.linalg.norm(gt[:, :3, 3] - est[:, :3, 3], dim=1)
    return rre, rte


def alignment_rmse(xyz1, gt, est):
    """The reference meter's rmse (datasets/deepgmr_mn40.py:124-126), batched:
    the mean over the points of [p, 3, n] clouds of |est p - gt p|, fp64 [p]."""
    gt, est = gt.to(torch.float64), est.to(torch.float64)
    return torch.linalg.norm(apply_transform(xyz1, est) - apply_transform(xyz1, gt), dim=1).mean(
        dim=1)


def fpfh_pairs(xyz1, normals1, xyz2, normals2, radius, k=100, solver="ransac", icp=None,
               search="knn", counts1=None, counts2=None, **solver_args):
    """Two clouds with normals in, transform out, with nothing trained: the
    FPFH descriptors of both clouds (ops.fpfh with `radius`, `k` and `search`:
    "knn" or "grid", the neighbour search behind the descriptor; DESIGN.md
    4.8f, 4.8g), then register_pairs on them (channel-major, 33 channels) with
    `solver`, `icp` and the solver's keyword arguments.  xyz [p, 3, n] and
    normals [p, 3, n] per side -> register_pairs' dict plus feat1 [p, 33, n1]
    and feat2 [p, 33, n2].  counts1 / counts2 [p] int32: ragged pairs, carried
    through the descriptors, the matching, the solver and ICP; they need
    search="grid".  icp with estimation="point_to_plane" and no normals2 of
    its own refines along normals2, the target normals given here."""
    if (counts1 is not None or counts2 is not None) and search != "grid":
        raise RuntimeError("fpfh_pairs: counts need search='grid'")
    feat1 = ops.fpfh(xyz1, normals1, radius, k, search=search, counts=counts1)
    feat2 = ops.fpfh(xyz2, normals2, radius, k, search=search, counts=counts2)
    icp = _icp_with_normals(icp, normals2)
    out = register_pairs(xyz1, xyz2, feat1, feat2, channel_major=True, icp=icp, solver=solver,
                         counts1=counts1, counts2=counts2, **solver_args)
    out["feat1"], out["feat2"] = feat1, feat2
    return out


def scan_pairs(scans1, scans2, cell, normal_radius=None, normal_k=30, feature_radius=None,
               feature_k=100, solver="ransac", icp=None, **solver_args):
    """Raw scan pairs in, transforms out, in one batched pass with nothing
    trained: scans1 / scans2 are lists of [3, n_i] float32
    clouds of any sizes (pair q is scans1[q], scans2[q]).  io.pad_clouds ->
    ops.grid_subsample at `cell` -> ops.estimate_normals_hybrid (radius
    normal_radius, 2 * cell by default, max_nn normal_k) -> ops.fpfh on the
    grid (radius feature_radius, 5 * cell by default, feature_k) -> the ragged
    matching -> `solver` -> the ragged ICP with `icp` (a dict of ops.icp
    keywords, may be empty; None: none; estimation="point_to_plane" refines
    along the targets' estimated normals).  The subsampled clouds stay ragged
    all the way and nothing visits the host between the stages.  Returns
    register_pairs' dict plus xyz1 / xyz2 [p, 3, n], counts1 / counts2 [p],
    normals1 / normals2, feat1 / feat2 [p, 33, n] and sub_status1 /
    sub_status2 [p] (ops.grid_subsample's status)."""
    from . import io
    if len(scans1) != len(scans2) or len(scans1) < 1:
        raise RuntimeError("scan_pairs: expected two lists of equal, non-zero length")
    cell = float(cell)
    nr = 2.0 * cell if normal_radius is None else float(normal_radius)
    fr = 5.0 * cell if feature_radius is None else float(feature_radius)
    side = []
    for scans in (scans1, scans2):
        xyz, cnt = io.pad_clouds(scans)
        sub = ops.grid_subsample(xyz, cell, counts=cnt)
        normals = ops.estimate_normals_hybrid(sub["xyz"], nr, normal_k, sub["count"])
        side.append((sub["xyz"], sub["count"], normals, sub["status"]))
    (x1, c1, nm1, s1), (x2, c2, nm2, s2) = side
    out = fpfh_pairs(x1, nm1, x2, nm2, fr, feature_k, solver=solver, icp=icp, search="grid",
                     counts1=c1, counts2=c2, **solver_args)
    out.update(xyz1=x1, xyz2=x2, counts1=c1, counts2=c2, normals1=nm1, normals2=nm2,
               sub_status1=s1, sub_status2=s2)
    return out
