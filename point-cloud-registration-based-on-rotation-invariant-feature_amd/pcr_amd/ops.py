"""Torch-tensor entry points of the MI355X hot path.

Each function reproduces one function of the reference's pybind11 module
``_multi_shape_pvcnn_backend`` (PVCNN/modules/functional/src/bindings.cpp:13-56)
-- same name, argument order, checks and return structure -- and calls the
C ABI of libpcr_amd.so on torch's current HIP stream.  Outputs are allocated
with ``torch.empty`` (the library writes every element, including the slots
the reference leaves at its ``torch::zeros`` / ``ones*10000`` fill).

Checks follow src/utils.hpp:15-28 (CHECK_CUDA / CHECK_CONTIGUOUS /
CHECK_IS_FLOAT / CHECK_IS_INT -> RuntimeError with the same messages).
"""
import torch

from . import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _check_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)


def _check_contig(t, name):
    if not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous tensor" % name)


def _check_float(t, name):
    if t.dtype != torch.float32:
        raise RuntimeError("%s must be a float tensor" % name)


def _check_int(t, name):
    if t.dtype != torch.int32:
        raise RuntimeError("%s must be an int tensor" % name)


def _check(t, name, kind="float"):
    _check_cuda(t, name)
    _check_contig(t, name)
    if kind == "float":
        _check_float(t, name)
    elif kind == "int":
        _check_int(t, name)


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _workspace_or(workspace, nbytes, device):
    """the caller's workspace if it is big enough, else a fresh one"""
    need = max(256, nbytes)
    if workspace is not None and workspace.numel() >= need:
        return workspace
    return torch.empty(need, dtype=torch.uint8, device=device)


def _check_counts(counts, p, what, shape_msg=None):
    """counts [p] int32 on the device, or None"""
    if counts is not None:
        _check(counts, what, "int")
        if tuple(counts.shape) != (p,):
            raise RuntimeError(shape_msg or "%s: expected [p] (one count per pair)" % what)


def _check_pairs(op, xyz1, xyz2, corr=None):
    """The solvers' common arguments: xyz1 [p, 3, n1] and xyz2 [p, 3, n2], and
    with corr = (idx1, idx2, count) the correspondence rows idx1 / idx2
    [p, n1] and count [p] -> p, n1, n2"""
    _check(xyz1, "xyz1")
    _check(xyz2, "xyz2")
    idx1, idx2, count = corr or (None, None, None)
    if corr:
        _check(idx1, "idx1", "int")
        _check(idx2, "idx2", "int")
        _check(count, "count", "int")
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[1] != 3 or xyz2.shape[1] != 3 or \
            xyz1.shape[0] != xyz2.shape[0]:
        raise RuntimeError("%s: expected [p, 3, n] clouds with equal pair counts" % op)
    p, _, n1 = xyz1.shape
    n2 = xyz2.shape[2]
    if corr and (tuple(idx1.shape) != (p, n1) or tuple(idx2.shape) != (p, n1) or
                 tuple(count.shape) != (p,)):
        raise RuntimeError("%s: expected idx1 / idx2 [p, n1] and count [p]" % op)
    return p, n1, n2


# ------------------------------------------------------------------ KNN
def knn_forward_cuda(xyz1, xyz2, k):
    """knn/knn.cpp:6-25 -> [dist1, dist2, idx1, idx2]."""
    _check(xyz1, "xyz1")
    _check(xyz2, "xyz2")
    b, c, n = xyz1.shape
    m = xyz2.shape[2]
    k = int(k)
    dev = xyz1.device
    dist1 = torch.empty((b, k, n), dtype=torch.float32, device=dev)
    dist2 = torch.empty((b, k, m), dtype=torch.float32, device=dev)
    idx1 = torch.empty((b, k, n), dtype=torch.int32, device=dev)
    idx2 = torch.empty((b, k, m), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.pcr_knn_workspace_size(b, n, m), dev)
    _lib.check(lib.pcr_knn_forward(
        _ptr(xyz1), _ptr(xyz2), b, c, n, m, k, _ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2),
        _ptr(ws), ws.numel(), _stream()), "knn_forward_cuda")
    return [dist1, dist2, idx1, idx2]


def knn_backward_cuda(xyz1, xyz2, graddist1, graddist2, idx1, idx2):
    """knn/knn.cpp:27-52 -> [gradxyz1, gradxyz2]."""
    _check(xyz1, "xyz1")
    _check(xyz2, "xyz2")
    _check(graddist1, "graddist1")
    _check(graddist2, "graddist2")
    _check(idx1, "idx1", "int")
    _check(idx2, "idx2", "int")
    b, c, n = xyz1.shape
    m = xyz2.shape[2]
    k = idx1.shape[1]
    g1 = torch.empty((b, c, n), dtype=torch.float32, device=xyz1.device)
    g2 = torch.empty((b, c, m), dtype=torch.float32, device=xyz1.device)
    # the atomics-free path: (query, slot) pairs counting-sorted by neighbour
    # in a workspace, then one gather per point (bit-repeatable)
    lib = _lib.load()
    ws = torch.empty(lib.pcr_knn_backward_workspace_size(b, n, m, k), dtype=torch.uint8,
                     device=xyz1.device)
    _lib.check(lib.pcr_knn_backward_ws(
        _ptr(xyz1), _ptr(xyz2), _ptr(graddist1), _ptr(graddist2), _ptr(idx1), _ptr(idx2),
        b, c, n, m, k, _ptr(g1), _ptr(g2), _ptr(ws), ws.numel(), _stream()),
        "knn_backward_cuda")
    return [g1, g2]


# ------------------------------------------------------------------ PPF
def spherical_ppf_forward(coords, center, normals, center_normal):
    """spherical_ppf/ppf.cpp:17-36 -> feat [b, 4, n]."""
    for t, nm in ((coords, "coords"), (center, "center"), (normals, "normals"),
                  (center_normal, "center_normal")):
        _check(t, nm)
    b, _, n = coords.shape
    feat = torch.empty((b, 4, n), dtype=torch.float32, device=coords.device)
    _lib.check(_lib.load().pcr_spherical_ppf_forward(
        _ptr(coords), _ptr(center), _ptr(normals), _ptr(center_normal), b, n, _ptr(feat),
        _stream()), "spherical_ppf_forward")
    return feat


def local_ppf_forward(points, normals, centers, center_normals, indices, kmajor=False,
                      relative=True):
    """Fused grouping + local PPF of pvcnn_classify.py:252-269 -> [b, 4, u, m]."""
    for t, nm in ((points, "points"), (normals, "normals"), (centers, "centers"),
                  (center_normals, "center_normals")):
        _check(t, nm)
    _check(indices, "indices", "int")
    b, _, n = points.shape
    m = centers.shape[2]
    u = indices.shape[1] if kmajor else indices.shape[2]
    out = torch.empty((b, 4, u, m), dtype=torch.float32, device=points.device)
    _lib.check(_lib.load().pcr_local_ppf_forward(
        _ptr(points), _ptr(normals), _ptr(centers), _ptr(center_normals), _ptr(indices),
        b, n, m, u, int(bool(kmajor)), int(bool(relative)), _ptr(out), _stream()),
        "local_ppf_forward")
    return out


def knn_local_ppf(xyz, normals, k, relative=True, want_dist=False):
    """Fused self-KNN + local PPF -> (idx [b,k,n], ppf [b,4,k,n], dist or None)."""
    _check(xyz, "xyz")
    _check(normals, "normals")
    b, _, n = xyz.shape
    dev = xyz.device
    idx = torch.empty((b, k, n), dtype=torch.int32, device=dev)
    ppf = torch.empty((b, 4, k, n), dtype=torch.float32, device=dev)
    dist = torch.empty((b, k, n), dtype=torch.float32, device=dev) if want_dist else None
    lib = _lib.load()
    ws = _workspace(lib.pcr_knn_workspace_size(b, n, n), dev)
    _lib.check(lib.pcr_knn_local_ppf(
        _ptr(xyz), _ptr(normals), b, n, int(k), int(bool(relative)), _ptr(idx), _ptr(dist),
        _ptr(ppf), _ptr(ws), ws.numel(), _stream()), "knn_local_ppf")
    return idx, ppf, dist


# -------------------------------------------------- ball query / grouping
def ball_query(centers_coords, points_coords, radius, num_neighbors):
    """ball_query/ball_query.cpp:6-30 -> idx [b, m, u]."""
    _check(centers_coords, "centers_coords")
    _check(points_coords, "points_coords")
    b, _, m = centers_coords.shape
    n = points_coords.shape[2]
    u = int(num_neighbors)
    idx = torch.empty((b, m, u), dtype=torch.int32, device=centers_coords.device)
    _lib.check(_lib.load().pcr_ball_query(
        _ptr(centers_coords), _ptr(points_coords), b, m, n, float(radius), u, _ptr(idx),
        _stream()), "ball_query")
    return idx


def grouping_forward(features, indices):
    """grouping/grouping.cpp:6-24 -> [b, c, m, u]."""
    _check(features, "features")
    _check(indices, "indices", "int")
    b, c, n = features.shape
    m, u = indices.shape[1], indices.shape[2]
    out = torch.empty((b, c, m, u), dtype=torch.float32, device=features.device)
    _lib.check(_lib.load().pcr_grouping_forward(
        _ptr(features), _ptr(indices), b, c, n, m, u, _ptr(out), _stream()), "grouping_forward")
    return out


def grouping_backward(grad_y, indices, n):
    """grouping/grouping.cpp:26-44 -> [b, c, n]."""
    _check(grad_y, "grad_y")
    _check(indices, "indices", "int")
    b, c = grad_y.shape[:2]
    m, u = indices.shape[1], indices.shape[2]
    gx = torch.empty((b, c, int(n)), dtype=torch.float32, device=grad_y.device)
    _lib.check(_lib.load().pcr_grouping_backward(
        _ptr(grad_y), _ptr(indices), b, c, int(n), m, u, _ptr(gx), _stream()),
        "grouping_backward")
    return gx


# ----------------------------------------------------------- voxelization
def spherical_avg_voxelize_forward(features, coords, resolution):
    """spherical_voxelization/spherical_vox.cpp:17-46 -> [out, ind, cnt]."""
    _check(features, "features")
    _check(coords, "coords")
    b, c, n = features.shape
    r = int(resolution)
    r3 = r * r * r
    dev = features.device
    out = torch.empty((b, c, r3), dtype=torch.float32, device=dev)
    ind = torch.empty((b, n), dtype=torch.int32, device=dev)
    cnt = torch.empty((b, r3), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.pcr_voxelize_workspace_size_c(b, c, n, r), dev)
    _lib.check(lib.pcr_spherical_avg_voxelize_forward(
        _ptr(features), _ptr(coords), b, c, n, r, _ptr(out), _ptr(ind), _ptr(cnt), _ptr(ws),
        ws.numel(), _stream()), "spherical_avg_voxelize_forward")
    return [out, ind, cnt]


def avg_voxelize_forward(features, coords, resolution):
    """voxelization/vox.cpp:17-46 (int voxel coords) -> [out, ind, cnt]."""
    _check(features, "features")
    _check(coords, "coords", "int")
    b, c, n = features.shape
    r = int(resolution)
    r3 = r * r * r
    dev = features.device
    out = torch.empty((b, c, r3), dtype=torch.float32, device=dev)
    ind = torch.empty((b, n), dtype=torch.int32, device=dev)
    cnt = torch.empty((b, r3), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.pcr_voxelize_workspace_size_c(b, c, n, r), dev)
    _lib.check(lib.pcr_avg_voxelize_forward(
        _ptr(features), _ptr(coords), b, c, n, r, _ptr(out), _ptr(ind), _ptr(cnt), _ptr(ws),
        ws.numel(), _stream()), "avg_voxelize_forward")
    return [out, ind, cnt]


def _avg_vox_backward(grad_y, indices, cnt, what):
    _check(grad_y, "grad_y")
    _check(indices, "indices", "int")
    _check(cnt, "cnt", "int")
    b, c, s = grad_y.shape
    n = indices.shape[1]
    gx = torch.empty((b, c, n), dtype=torch.float32, device=grad_y.device)
    _lib.check(_lib.load().pcr_avg_voxelize_backward(
        _ptr(grad_y), _ptr(indices), _ptr(cnt), b, c, n, s, _ptr(gx), _stream()), what)
    return gx


def spherical_avg_voxelize_backward(grad_y, indices, cnt):
    """spherical_vox.cpp:57-79 -> grad_x [b, c, n]."""
    return _avg_vox_backward(grad_y, indices, cnt, "spherical_avg_voxelize_backward")


def avg_voxelize_backward(grad_y, indices, cnt):
    """vox.cpp:57-76 -> grad_x [b, c, n]."""
    return _avg_vox_backward(grad_y, indices, cnt, "avg_voxelize_backward")


def spherical_normalize(coords):
    """Spherical_Voxelization's normalisation (modules/spherical_vox.py:16-20)."""
    _check(coords, "coords")
    b, _, n = coords.shape
    out = torch.empty_like(coords)
    _lib.check(_lib.load().pcr_spherical_normalize(_ptr(coords), b, n, _ptr(out), _stream()),
               "spherical_normalize")
    return out


# --------------------------------------------------------- devoxelization
def spherical_trilinear_devoxelize_forward(r, is_training, coords, features, g_inds):
    """interpolate/spherical_trilinear_devox.cpp:19-56 -> [outs, inds, wgts]."""
    _check(features, "features")
    _check(coords, "coords")
    _check_cuda(g_inds, "g_inds")
    g_inds = g_inds.contiguous()
    if g_inds.dtype != torch.int32:
        raise RuntimeError("g_inds must be an int tensor")
    b, c = features.shape[:2]
    n = coords.shape[2]
    dev = features.device
    outs = torch.empty((b, c, n), dtype=torch.float32, device=dev)
    inds = torch.empty((b, 8, n), dtype=torch.int32, device=dev)
    wgts = torch.empty((b, 8, n), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().pcr_spherical_trilinear_devoxelize_forward(
        int(r), int(bool(is_training)), _ptr(coords), _ptr(features), _ptr(g_inds), b, c, n,
        _ptr(outs), _ptr(inds), _ptr(wgts), _stream()), "spherical_trilinear_devoxelize_forward")
    return [outs, inds, wgts]


def trilinear_devoxelize_forward(r, is_training, coords, features):
    """interpolate/trilinear_devox.cpp:18-56 -> [outs, inds, wgts]."""
    _check(features, "features")
    _check(coords, "coords")
    b, c = features.shape[:2]
    n = coords.shape[2]
    dev = features.device
    outs = torch.empty((b, c, n), dtype=torch.float32, device=dev)
    inds = torch.empty((b, 8, n), dtype=torch.int32, device=dev)
    wgts = torch.empty((b, 8, n), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().pcr_trilinear_devoxelize_forward(
        int(r), int(bool(is_training)), _ptr(coords), _ptr(features), b, c, n, _ptr(outs),
        _ptr(inds), _ptr(wgts), _stream()), "trilinear_devoxelize_forward")
    return [outs, inds, wgts]


def _devox_backward(grad_y, indices, weights, r, spherical, what):
    _check(grad_y, "grad_y")
    _check(weights, "weights")
    _check(indices, "indices", "int")
    b, c, n = grad_y.shape
    r = int(r)
    gx = torch.empty((b, c, r * r * r), dtype=torch.float32, device=grad_y.device)
    lib = _lib.load()
    ws = _workspace(lib.pcr_devoxelize_backward_workspace_size_r(b, n, r, int(spherical)),
                    grad_y.device)
    _lib.check(lib.pcr_devoxelize_backward_ws(
        _ptr(grad_y), _ptr(indices), _ptr(weights), b, c, n, r, int(spherical), _ptr(gx),
        _ptr(ws), ws.numel(), _stream()), what)
    return gx


def spherical_trilinear_devoxelize_backward(grad_y, indices, weights, r):
    """spherical_trilinear_devox.cpp:68-92 -> grad_x [b, c, r^3]."""
    return _devox_backward(grad_y, indices, weights, r, True,
                           "spherical_trilinear_devoxelize_backward")


def trilinear_devoxelize_backward(grad_y, indices, weights, r):
    """trilinear_devox.cpp:58-91 -> grad_x [b, c, r^3]."""
    return _devox_backward(grad_y, indices, weights, r, False, "trilinear_devoxelize_backward")


def dgcnn_center_gather(features, avg_grid, ind):
    """PVConv dgcnn centre term (modules/pvconv.py:68-89) -> related [b, c, n]."""
    _check(features, "features")
    _check(avg_grid, "avg_grid")
    _check(ind, "ind", "int")
    b, c, n = features.shape
    r3 = avg_grid.shape[2]
    out = torch.empty_like(features)
    _lib.check(_lib.load().pcr_dgcnn_center_gather(
        _ptr(features), _ptr(avg_grid), _ptr(ind), b, c, n, r3, _ptr(out), _stream()),
        "dgcnn_center_gather")
    return out


# ---------------------------------------------- PointNet++ ops (8f f4)
def gather_features_forward(features, indices):
    """sampling/sampling.cpp:6-23 -> out [b, c, m]."""
    _check(features, "features")
    _check(indices, "indices", "int")
    b, c, n = features.shape
    m = indices.shape[1]
    out = torch.empty((b, c, m), dtype=torch.float32, device=features.device)
    _lib.check(_lib.load().pcr_gather_features_forward(
        _ptr(features), _ptr(indices), b, c, n, m, _ptr(out), _stream()),
        "gather_features_forward")
    return out


def gather_features_backward(grad_y, indices, n):
    """sampling/sampling.cpp:25-41 -> grad_x [b, c, n]."""
    _check(grad_y, "grad_y")
    _check(indices, "indices", "int")
    b, c, m = grad_y.shape
    n = int(n)
    gx = torch.empty((b, c, n), dtype=torch.float32, device=grad_y.device)
    _lib.check(_lib.load().pcr_gather_features_backward(
        _ptr(grad_y), _ptr(indices), b, c, n, m, _ptr(gx), _stream()),
        "gather_features_backward")
    return gx


def furthest_point_sampling(coords, num_samples):
    """sampling/sampling.cpp:43-58 (bound as ``furthest_point_sampling``,
    bindings.cpp:18) -> indices [b, num_samples] int32."""
    _check(coords, "coords")
    b, _, n = coords.shape
    m = int(num_samples)
    dev = coords.device
    idx = torch.empty((b, m), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.pcr_fps_workspace_size(b, n), dev)
    _lib.check(lib.pcr_furthest_point_sampling(
        _ptr(coords), b, n, m, _ptr(idx), _ptr(ws), ws.numel(), _stream()),
        "furthest_point_sampling")
    return idx


def three_nearest_neighbors_interpolate_forward(points_coords, centers_coords, centers_features):
    """interpolate/neighbor_interpolate.cpp:6-40 -> [out, indices, weights]."""
    _check(points_coords, "points_coords")
    _check(centers_coords, "centers_coords")
    _check(centers_features, "centers_features")
    b, c, m = centers_features.shape
    n = points_coords.shape[2]
    dev = points_coords.device
    out = torch.empty((b, c, n), dtype=torch.float32, device=dev)
    inds = torch.empty((b, 3, n), dtype=torch.int32, device=dev)
    wgts = torch.empty((b, 3, n), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().pcr_three_nn_interpolate_forward(
        _ptr(points_coords), _ptr(centers_coords), _ptr(centers_features), b, c, m, n,
        _ptr(out), _ptr(inds), _ptr(wgts), _stream()),
        "three_nearest_neighbors_interpolate_forward")
    return [out, inds, wgts]


def three_nearest_neighbors_interpolate_backward(grad_y, indices, weights, m):
    """interpolate/neighbor_interpolate.cpp:42-65 -> grad_x [b, c, m]."""
    _check(grad_y, "grad_y")
    _check(indices, "indices", "int")
    _check(weights, "weights")
    b, c, n = grad_y.shape
    m = int(m)
    gx = torch.empty((b, c, m), dtype=torch.float32, device=grad_y.device)
    _lib.check(_lib.load().pcr_three_nn_interpolate_backward(
        _ptr(grad_y), _ptr(indices), _ptr(weights), b, c, n, m, _ptr(gx), _stream()),
        "three_nearest_neighbors_interpolate_backward")
    return gx


# ------------------------------------------ LRF change_coords (8f f2)
class LRFAssertionError(AssertionError):
    """One of the reference's change_coords asserts (pvcnn_classify.py:159,
    :169, :177) fired for some cloud."""


_LRF_MSG = {1: "base_x.norm() <= 1e-5 (pvcnn_classify.py:159)",
            2: "no base_y with |lambda| < 0.9 (pvcnn_classify.py:169)",
            3: "degenerate Gram-Schmidt, |base_x| < 1e-5 (pvcnn_classify.py:177)"}


def lrf_change_coords(coords, check=True, return_basis=False):
    """rot_invariant_preprocess == 'change_coords' (models/pvcnn_classify.py:
    153-184): coords [b, 3, n] -> new_coords [b, 3, n] in each cloud's local
    frame.  With ``check`` the per-cloud status is read back (one host sync,
    as the reference's asserts) and LRFAssertionError raised on a failure.
    ``return_basis`` also returns (basis [b, 3, 3], picks [b, 2], status [b])."""
    _check(coords, "coords")
    if coords.dim() != 3 or coords.shape[1] != 3:
        raise RuntimeError("lrf_change_coords: expected coords [b, 3, n]")
    b, _, n = coords.shape
    dev = coords.device
    out = torch.empty_like(coords)
    basis = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    picks = torch.empty((b, 2), dtype=torch.int32, device=dev)
    status = torch.empty((b,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().pcr_lrf_change_coords(
        _ptr(coords), b, n, _ptr(out), _ptr(basis), _ptr(picks), _ptr(status), _stream()),
        "lrf_change_coords")
    if check and b > 0:
        st = status.cpu()
        bad = torch.nonzero(st).flatten().tolist()
        if bad:
            raise LRFAssertionError("change_coords: cloud %d: %s" % (bad[0], _LRF_MSG[int(st[bad[0]])]))
    if return_basis:
        return out, (basis, picks, status)
    return out


# ------------------------------------------ normal estimation (8f f3)
def estimate_normals(points, radius=0.1, return_counts=False):
    """get_normals (utils/open3d_func.py:77-83) for a batch on the GPU:
    points [b, 3, n] -> unit normals [b, 3, n] from the PCA of each point's
    radius neighbourhood, flipped to face the origin (Open3D's
    orient_normals_towards_camera_location default), (0, 0, 1) with fewer
    than 3 neighbours.  ``return_counts`` also returns the neighbour counts
    [b, n] int32."""
    _check(points, "points")
    if points.dim() != 3 or points.shape[1] != 3:
        raise RuntimeError("estimate_normals: expected points [b, 3, n]")
    b, _, n = points.shape
    normals = torch.empty_like(points)
    counts = torch.empty((b, n), dtype=torch.int32, device=points.device)
    _lib.check(_lib.load().pcr_estimate_normals(
        _ptr(points), b, n, float(radius), _ptr(normals), _ptr(counts), _stream()),
        "estimate_normals")
    return (normals, counts) if return_counts else normals


def normals_from_neighbors(xyz, nbr_idx, return_counts=False):
    """Normals from ready neighbour lists (Open3D's estimate_normals with
    KDTreeSearchParamHybrid, the search taken out): xyz
    [b, 3, n], nbr_idx [b, k, n] int32 as hybrid_search returns it (the point
    itself in its own row; k <= 128) -> unit normals [b, 3, n] from the PCA
    of each row's points, facing the origin, (0, 0, 1) with fewer than 3.  A
    slot outside [0, n) is skipped, so a point with an empty row -- every pad
    of a ragged cloud -- gets (0, 0, 1).  return_counts: also the slots
    counted [b, n] int32.  Bit-identical from run to run."""
    _check(xyz, "xyz")
    _check(nbr_idx, "nbr_idx", "int")
    if xyz.dim() != 3 or xyz.shape[1] != 3 or xyz.shape[2] < 1:
        raise RuntimeError("normals_from_neighbors: expected xyz [b, 3, n] with n >= 1")
    b, _, n = xyz.shape
    if nbr_idx.dim() != 3 or nbr_idx.shape[0] != b or nbr_idx.shape[2] != n:
        raise RuntimeError("normals_from_neighbors: expected nbr_idx [b, k, n]")
    k = nbr_idx.shape[1]
    normals = torch.empty_like(xyz)
    counts = torch.empty((b, n), dtype=torch.int32, device=xyz.device) if return_counts else None
    _lib.check(_lib.load().pcr_normals_from_neighbors(
        _ptr(xyz), _ptr(nbr_idx), b, n, k, _ptr(normals), _ptr(counts), _stream()),
        "normals_from_neighbors")
    return (normals, counts) if return_counts else normals


def estimate_normals_hybrid(xyz, radius, k=30, counts=None):
    """Open3D's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn=k)) of
    b ragged clouds: hybrid_search(xyz, radius, min(k, 128), counts), then
    normals_from_neighbors on its rows.  counts [b] int32 -- cloud q's valid
    points are its first counts[q] -- or None for all n; the points past them
    are in no row and get (0, 0, 1)."""
    k = min(int(k), 128)
    _, idx, _ = hybrid_search(xyz, radius, k, counts)
    return normals_from_neighbors(xyz, idx)


def mutual_nn_match(feat1, feat2, channel_major=False, workspace=None, return_keys=False,
                    counts1=None, counts2=None):
    """Feature-space mutual nearest neighbours of p registration pairs
    (datasets/deepgmr_mn40.py:232-244, batched): feat1 [p, n1, c],
    feat2 [p, n2, c] -> (corr12 [p, n1], corr21 [p, n2], idx1 [p, n1],
    idx2 [p, n1], count [p]); the first count[q] entries of idx1[q] / idx2[q]
    are the mutual pairs in ascending idx1, the rest -1.  channel_major:
    feat1 [p, c, n1], feat2 [p, c, n2] (the extractor's per-point layout),
    matched in place.  return_keys: also (rowbest [p, n1], colbest [p, n2]),
    the winning 64-bit pcr_match_key of every row / column as int64 views of
    the workspace (the layout include/pcr_amd.h guarantees; no copy, valid
    until the workspace is reused).  counts1 / counts2 [p] int32: ragged pairs
    (pcr_mutual_nn_match_ragged) -- pair q matches its first
    counts1[q] rows of feat1 against its first counts2[q] of feat2 and gives
    the dense result on that trimmed pair, -1 past the counts (keys: all
    ones); None on one side: all of it.  With both None the dense entry
    points are called."""
    _check(feat1, "feat1")
    _check(feat2, "feat2")
    if feat1.dim() != 3 or feat2.dim() != 3 or feat1.shape[0] != feat2.shape[0]:
        raise RuntimeError("mutual_nn_match: expected 3-d features with equal pair counts")
    if channel_major:
        p, c, n1 = feat1.shape
        n2, c2 = feat2.shape[2], feat2.shape[1]
    else:
        p, n1, c = feat1.shape
        n2, c2 = feat2.shape[1], feat2.shape[2]
    if c != c2:
        raise RuntimeError("mutual_nn_match: channel counts differ (%d vs %d)" % (c, c2))
    dev = feat1.device
    i32 = dict(dtype=torch.int32, device=dev)
    corr12, corr21 = torch.empty((p, n1), **i32), torch.empty((p, n2), **i32)
    idx1, idx2 = torch.empty((p, n1), **i32), torch.empty((p, n1), **i32)
    count = torch.empty((p,), **i32)
    lib = _lib.load()
    ws = _workspace_or(workspace, lib.pcr_mutual_nn_workspace_size(p, n1, n2), dev)
    _check_counts(counts1, p, "counts1")
    _check_counts(counts2, p, "counts2")
    if counts1 is None and counts2 is None:
        fn = lib.pcr_mutual_nn_match_cm if channel_major else lib.pcr_mutual_nn_match
        _lib.check(fn(_ptr(feat1), _ptr(feat2), p, n1, n2, c, _ptr(corr12), _ptr(corr21),
                      _ptr(idx1), _ptr(idx2), _ptr(count), _ptr(ws), ws.numel(), _stream()),
                   "mutual_nn_match")
    else:
        _lib.check(lib.pcr_mutual_nn_match_ragged(
            _ptr(feat1), _ptr(feat2), p, n1, n2, c, _ptr(counts1), _ptr(counts2),
            int(bool(channel_major)), _ptr(corr12), _ptr(corr21), _ptr(idx1), _ptr(idx2),
            _ptr(count), _ptr(ws), ws.numel(), _stream()), "mutual_nn_match")
    if return_keys:
        off = (p * n1 * 8 + 255) // 256 * 256
        rowbest = ws[:p * n1 * 8].view(torch.int64).view(p, n1)
        colbest = ws[off:off + p * n2 * 8].view(torch.int64).view(p, n2)
        return corr12, corr21, idx1, idx2, count, rowbest, colbest
    return corr12, corr21, idx1, idx2, count


def find_correspondence_one_pair(feat1, feat2):
    """datasets/deepgmr_mn40.py:232-244 on the GPU: feat1 [n1, c],
    feat2 [n2, c] -> (idx1, idx2), the mutual nearest neighbours in feature
    space (int64 tensors on the features' device, ascending idx1)."""
    _, _, idx1, idx2, count = mutual_nn_match(feat1.unsqueeze(0), feat2.unsqueeze(0))
    n = int(count[0].item())
    return idx1[0, :n].long(), idx2[0, :n].long()


def rigid_ransac(xyz1, xyz2, idx1, idx2, count, hyps=1000, inlier_dist=0.08, edge_ratio=0.9,
                 refine_iters=2, seed=0, return_scores=False, workspace=None):
    """Rigid transforms of p registration pairs from their correspondences
    (datasets/deepgmr_mn40.py:165-231 register_one_pair(func='ransac'),
    batched; the defaults follow its max_iter=1000, voxel_size=0.08 and edge
    length 0.9): xyz1 [p, 3, n1], xyz2 [p, 3, n2], idx1 / idx2 [p, n1] and
    count [p] as mutual_nn_match returns them -> (transform [p, 4, 4] fp64
    with xyz2 ~ R xyz1 + t, inliers [p, n1] 0/1 per correspondence slot,
    num_inliers [p], best_hyp [p], status [p]: 0 ok, 1 fewer than 3
    correspondences, 2 every hypothesis rejected), plus scores [p, hyps] with
    return_scores.  Seeded and bit-identical from run to run."""
    p, n1, n2 = _check_pairs("rigid_ransac", xyz1, xyz2, (idx1, idx2, count))
    hyps, refine_iters = int(hyps), int(refine_iters)
    dev = xyz1.device
    i32 = dict(dtype=torch.int32, device=dev)
    transform = torch.empty((p, 4, 4), dtype=torch.float64, device=dev)
    inliers = torch.empty((p, n1), **i32)
    num_inliers, best_hyp, status = (torch.empty((p,), **i32) for _ in range(3))
    scores = torch.empty((p, max(hyps, 0)), **i32) if return_scores else None
    lib = _lib.load()
    ws = _workspace_or(workspace, lib.pcr_rigid_ransac_workspace_size(p, n1, hyps), dev)
    _lib.check(lib.pcr_rigid_ransac(
        _ptr(xyz1), _ptr(xyz2), p, n1, n2, _ptr(idx1), _ptr(idx2), _ptr(count), hyps,
        float(inlier_dist), float(edge_ratio), refine_iters, int(seed) & 0xFFFFFFFF,
        _ptr(transform), _ptr(inliers), _ptr(num_inliers), _ptr(best_hyp), _ptr(scores),
        _ptr(status), _ptr(ws), ws.numel(), _stream()), "rigid_ransac")
    out = (transform, inliers, num_inliers, best_hyp, status)
    return out + (scores,) if return_scores else out


def icp(xyz1, xyz2, init=None, max_dist=0.2, max_iters=200, rel_fitness=1e-6, rel_rmse=1e-6,
        counts1=None, counts2=None, estimation="point_to_point", normals2=None):
    """Point-to-point ICP of p registration pairs (utils/open3d_func.py:63-72,
    register_one_pair(func='icp'), batched; the defaults are its distance 0.2
    and 200 iterations with Open3D's default convergence criteria): xyz1
    [p, 3, n1] source, xyz2 [p, 3, n2] target, init [p, 4, 4] float64 (None:
    the identity) -> (transform [p, 4, 4] fp64 with xyz2 ~ R xyz1 + t, corr
    [p, n1] nearest target within max_dist or -1, num_corr [p], fitness [p],
    rmse [p], iterations [p], status [p]: 0 converged, 1 fewer than 3
    correspondences, 2 iteration limit).  max_iters = 0 evaluates init.  The
    whole loop runs on the device; bit-identical from run to run.  counts1 /
    counts2 [p] int32: ragged pairs (pcr_icp_point_to_point_ragged, DESIGN.md
    4.8h) -- only the first counts1[q] sources and counts2[q] targets exist,
    fitness is over counts1[q], corr is -1 past it, and the result is the
    dense one on the trimmed pair; an empty source returns init with status
    1.  With both None the dense entry point is called.
    estimation="point_to_plane" (pcr_icp_point_to_plane, DESIGN.md 4.8i;
    Open3D's TransformationEstimationPointToPlane): the same evaluation, but
    each step is the Gauss-Newton one on the residuals (R a + t - b) . n along
    the target's normals, normals2 [p, 3, n2] float32 (needed then; counts2
    covers them too).  Its status 1 is fewer than 6 correspondences, and
    status 3 a step whose 6 x 6 system has no Cholesky factor (a planar
    target, a NaN normal): the transform is then the last evaluated one."""
    if estimation not in ("point_to_point", "point_to_plane"):
        raise RuntimeError("icp: unknown estimation %r: expected 'point_to_point' or "
                           "'point_to_plane'" % (estimation,))
    plane = estimation == "point_to_plane"
    p, n1, n2 = _check_pairs("icp", xyz1, xyz2)
    if init is not None:
        _check(init, "init", None)
        if init.dtype != torch.float64 or tuple(init.shape) != (p, 4, 4):
            raise RuntimeError("icp: init must be a float64 [p, 4, 4] tensor")
    if plane:
        if normals2 is None:
            raise RuntimeError("icp: estimation='point_to_plane' needs normals2")
        _check(normals2, "normals2")
        if tuple(normals2.shape) != (p, 3, n2) or normals2.device != xyz2.device:
            raise RuntimeError("icp: normals2 must be a float [p, 3, n2] tensor on xyz2's device")
    dev = xyz1.device
    i32 = dict(dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    transform = torch.empty((p, 4, 4), **f64)
    corr = torch.empty((p, n1), **i32)
    num_corr, iterations, status = (torch.empty((p,), **i32) for _ in range(3))
    fitness, rmse = torch.empty((p,), **f64), torch.empty((p,), **f64)
    _check_counts(counts1, p, "counts1")
    _check_counts(counts2, p, "counts2")
    tail = (_ptr(init), float(max_dist), int(max_iters), float(rel_fitness), float(rel_rmse),
            _ptr(transform), _ptr(corr), _ptr(num_corr), _ptr(fitness), _ptr(rmse),
            _ptr(iterations), _ptr(status), _stream())
    if plane:
        _lib.check(_lib.load().pcr_icp_point_to_plane(
            _ptr(xyz1), _ptr(xyz2), _ptr(normals2), p, n1, n2, _ptr(counts1), _ptr(counts2),
            *tail), "icp")
    elif counts1 is None and counts2 is None:
        _lib.check(_lib.load().pcr_icp_point_to_point(_ptr(xyz1), _ptr(xyz2), p, n1, n2, *tail),
                   "icp")
    else:
        _lib.check(_lib.load().pcr_icp_point_to_point_ragged(
            _ptr(xyz1), _ptr(xyz2), p, n1, n2, _ptr(counts1), _ptr(counts2), *tail), "icp")
    return transform, corr, num_corr, fitness, rmse, iterations, status


def fgr(xyz1, xyz2, idx1, idx2, count, max_corr_dist=0.08, iterations=64, division_factor=1.4,
        decrease_mu=True, tuple_scale=0.95, max_tuples=1000, trials_per_corr=100,
        absolute_scale=False, seed=0, workspace=None, counts1=None, counts2=None):
    """Fast Global Registration of p registration pairs from their
    correspondences (utils/open3d_func.py:34-75, register_one_pair(func='fgr'),
    batched; the defaults are Open3D's FastGlobalRegistrationOption with the
    reference's maximum_correspondence_distance 0.08): xyz1 [p, 3, n1], xyz2
    [p, 3, n2], idx1 / idx2 [p, n1] and count [p] as mutual_nn_match returns
    them -> (transform [p, 4, 4] fp64 with xyz2 ~ R xyz1 + t, slots
    [p, 3 * max_tuples] -- the correspondence slots the tuple test kept, three
    per accepted triple in trial order, then -1 ([p, n1] and the slots
    themselves with max_tuples = 0) --, num_corr [p] their number, num_trials
    [p], mu [p] fp64 the final line-process parameter, status [p]: 0 ok, 1
    fewer than 10 correspondences kept, 2 degenerate or non-finite clouds, 3 a
    singular step).  Seeded and bit-identical from run to run.  counts1 /
    counts2 [p] int32: ragged pairs (pcr_fgr_ragged) -- the
    centroids and the scale run over the first counts1[q] / counts2[q] points,
    which gives the dense result on the trimmed pair (an empty cloud: status
    2).  With both None the dense entry point is called."""
    p, n1, n2 = _check_pairs("fgr", xyz1, xyz2, (idx1, idx2, count))
    max_tuples = int(max_tuples)
    if max_tuples < 0:
        raise RuntimeError("fgr: negative max_tuples (%d)" % max_tuples)
    dev = xyz1.device
    i32 = dict(dtype=torch.int32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    transform = torch.empty((p, 4, 4), **f64)
    slots = torch.empty((p, 3 * max_tuples if max_tuples else n1), **i32)
    num_corr, num_trials, status = (torch.empty((p,), **i32) for _ in range(3))
    mu = torch.empty((p,), **f64)
    lib = _lib.load()
    ws = _workspace_or(workspace, lib.pcr_fgr_workspace_size(p, n1, max_tuples), dev)
    _check_counts(counts1, p, "counts1")
    _check_counts(counts2, p, "counts2")
    tail = (_ptr(idx1), _ptr(idx2), _ptr(count),
            float(max_corr_dist), int(iterations), float(division_factor), int(bool(decrease_mu)),
            float(tuple_scale), max_tuples, int(trials_per_corr), int(bool(absolute_scale)),
            int(seed) & 0xFFFFFFFF, _ptr(transform), _ptr(slots), _ptr(num_corr), _ptr(num_trials),
            _ptr(mu), _ptr(status), _ptr(ws), ws.numel(), _stream())
    if counts1 is None and counts2 is None:
        _lib.check(lib.pcr_fgr(_ptr(xyz1), _ptr(xyz2), p, n1, n2, *tail), "fgr")
    else:
        _lib.check(lib.pcr_fgr_ragged(_ptr(xyz1), _ptr(xyz2), p, n1, n2, _ptr(counts1),
                                      _ptr(counts2), *tail), "fgr")
    return transform, slots, num_corr, num_trials, mu, status


def teaser(xyz1, xyz2, idx1, idx2, count, noise_bound=0.02, cbar2=1.0, gnc_factor=1.4,
           max_iters=100, cost_threshold=1e-12, seeds=0, inlier_selection=True, workspace=None):
    """TEASER-style robust registration of p registration pairs from their
    correspondences (datasets/modelnet40_registration.py:274-327,
    register_one_pair(func='teaserpp'), batched; noise_bound and cbar2 are the
    reference's call, the rest TEASER++'s defaults): xyz1
    [p, 3, n1], xyz2 [p, 3, n2], idx1 / idx2 [p, n1] and count [p] as
    mutual_nn_match returns them -> (transform [p, 4, 4] fp64 with xyz2 ~ R xyz1
    + t, clique [p, n1] -- the slots of the pairwise-consistent set a bounded
    greedy search found, ascending, then -1 (every slot with inlier_selection
    off) --, clique_size [p], inliers [p, n1] 0 / 1 per slot, num_inliers [p],
    iterations [p] the rotation solves made, status [p]: 0 ok, 1 a clique of
    fewer than 3, 2 non-finite points, 3 the iteration limit).  seeds: how many
    of the best-ranked slots start a search (0: all).  n1 <= 4096.
    Bit-identical from run to run."""
    p, n1, n2 = _check_pairs("teaser", xyz1, xyz2, (idx1, idx2, count))
    dev = xyz1.device
    i32 = dict(dtype=torch.int32, device=dev)
    transform = torch.empty((p, 4, 4), dtype=torch.float64, device=dev)
    clique, inliers = torch.empty((p, n1), **i32), torch.empty((p, n1), **i32)
    clique_size, num_inliers, iterations, status = (torch.empty((p,), **i32) for _ in range(4))
    lib = _lib.load()
    ws = _workspace_or(workspace, lib.pcr_teaser_workspace_size(p, n1), dev)
    _lib.check(lib.pcr_teaser(
        _ptr(xyz1), _ptr(xyz2), p, n1, n2, _ptr(idx1), _ptr(idx2), _ptr(count), float(noise_bound),
        float(cbar2), float(gnc_factor), int(max_iters), float(cost_threshold), int(seeds),
        int(bool(inlier_selection)), _ptr(transform), _ptr(clique), _ptr(clique_size),
        _ptr(inliers), _ptr(num_inliers), _ptr(iterations), _ptr(status), _ptr(ws), ws.numel(),
        _stream()), "teaser")
    return transform, clique, clique_size, inliers, num_inliers, iterations, status


def grid_subsample(xyz, cell, features=None, counts=None):
    """Grid subsampling (voxel-grid barycentres) of b ragged clouds
    (cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp,
    utils/grid_subsampleing.py grid_sub_sampling, batched):
    xyz [b, 3, n], cell the cell size, features [b, c, n] or None, counts [b]
    int32 -- cloud q's valid points are its first counts[q] -- or None for all
    n -> a dict: xyz [b, 3, n] and features [b, c, n] (None without features)
    hold the cells' barycentres in slots 0 .. count - 1, in ascending cell key,
    and 0 after them; count [b]; cell_of [b, n] the output slot of every input
    point (-1 past the valid count); cell_count [b, n] the points per slot;
    origin [b, 3] and dims [b, 3] of the grid; status [b]: 0 ok, 1 valid count
    outside [1, n], 2 a non-finite coordinate, 3 a grid finer than 2^20 cells
    along an axis (count 0 for those clouds).  Every cell sums its points in
    ascending point index: bit-identical from run to run."""
    _check(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[1] != 3 or xyz.shape[2] < 1:
        raise RuntimeError("grid_subsample: expected xyz [b, 3, n] with n >= 1")
    b, _, n = xyz.shape
    c = 0
    if features is not None:
        _check(features, "features")
        if features.dim() != 3 or features.shape[0] != b or features.shape[2] != n:
            raise RuntimeError("grid_subsample: expected features [b, c, n]")
        c = features.shape[1]
    _check_counts(counts, b, "counts", "grid_subsample: expected counts [b]")
    dev = xyz.device
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out_xyz = torch.empty((b, 3, n), **f32)
    out_feat = torch.empty((b, c, n), **f32) if features is not None else None
    count, status = torch.empty((b,), **i32), torch.empty((b,), **i32)
    cell_of, cell_count = torch.empty((b, n), **i32), torch.empty((b, n), **i32)
    origin, dims = torch.empty((b, 3), **f32), torch.empty((b, 3), **i32)
    lib = _lib.load()
    ws = _workspace(lib.pcr_grid_subsample_workspace_size(b, n, c), dev)
    _lib.check(lib.pcr_grid_subsample(
        _ptr(xyz), _ptr(features) if c else None, _ptr(counts), b, n, c, float(cell), _ptr(out_xyz),
        _ptr(out_feat) if c else None, _ptr(count), _ptr(cell_of), _ptr(cell_count), _ptr(origin),
        _ptr(dims), _ptr(status), _ptr(ws), ws.numel(), _stream()), "grid_subsample")
    return dict(xyz=out_xyz, features=out_feat, count=count, cell_of=cell_of,
                cell_count=cell_count, origin=origin, dims=dims, status=status)


# ------------------------------------------------ FPFH descriptors (4.8f)
def fpfh_from_neighbors(xyz, normals, nbr_idx, nbr_dist, radius, return_spfh=False,
                        return_counts=False):
    """FPFH descriptors (Open3D's compute_fpfh_feature, batched; DESIGN.md
    4.8f, include/pcr_fpfh.h) from ready neighbour lists: xyz [b, 3, n],
    normals [b, 3, n], nbr_idx [b, k, n] int32 and nbr_dist [b, k, n] as
    knn_forward_cuda(xyz, xyz, k) returns them (squared distances, ascending;
    k <= 128) -> fpfh [b, 33, n], the channel-major layout of
    mutual_nn_match(channel_major=True).  A point's neighbours are the listed
    points other than itself within `radius`.  return_spfh: also the stage-1
    histograms [b, 33, n]; return_counts: also the neighbour counts [b, n]
    int32 (in that order).  Bit-identical from run to run."""
    _check(xyz, "xyz")
    _check(normals, "normals")
    _check(nbr_idx, "nbr_idx", "int")
    _check(nbr_dist, "nbr_dist")
    if xyz.dim() != 3 or xyz.shape[1] != 3 or xyz.shape[2] < 1:
        raise RuntimeError("fpfh: expected xyz [b, 3, n] with n >= 1")
    b, _, n = xyz.shape
    if tuple(normals.shape) != (b, 3, n):
        raise RuntimeError("fpfh: expected normals [b, 3, n]")
    if nbr_idx.dim() != 3 or nbr_idx.shape[0] != b or nbr_idx.shape[2] != n or \
            nbr_idx.shape != nbr_dist.shape:
        raise RuntimeError("fpfh: expected nbr_idx and nbr_dist [b, k, n]")
    k = nbr_idx.shape[1]
    dev = xyz.device
    out = torch.empty((b, 33, n), dtype=torch.float32, device=dev)
    spfh = torch.empty((b, 33, n), dtype=torch.float32, device=dev) if return_spfh else None
    counts = torch.empty((b, n), dtype=torch.int32, device=dev) if return_counts else None
    lib = _lib.load()
    ws = _workspace(lib.pcr_fpfh_workspace_size(b, n), dev)
    _lib.check(lib.pcr_fpfh(
        _ptr(xyz), _ptr(normals), _ptr(nbr_idx), _ptr(nbr_dist), b, n, k, float(radius), _ptr(out),
        _ptr(spfh), _ptr(counts), _ptr(ws), ws.numel(), _stream()), "fpfh")
    res = (out,) + ((spfh,) if return_spfh else ()) + ((counts,) if return_counts else ())
    return res if len(res) > 1 else out


def fpfh(xyz, normals, radius, k=100, return_spfh=False, return_counts=False, search="knn",
         counts=None):
    """FPFH descriptors of b clouds from points and normals alone: neighbour
    lists, then fpfh_from_neighbors.  k counts the point itself, as the max_nn
    of Open3D's KDTreeSearchParamHybrid(radius, max_nn) does.  search="knn":
    the lists of knn_forward_cuda(xyz, xyz, min(k, 128)); search="grid": those
    of hybrid_search(xyz, radius, min(k, 128), counts), which
    also takes ragged clouds: counts [b] int32, cloud q's valid points are its
    first counts[q]; the points past them get zero descriptors."""
    _check(xyz, "xyz")
    _check(normals, "normals")
    k = min(int(k), 128)
    if k < 1:
        raise RuntimeError("fpfh: k must be at least 1")
    if search not in ("knn", "grid"):
        raise RuntimeError("fpfh: search must be 'knn' or 'grid' (got %r)" % (search,))
    if search == "knn":
        if counts is not None:
            raise RuntimeError("fpfh: counts needs search='grid'")
        dist, _, idx, _ = knn_forward_cuda(xyz, xyz, k)
    else:
        dist, idx, _ = hybrid_search(xyz, radius, k, counts)
    return fpfh_from_neighbors(xyz, normals, idx, dist, radius, return_spfh, return_counts)


# ------------------------------------- hybrid neighbour search (4.8g)
def hybrid_search(xyz, radius, k, counts=None, return_within=False):
    """Hybrid (radius + max_nn) neighbour search of b clouds against
    themselves (Open3D's KDTreeSearchParamHybrid(radius, max_nn), batched;
    DESIGN.md 4.8g, include/pcr_hybrid.h): xyz [b, 3, n], k <= 128 counting
    the point itself, counts [b] int32 -- cloud q's valid points are its first
    counts[q] -- or None for all n -> dist [b, k, n] (squared, knn_forward_cuda's
    distance bit for bit), idx [b, k, n] int32, count [b, n] int32: per query
    the valid points within `radius`, ascending by (distance, index), cut to
    k; unfilled slots hold (+inf, -1).  return_within: also within [b, n]
    int32, the points within the radius before the cut.  A query past its
    cloud's count, or with a non-finite coordinate, has an empty row.
    Bit-identical from run to run."""
    _check(xyz, "xyz")
    if xyz.dim() != 3 or xyz.shape[1] != 3 or xyz.shape[2] < 1:
        raise RuntimeError("hybrid_search: expected xyz [b, 3, n] with n >= 1")
    b, _, n = xyz.shape
    k = int(k)
    if k < 1 or k > 128:
        raise RuntimeError("hybrid_search: k must be in [1, 128] (got %d)" % k)
    _check_counts(counts, b, "counts", "hybrid_search: expected counts [b]")
    dev = xyz.device
    dist = torch.empty((b, k, n), dtype=torch.float32, device=dev)
    idx = torch.empty((b, k, n), dtype=torch.int32, device=dev)
    count = torch.empty((b, n), dtype=torch.int32, device=dev)
    within = torch.empty((b, n), dtype=torch.int32, device=dev) if return_within else None
    lib = _lib.load()
    ws = _workspace(lib.pcr_hybrid_search_workspace_size(b, n), dev)
    _lib.check(lib.pcr_hybrid_search(
        _ptr(xyz), _ptr(counts), b, n, k, float(radius), _ptr(dist), _ptr(idx), _ptr(count),
        _ptr(within), _ptr(ws), ws.numel(), _stream()), "hybrid_search")
    return (dist, idx, count, within) if return_within else (dist, idx, count)
