"""Input side of the path: the reference's on-disk point
format, the ModelNet40 sample pipeline around it, and GPU normals.

- ``read_xyzn_txt`` is the native parser of libpcr_amd.so for the
  ``modelnet40_normal_resampled/*.txt`` rows (datasets/modelnet40.py:30).
- ``ModelNet40Dataset`` mirrors ``_ModelNet40Dataset`` (datasets/modelnet40.py:
  11-95): the class list, the split files, random point choice, centring and
  the optional random rotation, returning ``(pcd [3|6, n], target)``.
- ``random_rotation`` keeps the reference's quirk (utils/open3d_func.py:85-87):
  it reseeds numpy with ``seed=0`` on every call, so every sample gets the
  same rotation.
- ``get_normals`` is utils/open3d_func.py:77-83 on the GPU
  (``ops.estimate_normals``, radius 0.1).
- ``grid_sub_sampling`` is utils/grid_subsampleing.py's wrapper of KPConv's
  grid subsampling on the GPU (``ops.grid_subsample``), for one numpy cloud;
  ``pad_clouds`` builds the ragged batch the op takes.

The DeepGMR h5 test files (datasets/deepgmr_mn40.py:46-49) need h5py, which
is not installed; they are out of reach here.
"""
import ctypes
import os

import numpy as np

from . import _lib


def read_xyzn_txt(path):
    """np.loadtxt(path, delimiter=',').astype(np.float32), natively: ->
    float32 array [rows, cols]."""
    lib = _lib.load()
    p = os.fsencode(path)
    rows, cols = ctypes.c_longlong(0), ctypes.c_int(0)
    _lib.check(lib.pcr_txt_shape(p, ctypes.byref(rows), ctypes.byref(cols)), "txt_shape")
    out = np.empty((rows.value, max(cols.value, 1)), np.float32)
    if rows.value:
        _lib.check(lib.pcr_read_xyzn_txt(p, out.ctypes.data, rows.value, cols.value),
                   "read_xyzn_txt")
    return out


def randchoice(n, m):
    """utils/random_choice.py:2-7."""
    return np.random.choice(n, m, replace=n < m)


def random_rotation(points, normals=None, max_degree=360, max_amp=3, seed=0):
    """utils/open3d_func.py:85-104: a rotation about a random axis plus a
    random translation, drawn after np.random.seed(seed)."""
    from scipy.spatial.transform import Rotation
    np.random.seed(seed)
    x = np.random.rand(6)
    degree = np.random.rand(1) * max_degree * np.pi / 180
    amp = np.random.rand(1) * max_amp
    w, v = x[:3] / np.linalg.norm(x[:3]), x[3:] / np.linalg.norm(x[3:])
    w = w * degree
    v = v * amp
    r = Rotation.from_rotvec(w)
    pts = r.apply(points) + v[np.newaxis, :]
    t = np.eye(4)
    t[:3, :3] = r.as_matrix()
    t[:3, 3] = v
    if normals is not None:
        return t, pts.astype(np.float32), r.apply(normals).astype(np.float32)
    return t, pts.astype(np.float32)


class ModelNet40Dataset:
    """datasets/modelnet40.py:11-95 without the 'fps' cache files (the
    reference's host FPS helper does not run: utils/random_choice.py:22 calls
    np.randint).  Returns (pcd [6 or 3, num_points] float32, target int)."""

    def __init__(self, datadir, partition, shapenum, num_points, normalize=True,
                 with_normals=True, random_rot=False):
        self.rootdir = datadir
        self.num_points = num_points
        self.normalize = normalize
        self.with_normals = with_normals
        self.random_rot = random_rot
        with open(os.path.join(datadir, "modelnet%s_shape_names.txt" % shapenum)) as f:
            classes = sorted(line.strip() for line in f)
        self.classes = classes
        class_to_idx = {c: i for i, c in enumerate(classes)}
        self.samples = []
        with open(os.path.join(datadir, "modelnet%s_%s.txt" % (shapenum, partition))) as f:
            for line in f:
                name = line.strip()
                cls = name[:-5]
                self.samples.append((os.path.join(cls, name), class_to_idx[cls]))

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        sample, target = self.samples[index]
        pc = read_xyzn_txt(os.path.join(self.rootdir, sample + ".txt"))
        idx = randchoice(pc.shape[0], self.num_points)
        points = pc[idx, :3].copy()
        normals = pc[idx, 3:].copy()
        if self.normalize:
            points -= np.mean(points, axis=0, keepdims=True)
        if self.random_rot:
            if self.with_normals:
                _, points, normals = random_rotation(points, normals)
                pcd = np.concatenate((points, normals), axis=1)
            else:
                _, pcd = random_rotation(points)
        else:
            pcd = np.concatenate((points, normals), axis=1) if self.with_normals else points
        return pcd.T, target


def get_normals(points, radius=0.1):
    """utils/open3d_func.py:77-83 on the GPU.  points: [n, 3] (numpy or
    tensor, one cloud, as the reference) or a [b, 3, n] CUDA tensor ->
    normals of the same layout; numpy input gives a float32 numpy result."""
    import torch
    from . import ops
    if isinstance(points, np.ndarray):
        dev = torch.device("cuda", torch.cuda.current_device())
        t = torch.from_numpy(np.ascontiguousarray(points.T, np.float32))[None].to(dev)
        return ops.estimate_normals(t, radius)[0].T.cpu().numpy()
    if points.dim() == 2:
        return ops.estimate_normals(points.t().contiguous()[None], radius)[0].t()
    return ops.estimate_normals(points.contiguous(), radius)


def pad_clouds(clouds):
    """A ragged batch for ``ops.grid_subsample``: clouds, a list of [3, n_i]
    arrays or tensors -> (xyz [b, 3, n_max] float32, zero padded; counts [b]
    int32).  Tensors in, tensors out (on the first cloud's device); numpy in,
    numpy out."""
    if len(clouds) == 0:
        raise ValueError("pad_clouds: no clouds")
    for x in clouds:
        if len(x.shape) != 2 or x.shape[0] != 3:
            raise ValueError("pad_clouds: expected [3, n] clouds, got %s" % (tuple(x.shape),))
    sizes = [int(x.shape[1]) for x in clouds]
    b, n = len(clouds), max(max(sizes), 1)
    if isinstance(clouds[0], np.ndarray):
        xyz = np.zeros((b, 3, n), np.float32)
        for q, x in enumerate(clouds):
            xyz[q, :, :sizes[q]] = x
        return xyz, np.asarray(sizes, np.int32)
    import torch
    dev = clouds[0].device
    xyz = torch.zeros((b, 3, n), dtype=torch.float32, device=dev)
    for q, x in enumerate(clouds):
        xyz[q, :, :sizes[q]] = x
    return xyz, torch.tensor(sizes, dtype=torch.int32, device=dev)


def grid_sub_sampling(points, features=None, labels=None, grid_size=0.1, verbose=0):
    """utils/grid_subsampleing.py grid_sub_sampling on the GPU
    (``ops.grid_subsample``): one cloud, points (N, 3) and features (N, d)
    numpy -> subsampled points (M, 3) float32, and features (M, d) when given.
    The cells come in ascending cell key (the reference's order is that of a
    hash map).  labels raise: the reference's majority vote breaks ties by
    hash-map order, which cannot be pinned; vote with ``cell_of`` of
    ``ops.grid_subsample`` instead."""
    import torch
    from . import ops
    del verbose
    if labels is not None:
        raise RuntimeError("grid_sub_sampling: labels are not supported (the reference's vote "
                           "breaks ties by hash-map order); vote with ops.grid_subsample's "
                           "cell_of")
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise RuntimeError("grid_sub_sampling: expected points (N, 3) with N >= 1")
    dev = torch.device("cuda", torch.cuda.current_device())
    xyz = torch.from_numpy(np.ascontiguousarray(points.T, np.float32))[None].to(dev)
    feat = None
    if features is not None:
        features = np.asarray(features)
        if features.ndim != 2 or features.shape[0] != points.shape[0]:
            raise RuntimeError("grid_sub_sampling: expected features (N, d)")
        feat = torch.from_numpy(np.ascontiguousarray(features.T, np.float32))[None].to(dev)
    out = ops.grid_subsample(xyz, grid_size, feat)
    if int(out["status"][0]) != 0:
        raise RuntimeError("grid_sub_sampling: status %d (2: a non-finite coordinate, 3: the "
                           "grid is finer than 2^20 cells along an axis)" % int(out["status"][0]))
    m = int(out["count"][0])
    sub = out["xyz"][0, :, :m].t().contiguous().cpu().numpy()
    if feat is None:
        return sub
    return sub, out["features"][0, :, :m].t().contiguous().cpu().numpy()
