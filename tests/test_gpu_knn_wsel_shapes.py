"""The transposed selection (knn_wsel_kernel) at the shapes where its LDS
staging of the cloud can go wrong, bit-exact against the oracle through the
extractor's entry points (pcr_knn_prepare + pcr_knn_select_ppf, workspace
and outputs poisoned: test_gpu_knn_select.check_sorted):

  - the workgroup's copy of the cloud is whole 1 KB pieces of rows of
    npad = 64 * ceil(n / 64) elements: clouds that end inside a 64-point
    block, on a block, one past it, inside and at the end of a 1 KB piece,
    and fewer points than k (everything past the row must read as NaN / -1);
  - both instantiations: <16, 12> (at most 4096 waves at 8 per block) and
    <16, 8> (more: nblk * b * 8 > 4096), the second also on ragged clouds;
  - ties, exact duplicates, NaN and far points through both.
"""
import functools

import numpy as np
import pytest

import oracle
from clouds import edge_clouds_for_knn, gaussian_clouds
from test_gpu_knn_select import check_sorted

pytestmark = pytest.mark.gpu


def narrow(b, n):
    """launch_wsel's choice: True = knn_wsel_kernel<16, 8>."""
    return ((n + 63) // 64) * b * 8 > 4096


def with_normals(xyz):
    xyz = np.array(xyz, dtype=np.float32, order="C")  # a copy: the shared references stay as they are
    return xyz, np.ascontiguousarray(np.roll(xyz, 1, axis=1))


@functools.lru_cache(maxsize=None)
def edge_base(n):
    """Three clouds of n points and their oracle ids for k = 32: a lattice with
    duplicates (ties at every distance), a lattice with NaN points and a far
    cluster (short lists), a Gaussian cloud with 100 copies of one point, a
    NaN coordinate and an outlier past 10000."""
    xyz = np.concatenate([edge_clouds_for_knn(2, n, seed=5),
                          gaussian_clouds(1, n, seed=13)[0]]).astype(np.float32)
    xyz[1, :, 3] = np.nan
    xyz[1, 2, n // 3] = np.nan
    xyz[1, :, n - 24:] += np.float32(500.0)
    xyz[2, :, 200:300] = xyz[2, :, 200:201]
    xyz[2, 0, 77] = np.nan
    xyz[2, :, n - 1] = (150.0, 0.0, 0.0)
    xyz = np.ascontiguousarray(xyz)
    xyz.setflags(write=False)
    ei = oracle.knn_forward(xyz, xyz, 32)[2]
    ei.setflags(write=False)
    return xyz, ei


@pytest.mark.parametrize("n,k", [(20, 32), (63, 32), (64, 32), (65, 32), (127, 32), (960, 32),
                                 (1001, 32), (1023, 32), (1024, 32), (65, 1), (1024, 1)])
def test_wsel_staging_tail(dev, n, k):
    """<16, 12>, two clouds: the end of the cloud against the 64-point blocks
    and the 1 KB copy pieces; n = 20 < k leaves unfilled slots (index 0)."""
    assert not narrow(2, n)
    xyz, nrm = with_normals(gaussian_clouds(2, n, seed=100 + n)[0])
    check_sorted(dev, xyz, nrm, k, oracle.knn_forward(xyz, xyz, k)[2])


@pytest.mark.parametrize("b,n,k", [(33, 1024, 32), (70, 500, 16)])
def test_wsel_pairs_instantiation(dev, b, n, k):
    """<16, 8>: the smallest batch of full clouds past the line (16 * 33 * 8 >
    4096), and ragged clouds (500 = 7 blocks + 52 points, npad = 512: two
    whole pieces)."""
    assert narrow(b, n)
    xyz, nrm = with_normals(gaussian_clouds(b, n, seed=b + n + k)[0])
    check_sorted(dev, xyz, nrm, k, oracle.knn_forward(xyz, xyz, k)[2])


@pytest.mark.parametrize("reps", [1, 11])
def test_wsel_edge_clouds(dev, reps):
    """Ties, duplicates, NaN and far points at n = 1024: three clouds through
    <16, 12>, and tiled to 33 clouds through <16, 8>."""
    xyz, ei = edge_base(1024)
    assert narrow(3 * reps, 1024) == (reps > 1)
    xyz, nrm = with_normals(np.tile(xyz, (reps, 1, 1)))
    check_sorted(dev, xyz, nrm, 32, np.ascontiguousarray(np.tile(ei, (reps, 1, 1))))


def test_wsel_edge_clouds_ragged(dev):
    """The same kinds of cloud ending inside a block (n = 700), k = 32."""
    xyz, ei = edge_base(700)
    xyz, nrm = with_normals(xyz)
    check_sorted(dev, xyz, nrm, 32, np.array(ei))
