"""CPU: the FPFH descriptors' ABI surface, the contract run in plain C loops on
include/pcr_fpfh.h (gcc) against the numpy restatement (tests/fpfh_restate.py)
bit for bit, hand-derived known answers, rotation invariance, and the Python
wrappers' argument handling."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fpfh_restate as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("pcr_fpfh", "pcr_fpfh_workspace_size")
F = np.float32

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "pcr_fpfh.h"

/* fpfh <file>: the whole contract in plain loops.  File: int b n k; float
 * radius; xyz [b][3][n]; normals [b][3][n]; idx [b][k][n]; dist [b][k][n].
 * Writes fpfh [b][33][n], spfh [b][33][n] (floats) and count [b][n] (ints) to
 * stdout as raw bytes. */
int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
  int hd[3], b, n, k, kk, q, i, s, c, g, a;
  float radius, r2, *X, *N, *D, *out, *sp;
  int *I, *cnt;
  size_t pts, lst;
  if (!f || fread(hd, 4, 3, f) != 3 || fread(&radius, 4, 1, f) != 1) return 1;
  b = hd[0]; n = hd[1]; k = hd[2];
  kk = k < n ? k : n;
  r2 = radius * radius;
  pts = (size_t)b * 3 * n; lst = (size_t)b * k * n;
  X = malloc(4 * pts); N = malloc(4 * pts); I = malloc(4 * lst); D = malloc(4 * lst);
  out = malloc(4 * (size_t)b * 33 * n); sp = malloc(4 * (size_t)b * 33 * n);
  cnt = malloc(4 * (size_t)b * n);
  if (fread(X, 4, pts, f) != pts || fread(N, 4, pts, f) != pts || fread(I, 4, lst, f) != lst ||
      fread(D, 4, lst, f) != lst)
    return 1;
  for (q = 0; q < b; q++) {
    const float *x = X + (size_t)q * 3 * n, *nr = N + (size_t)q * 3 * n;
    const int *idx = I + (size_t)q * k * n;
    const float *dist = D + (size_t)q * k * n;
    float *S = sp + (size_t)q * 33 * n, *O = out + (size_t)q * 33 * n;
    for (i = 0; i < n; i++) {
      int h[33] = {0}, m = 0;
      float pi[3], ni[3];
      for (a = 0; a < 3; a++) { pi[a] = x[a * n + i]; ni[a] = nr[a * n + i]; }
      for (s = 0; s < kk; s++) {
        const int j = idx[s * n + i];
        float pj[3], nj[3], ft[3];
        int ch[3];
        if (!pcr_fpfh_in_set(j, dist[s * n + i], i, n, r2)) continue;
        for (a = 0; a < 3; a++) { pj[a] = x[a * n + j]; nj[a] = nr[a * n + j]; }
        pcr_fpfh_pair(pi, ni, pj, nj, ft);
        pcr_fpfh_bins(ft, ch);
        h[ch[0]]++; h[ch[1]]++; h[ch[2]]++;
        m++;
      }
      for (c = 0; c < 33; c++) S[c * n + i] = pcr_fpfh_spfh(h[c], m);
      cnt[(size_t)q * n + i] = m;
    }
    for (i = 0; i < n; i++) {
      float acc[33];
      for (c = 0; c < 33; c++) acc[c] = 0.0f;
      for (s = 0; s < kk; s++) {
        const int j = idx[s * n + i];
        const float d = dist[s * n + i];
        if (!pcr_fpfh_in_set(j, d, i, n, r2)) continue;
        for (c = 0; c < 33; c++) acc[c] = pcr_fpfh_add(acc[c], S[c * n + j], d);
      }
      for (g = 0; g < 3; g++) {
        const float sum = pcr_fpfh_group_sum(acc + 11 * g);
        for (c = 11 * g; c < 11 * g + 11; c++)
          O[c * n + i] = pcr_fpfh_value(acc[c], sum, S[c * n + i]);
      }
    }
  }
  fwrite(out, 4, (size_t)b * 33 * n, stdout);
  fwrite(sp, 4, (size_t)b * 33 * n, stdout);
  fwrite(cnt, 4, (size_t)b * n, stdout);
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("fpfh")
    src = d / "fpfh_host.c"
    src.write_text(PROGRAM)
    out = d / "fpfh_host"
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-I", INCLUDE, str(src), "-o",
                           str(out), "-lm"])
    return str(out)


def run_c(exe, path, xyz, normals, idx, dist, radius):
    """-> fpfh [b, 33, n], spfh [b, 33, n], nbr_count [b, n]"""
    b, _, n = xyz.shape
    k = idx.shape[1]
    path.write_bytes(struct.pack("<3if", b, n, k, radius) +
                     np.ascontiguousarray(xyz, F).tobytes() +
                     np.ascontiguousarray(normals, F).tobytes() +
                     np.ascontiguousarray(idx, np.int32).tobytes() +
                     np.ascontiguousarray(dist, F).tobytes())
    raw = subprocess.check_output([exe, str(path)])
    m = b * 33 * n
    assert len(raw) == 4 * (2 * m + b * n)
    return (np.frombuffer(raw, F, m).reshape(b, 33, n),
            np.frombuffer(raw, F, m, 4 * m).reshape(b, 33, n),
            np.frombuffer(raw, np.int32, b * n, 8 * m).reshape(b, n))


def both(exe, path, xyz, normals, idx, dist, radius):
    """the restatement's and the header's results, after checking that they
    are the same bits"""
    exp = fr.fpfh(xyz, normals, idx, dist, radius)
    got = run_c(exe, path, xyz, normals, idx, dist, radius)
    for g, e, name in zip(got, exp, ("fpfh", "spfh", "nbr_count")):
        fr.assert_same_bits(g, e, name)
    return exp


# ------------------------------------------------------------------- ABI
def test_header_library_and_signatures_have_the_entry_points():
    from pcr_amd import _lib
    text = open(os.path.join(INCLUDE, "pcr_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text)
        assert hasattr(_lib.load(), name)
        assert name in _lib.SIGNATURES
    assert '#include "pcr_math.h"' in open(os.path.join(INCLUDE, "pcr_fpfh.h")).read()
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"fpfh_spfh_kernel" in data and b"fpfh_fpfh_kernel" in data


def test_argument_checks_need_no_gpu():
    """bad sizes and radii are refused before anything touches the device
    (every pointer is a dummy)"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000
    names = ("xyz", "normals", "idx", "dist", "fpfh", "spfh", "count", "ws")

    def call(b=2, n=100, k=16, radius=0.3, ws_bytes=1 << 30, **kw):
        a = dict({key: one for key in names}, **kw)
        return lib.pcr_fpfh(a["xyz"], a["normals"], a["idx"], a["dist"], b, n, k, radius,
                            a["fpfh"], a["spfh"], a["count"], a["ws"], ws_bytes, None)
    for radius in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert call(radius=radius) == -1, radius
        assert b"radius" in lib.pcr_last_error()
    assert call(b=-1) == -1 and call(n=0) == -1 and call(n=-1) == -1
    assert call(k=0) == -1 and call(k=129) == -1 and call(k=-1) == -1
    assert b"k must be" in lib.pcr_last_error()
    assert call(b=0) == 0
    assert call(b=0, k=0) == -1 and call(b=0, radius=0.0) == -1 and call(b=0, n=0) == -1
    for key in ("xyz", "normals", "idx", "dist", "fpfh", "ws"):
        assert call(**{key: None}) == -1, key
    need = lib.pcr_fpfh_workspace_size(2, 100)
    assert need >= 2 * 100 * (33 + 6) * 4 and need % 256 == 0
    assert lib.pcr_fpfh_workspace_size(0, 100) == 256
    assert call(ws_bytes=need - 1) == -1
    assert b"workspace" in lib.pcr_last_error()
    assert call(b=1 << 12, n=1 << 13, k=64) == -1  # b * k * n reaches 2^31


def test_wrappers_reject_cpu_tensors():
    import torch
    from pcr_amd import ops, registration
    x = torch.zeros((2, 3, 8))
    idx = torch.zeros((2, 4, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.fpfh(x, x, 0.3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.fpfh_from_neighbors(x, x, idx, torch.zeros((2, 4, 8)), 0.3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        registration.fpfh_pairs(x, x, x, x, 0.3)


# -------------------------------------------------------------- contract
@pytest.mark.parametrize("b,n,k,radius", fr.SHAPES)
def test_scalar_run_of_the_header_matches_the_restatement(exe, tmp_path, b, n, k, radius):
    xyz, nrm, idx, dist = fr.shape_inputs(b, n, k)
    fp, sp, cnt = both(exe, tmp_path / "in.bin", xyz, nrm, idx, dist, radius)
    assert np.isfinite(fp).all() and (cnt <= min(k, n) - 1).all()
    # every neighbour counts once per group of 11 bins
    for g in range(3):
        tot = sp[:, 11 * g:11 * g + 11].sum(axis=1)
        assert np.allclose(tot, np.where(cnt > 0, 100.0, 0.0), atol=1e-3)
    if n >= 63:
        assert cnt.max() >= 1


def test_salted_lists_and_a_nan_normal(exe, tmp_path):
    """-1, n, INT_MAX and NaN distances in the lists are skipped; a NaN normal
    changes only the point itself and the points that list it"""
    xyz, nrm, idx, dist, radius = fr.salted_inputs()
    both(exe, tmp_path / "in.bin", xyz, nrm, idx, dist, radius)
    xyz, nrm, idx, dist = fr.shape_inputs(1, 300, 33)
    clean = both(exe, tmp_path / "in.bin", xyz, nrm, idx, dist, 0.45)
    bad = nrm.copy()
    bad[0, 1, 17] = np.nan
    dirty = both(exe, tmp_path / "in.bin", xyz, bad, idx, dist, 0.45)
    assert np.isfinite(dirty[0]).all()
    listing = fr.listers(idx[0], dist[0], 300, 0.45, 17)
    assert 3 <= listing.sum() < 150
    spfh_changed = (clean[1][0] != dirty[1][0]).any(axis=0)
    assert spfh_changed[17] and not (spfh_changed & ~listing).any()
    # the FPFH mixes the neighbours' SPFH: one more ring
    ring = listing.copy()
    for p in np.nonzero(listing)[0]:
        ring |= fr.listers(idx[0], dist[0], 300, 0.45, p)
    assert not ((clean[0][0] != dirty[0][0]).any(axis=0) & ~ring).any()
    assert np.array_equal(clean[2], dirty[2])


# ---------------------------------------------------------- known answers
def test_planar_grid_with_constant_normals(exe, tmp_path):
    """Points of a plane with the plane's normal: a1 = a2 = 0, no swap, f2 = 0;
    v = dp x n lies in the plane, so f1 = v . n = 0; w = n x v lies in the
    plane, so f0 = atan2(0, 1) = 0.  floor(11 * (0 + pi) / (2 pi)) =
    floor(11 * (0 + 1) / 2) = floor(5.5) = 5: every pair counts in channels 5,
    16 and 27.  spfh is exactly 100.0 there; fpfh = acc * (100 / acc) + 100,
    200 to within an ulp of 100 plus the rounding of the sum (2e-5)."""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij")).reshape(2, -1)
    xyz = np.zeros((1, 3, 36), F)
    xyz[0, :2] = g * F(0.1)
    nrm = np.zeros((1, 3, 36), F)
    nrm[0, 2] = 1.0
    dist, idx = fr.knn(xyz, 16)
    fp, sp, cnt = both(exe, tmp_path / "in.bin", xyz, nrm, idx, dist, 0.25)
    assert cnt.min() == 7 and cnt.max() == 15  # a corner's and an inner point's
    hot = np.zeros(33, bool)
    hot[[5, 16, 27]] = True
    assert (sp[0, hot] == F(100.0)).all() and (sp[0, ~hot] == 0).all()
    assert np.abs(fp[0, hot] - 200.0).max() <= 2e-5 and (fp[0, ~hot] == 0).all()


def test_two_points_alone(exe, tmp_path):
    """n = 2: each point's only neighbour is the other, m = 1; every group of
    bins holds exactly one 100.0 and the FPFH one 200.0 (100 / d * (100 / (100
    / d)) is 100 to an ulp)"""
    xyz = np.array([[[0.0, 0.3], [0.0, 0.1], [0.0, -0.2]]], F)
    nrm = np.array([[[0.0, 0.6], [0.0, 0.0], [1.0, 0.8]]], F)
    dist, idx = fr.knn(xyz, 2)
    fp, sp, cnt = both(exe, tmp_path / "in.bin", xyz, nrm, idx, dist, 1.0)
    assert cnt.tolist() == [[1, 1]]
    for i in range(2):
        for g in range(3):
            assert sorted(sp[0, 11 * g:11 * g + 11, i].tolist()) == [0.0] * 10 + [100.0]
        assert np.array_equal(fp[0, :, i] != 0, sp[0, :, i] != 0)
        assert np.abs(fp[0, sp[0, :, i] != 0, i] - 200.0).max() <= 2e-5
    # a radius below their distance: nobody, all zero
    fp, sp, cnt = both(exe, tmp_path / "in.bin", xyz, nrm, idx, dist, 0.3)
    assert not cnt.any() and not fp.any() and not sp.any()


def test_an_exact_duplicate_is_not_a_neighbour(exe, tmp_path):
    """d = 0 fails 0 < d: points 0 and 1 coincide, so each has the other three
    points as neighbours, not its twin"""
    xyz = np.array([[[0.0, 0.0, 0.2, 0.1, -0.1], [0.0, 0.0, 0.1, -0.2, 0.1],
                     [0.0, 0.0, 0.0, 0.1, 0.2]]], F)
    nrm = np.zeros((1, 3, 5), F)
    nrm[0, 2] = 1.0
    dist, idx = fr.knn(xyz, 5)
    assert dist[0, 1, 0] == 0 and dist[0, 1, 1] == 0
    fp, sp, cnt = both(exe, tmp_path / "in.bin", xyz, nrm, idx, dist, 1.0)
    assert cnt.tolist() == [[3, 3, 4, 4, 4]]
    assert np.array_equal(sp[0, :, 0], sp[0, :, 1]) and np.array_equal(fp[0, :, 0], fp[0, :, 1])


# ------------------------------------------------------ rotation invariance
# the largest difference between the features of the surface and of its moved
# copy, as the restatement measures it on this input: two ulps of 200 (every
# bin count agrees; the sums of spfh / d differ by the fp32 rounding of the moved
# coordinates)
MEASURED_DIFF = 3.05e-5


def test_rotation_invariance(exe, tmp_path):
    """n = 256, k = 24, r = 0.35: the moved, permuted copy has the same
    neighbour counts, features within 10 x the measured difference, and at
    least 95 % of the points are mutual nearest neighbours of their copy"""
    n, k, r = 256, 24, 0.35
    xyz, nrm = fr.surface(n, seed=5)
    x2, n2, perm, _ = fr.moved_copy(xyz, nrm, seed=6)
    d1, i1 = fr.knn(xyz[None], k)
    d2, i2 = fr.knn(x2[None], k)
    fa, _, ca = both(exe, tmp_path / "a.bin", xyz[None], nrm[None], i1, d1, r)
    fb, _, cb = both(exe, tmp_path / "b.bin", x2[None], n2[None], i2, d2, r)
    assert np.array_equal(cb[0], ca[0][perm])
    diff = float(np.abs(fb[0] - fa[0][:, perm]).max())
    print("rotation invariance: measured feature difference %.3g" % diff)
    assert diff <= 10 * MEASURED_DIFF
    m1, m2 = fr.mutual_nn(fa[0], fb[0])
    # the numpy matcher counts what the matching's C oracle counts
    import oracle
    _, _, o1, o2, oc = oracle.mutual_nn(np.ascontiguousarray(fa.transpose(0, 2, 1)),
                                        np.ascontiguousarray(fb.transpose(0, 2, 1)))
    assert oc[0] == len(m1) and np.array_equal(o1[0, :oc[0]], m1)
    assert np.array_equal(o2[0, :oc[0]], m2)
    right = int((perm[m2] == m1).sum())
    print("rotation invariance: %d of %d points mutual and correct" % (right, n))
    assert right >= 0.95 * n
