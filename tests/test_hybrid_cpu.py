"""CPU: the hybrid neighbour search's ABI surface and argument checks, the
numpy restatement (tests/hybrid_restate.py: brute force over all pairs)
against np_restate.knn_dir, and the grid algorithm -- bounds, cells, 27-cell
scan, key selection -- run in plain C loops on include/pcr_hybrid.h (gcc)
against the restatement bit for bit, on every input the GPU tests use.  The
C run is what checks the cell-edge logic without a GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import hybrid_restate as hr
from oracle import np_restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("pcr_hybrid_search", "pcr_hybrid_search_workspace_size")
F = np.float32

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pcr_gridsub.h"
#include "pcr_hybrid.h"

/* hybrid <file>: the grid algorithm for one cloud.  File: int n m k; float
 * radius; xyz [3][n].  Prints dims / then per point: nbr_count within, k
 * (distance bits, index) pairs. */
static int cmp_u64(const void *a, const void *b) {
  const unsigned long long x = *(const unsigned long long *)a, y = *(const unsigned long long *)b;
  return x < y ? -1 : x > y;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
  int hd[3], n, m, k, i, d, s, any = 0, dims[3], g, nc, *cellof, *start, *fill, *order;
  float radius, r2, mn[3], mx[3], origin[3], inv, *X;
  unsigned lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  unsigned long long *keys;
  if (!f || fread(hd, 4, 3, f) != 3 || fread(&radius, 4, 1, f) != 1) return 1;
  n = hd[0]; m = hd[1]; k = hd[2];
  m = m < 0 ? 0 : (m > n ? n : m);
  X = malloc(12 * (size_t)n);
  if (fread(X, 4, 3 * (size_t)n, f) != 3 * (size_t)n) return 1;
  r2 = radius * radius;
  /* bounds of the valid points with finite coordinates */
  for (i = 0; i < m; i++) {
    if (!pcr_hybrid_finite3(X[i], X[n + i], X[2 * n + i])) continue;
    for (d = 0; d < 3; d++) {
      const unsigned u = pcr_gridsub_ord(X[d * n + i]);
      if (!any || u < lo[d]) lo[d] = u;
      if (!any || u > hi[d]) hi[d] = u;
    }
    any = 1;
  }
  for (d = 0; d < 3; d++) {
    mn[d] = pcr_gridsub_unord(lo[d]);
    mx[d] = pcr_gridsub_unord(hi[d]);
  }
  g = pcr_hybrid_gmax(n);
  pcr_hybrid_grid(mn, mx, any, radius, g, origin, &inv, dims);
  nc = dims[0] * dims[1] * dims[2];
  /* cells, their populations and first positions, the points in cell order */
  cellof = malloc(4 * (size_t)n);
  start = calloc((size_t)nc + 1, 4);
  fill = calloc((size_t)nc, 4);
  order = malloc(4 * (size_t)n);
  keys = malloc(8 * (size_t)n);
  for (i = 0; i < n; i++) {
    cellof[i] = -1;
    if (i < m && pcr_hybrid_finite3(X[i], X[n + i], X[2 * n + i])) {
      const int cx = pcr_hybrid_cell(X[i], origin[0], inv, dims[0]);
      const int cy = pcr_hybrid_cell(X[n + i], origin[1], inv, dims[1]);
      const int cz = pcr_hybrid_cell(X[2 * n + i], origin[2], inv, dims[2]);
      cellof[i] = cx + dims[0] * (cy + dims[1] * cz);
      start[cellof[i] + 1]++;
    }
  }
  for (s = 0; s < nc; s++) start[s + 1] += start[s];
  for (i = 0; i < n; i++)
    if (cellof[i] >= 0) order[start[cellof[i]] + fill[cellof[i]]++] = i;
  printf("%d %d %d\n", dims[0], dims[1], dims[2]);
  for (i = 0; i < n; i++) {
    int within = 0, cnt;
    if (cellof[i] >= 0) {
      const int cx = cellof[i] % dims[0], cy = (cellof[i] / dims[0]) % dims[1];
      const int cz = cellof[i] / (dims[0] * dims[1]);
      int dy, dz, p;
      for (dz = -1; dz <= 1; dz++)
        for (dy = -1; dy <= 1; dy++) {
          const int yy = cy + dy, zz = cz + dz;
          int x0 = cx - 1, x1 = cx + 1, base;
          if (yy < 0 || yy >= dims[1] || zz < 0 || zz >= dims[2]) continue;
          if (x0 < 0) x0 = 0;
          if (x1 > dims[0] - 1) x1 = dims[0] - 1;
          base = dims[0] * (yy + dims[1] * zz);
          for (p = start[base + x0]; p < start[base + x1 + 1]; p++) {
            const int j = order[p];
            const float dd = pcr_hybrid_dist(X[i], X[n + i], X[2 * n + i], X[j], X[n + j],
                                             X[2 * n + j]);
            if (pcr_hybrid_in_radius(dd, r2)) keys[within++] = pcr_hybrid_key(dd, j);
          }
        }
      qsort(keys, within, 8, cmp_u64);
    }
    cnt = within < k ? within : k;
    printf("%d %d", cnt, within);
    for (s = 0; s < k; s++) {
      const unsigned long long key = s < cnt ? keys[s] : PCR_HYBRID_EMPTY;
      printf(" %u %d", pcr_hybrid_bits(pcr_hybrid_key_dist(key)), pcr_hybrid_key_index(key));
    }
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("hybrid")
    src = d / "hybrid_host.c"
    src.write_text(PROGRAM)
    out = d / "hybrid_host"
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-I", INCLUDE, str(src), "-o",
                           str(out), "-lm"])
    return str(out)


def run_c(exe, path, xyz, radius, k, count=None):
    """one cloud [3, n] -> dims, (dist [k, n], idx [k, n], nbr_count [n], within [n])"""
    xyz = np.ascontiguousarray(xyz, F)
    n = xyz.shape[1]
    path.write_bytes(struct.pack("<3if", n, n if count is None else int(count), k, radius) +
                     xyz.tobytes())
    lines = subprocess.check_output([exe, str(path)]).decode().split("\n")
    dims = [int(v) for v in lines[0].split()]
    rows = np.array([ln.split() for ln in lines[1:n + 1]], dtype=np.int64)
    assert rows.shape == (n, 2 + 2 * k)
    dist = rows[:, 2::2].astype(np.uint32).view(F).T
    idx = rows[:, 3::2].astype(np.int32).T
    return dims, (np.ascontiguousarray(dist), np.ascontiguousarray(idx),
                  rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32))


# ------------------------------------------------------------------- ABI
def test_header_library_and_signatures_have_the_entry_points():
    from pcr_amd import _lib
    text = open(os.path.join(INCLUDE, "pcr_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text)
        assert hasattr(_lib.load(), name)
        assert name in _lib.SIGNATURES
    head = open(os.path.join(INCLUDE, "pcr_hybrid.h")).read()
    assert '#include "pcr_math.h"' in head
    assert re.search(r"#define\s+PCR_HYBRID_WAVE_CAP\s+\d+", head)
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"hybrid_query_kernel" in data and b"hybrid_scatter_kernel" in data


def test_argument_checks_need_no_gpu():
    """a bad radius, k outside [1, 128] and sizes that overflow are refused
    before anything touches the device (every pointer is a dummy)"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000
    names = ("xyz", "counts", "dist", "idx", "count", "within", "ws")

    def call(b=2, n=100, k=16, radius=0.1, ws_bytes=1 << 30, **kw):
        a = dict({key: one for key in names}, **kw)
        return lib.pcr_hybrid_search(a["xyz"], a["counts"], b, n, k, radius, a["dist"], a["idx"],
                                     a["count"], a["within"], a["ws"], ws_bytes, None)
    for radius in (0.0, -0.1, float("nan"), float("inf"), -float("inf"), 1e20, 3e38):
        assert call(radius=radius) == -1, radius  # 1e20: radius * radius is not finite
        assert b"radius" in lib.pcr_last_error()
    for k in (0, -1, 129, 1 << 20):
        assert call(k=k) == -1, k
        assert b"k must be" in lib.pcr_last_error()
    assert call(b=-1) == -1 and call(n=0) == -1 and call(n=-1) == -1
    assert call(b=0) == 0
    for key in ("xyz", "dist", "idx", "count", "ws"):
        assert call(**{key: None}) == -1, key
    need = lib.pcr_hybrid_search_workspace_size(2, 100)
    assert need >= 2 * 100 * 20 and need % 256 == 0
    assert lib.pcr_hybrid_search_workspace_size(0, 100) == 256
    assert call(ws_bytes=need - 1) == -1
    assert b"workspace" in lib.pcr_last_error()
    assert call(b=1 << 10, n=1 << 14, k=128) == -1  # b * k * n reaches 2^31
    assert b"too large" in lib.pcr_last_error()


def test_python_mirrors():
    import torch
    from pcr_amd import ops, registration
    import inspect
    x = torch.zeros((2, 3, 8))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.hybrid_search(x, 0.1, 4)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.fpfh(x, x, 0.1, search="grid")
    sig = inspect.signature(ops.fpfh).parameters
    assert sig["search"].default == "knn" and sig["counts"].default is None
    assert sig["k"].default == 100
    assert inspect.signature(registration.fpfh_pairs).parameters["search"].default == "knn"
    assert list(inspect.signature(ops.hybrid_search).parameters) == \
        ["xyz", "radius", "k", "counts", "return_within"]


# ----------------------------------------------- restatement against the KNN
@pytest.mark.parametrize("seed,n,k,radius", [(1, 1, 1, 0.5), (2, 40, 8, 0.3), (3, 97, 32, 0.4),
                                             (4, 97, 100, 0.25), (5, 64, 16, 50.0)])
def test_restatement_rows_are_the_knn_rows_within_the_radius(seed, n, k, radius):
    """finite inputs, full counts, r2 < 10000: every slot below nbr_count is
    knn_dir's slot, and knn_dir's next slot, where it has one, is beyond r2"""
    rng = np.random.default_rng(seed)
    xyz = np.stack([hr.cube(rng, n), hr.cube(rng, n, 3.0, -1.0)])
    r2 = F(radius) * F(radius)
    assert r2 < 10000
    dist, idx, cnt, within = hr.search(xyz, radius, k)
    kd, ki = np_restate.knn_dir(xyz, xyz, k)
    assert cnt.min() >= 1 and (within >= cnt).all()
    for q in range(2):
        for i in range(n):
            c = cnt[q, i]
            assert np.array_equal(idx[q, :c, i], ki[q, :c, i])
            assert np.array_equal(dist[q, :c, i].view(np.uint32), kd[q, :c, i].view(np.uint32))
            assert (idx[q, c:, i] == -1).all() and np.isposinf(dist[q, c:, i]).all()
            if c < min(k, n):
                assert kd[q, c, i] > r2
            else:
                assert within[q, i] >= c
    if radius == 50.0:
        assert (cnt == min(k, n)).all() and (within == n).all()


# --------------------------------------------------- grid against brute force
CASE_K = [(name, k) for name, (_, _, ks, _) in hr.cases().items() for k in ks]


@pytest.mark.parametrize("name,k", CASE_K)
def test_grid_run_of_the_header_matches_brute_force(exe, tmp_path, name, k):
    xyz, radius, _, counts = hr.cases()[name]
    exp = hr.expected(name, k)
    cells = 0
    for q in range(xyz.shape[0]):
        count = None if counts is None else counts[q]
        dims, got = run_c(exe, tmp_path / "cloud.bin", xyz[q], radius, k, count)
        hr.assert_same(got, tuple(e[q] for e in exp), (name, k, q))
        cells = max(cells, dims[0] * dims[1] * dims[2])
        assert max(dims) <= 32
    if name in ("overflow", "huge"):
        assert cells == 1
    if name.startswith("lattice") or name in ("both", "tiny_radius", "far_from_origin"):
        assert cells >= 27, (name, cells)


@pytest.mark.parametrize("name", list(hr.cases()))
def test_the_inputs_reach_their_branches(name):
    """asserted on the restatement: what each input is there for"""
    hr.assert_reaches(name)
