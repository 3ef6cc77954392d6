"""CPU: the grid subsampling's ABI surface, its contract run in plain C loops on
include/pcr_gridsub.h (gcc) against the numpy restatement
(tests/gridsub_restate.py) bit for bit, hand-derived known answers, and the
Python mirrors' argument handling."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gridsub_restate as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("pcr_grid_subsample", "pcr_grid_subsample_workspace_size")
F = np.float32

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pcr_gridsub.h"

/* gridsub <file>: the whole contract for one cloud.  File: int n m c; float
 * dl; xyz [3][n]; features [c][n].  Prints status count / dims / origin bits /
 * cell_of [n] / cell_count [n] / xyz bits [3][n] / feature bits [c][n]. */
static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

static int cmp_u64(const void *a, const void *b) {
  const unsigned long long x = *(const unsigned long long *)a, y = *(const unsigned long long *)b;
  return x < y ? -1 : x > y;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
  int hd[3], n, m, c, i, d, s, status = 0, cells = 0, dims[3] = {0, 0, 0};
  float dl, origin[3] = {0, 0, 0}, *X, *Fe, *out;
  int *cell_of, *cell_count;
  unsigned long long *key, *uniq;
  if (!f || fread(hd, 4, 3, f) != 3 || fread(&dl, 4, 1, f) != 1) return 1;
  n = hd[0]; m = hd[1]; c = hd[2];
  X = malloc(12 * n); Fe = malloc(4 * (size_t)(c ? c : 1) * n);
  out = calloc((size_t)(3 + c) * n, 4);
  cell_of = malloc(4 * n); cell_count = calloc(n, 4);
  key = malloc(8 * n); uniq = malloc(8 * n);
  if (fread(X, 4, 3 * n, f) != (size_t)(3 * n) || fread(Fe, 4, (size_t)c * n, f) != (size_t)c * n)
    return 1;
  for (i = 0; i < n; i++) cell_of[i] = -1;
  if (m < 1 || m > n) {
    status = PCR_GRIDSUB_COUNT;
  } else {
    for (i = 0; i < m && !status; i++)
      for (d = 0; d < 3; d++)
        if (!pcr_gridsub_finite(X[d * n + i])) status = PCR_GRIDSUB_NONFINITE;
  }
  if (!status) {
    float mn[3], mx[3];
    for (d = 0; d < 3; d++) {
      unsigned lo = pcr_gridsub_ord(X[d * n]), hi = lo;
      for (i = 1; i < m; i++) {
        const unsigned u = pcr_gridsub_ord(X[d * n + i]);
        if (u < lo) lo = u;
        if (u > hi) hi = u;
      }
      mn[d] = pcr_gridsub_unord(lo);
      mx[d] = pcr_gridsub_unord(hi);
    }
    status = pcr_gridsub_grid(mn, mx, dl, origin, dims);
  }
  if (!status) {
    for (i = 0; i < m; i++) {
      key[i] = pcr_gridsub_key(pcr_gridsub_index(X[i], origin[0], dl),
                               pcr_gridsub_index(X[n + i], origin[1], dl),
                               pcr_gridsub_index(X[2 * n + i], origin[2], dl), dims[0], dims[1]);
      uniq[i] = key[i];
    }
    qsort(uniq, m, 8, cmp_u64);
    for (i = 0; i < m; i++)
      if (i == 0 || uniq[i] != uniq[i - 1]) uniq[cells++] = uniq[i];
    for (i = 0; i < m; i++) { /* ascending point index; out starts at 0.0f */
      int lo = 0, hi = cells - 1;
      while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (uniq[mid] < key[i]) lo = mid + 1; else hi = mid;
      }
      cell_of[i] = lo;
      cell_count[lo]++;
      for (d = 0; d < 3; d++) out[d * n + lo] += X[d * n + i];
      for (d = 0; d < c; d++) out[(3 + d) * n + lo] += Fe[d * n + i];
    }
    for (s = 0; s < cells; s++) {
      for (d = 0; d < 3; d++) out[d * n + s] = pcr_gridsub_xyz_mean(out[d * n + s], cell_count[s]);
      for (d = 0; d < c; d++)
        out[(3 + d) * n + s] = pcr_gridsub_feat_mean(out[(3 + d) * n + s], cell_count[s]);
    }
  } else if (status != PCR_GRIDSUB_TOO_FINE) {
    for (d = 0; d < 3; d++) { origin[d] = 0.0f; dims[d] = 0; }
  }
  printf("%d %d\n%d %d %d\n%u %u %u\n", status, cells, dims[0], dims[1], dims[2],
         bits(origin[0]), bits(origin[1]), bits(origin[2]));
  for (i = 0; i < n; i++) printf("%d ", cell_of[i]);
  printf("\n");
  for (i = 0; i < n; i++) printf("%d ", cell_count[i]);
  printf("\n");
  for (i = 0; i < 3 * n; i++) printf("%u ", bits(out[i]));
  printf("\n");
  for (i = 3 * n; i < (3 + c) * n; i++) printf("%u ", bits(out[i]));
  printf("\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("gridsub")
    src = d / "gridsub_host.c"
    src.write_text(PROGRAM)
    out = d / "gridsub_host"
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-I", INCLUDE, str(src), "-o",
                           str(out), "-lm"])
    return str(out)


def run_c(exe, path, xyz, cell, features=None, count=None):
    xyz = np.ascontiguousarray(xyz, F)
    n = xyz.shape[1]
    c = 0 if features is None else features.shape[0]
    feat = b"" if features is None else np.ascontiguousarray(features, F).tobytes()
    path.write_bytes(struct.pack("<3if", n, n if count is None else count, c, cell) +
                     xyz.tobytes() + feat)
    got = subprocess.check_output([exe, str(path)]).decode().split("\n")
    status, cells = (int(v) for v in got[0].split())

    def floats(line, shape):
        return np.array(line.split(), dtype=np.uint32).view(F).reshape(shape)
    return dict(status=status, count=cells, dims=np.array(got[1].split(), dtype=np.int32),
                origin=floats(got[2], (3,)), cell_of=np.array(got[3].split(), dtype=np.int32),
                cell_count=np.array(got[4].split(), dtype=np.int32), xyz=floats(got[5], (3, n)),
                features=None if features is None else floats(got[6], (c, n)))


# ------------------------------------------------------------------- ABI
def test_header_library_and_signatures_have_the_entry_points():
    from pcr_amd import _lib
    text = open(os.path.join(INCLUDE, "pcr_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text)
        assert hasattr(_lib.load(), name)
        assert name in _lib.SIGNATURES
    assert '#include "pcr_math.h"' in open(os.path.join(INCLUDE, "pcr_gridsub.h")).read()
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gridsub_scatter_kernel" in data and b"gridsub_sum_kernel" in data


def test_argument_checks_need_no_gpu():
    """a bad cell size and negative sizes are refused before anything touches
    the device (every pointer is a dummy)"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000
    names = ("xyz", "features", "counts", "out_xyz", "out_features", "out_count", "cell_of",
             "cell_count", "origin", "dims", "status", "ws")

    def call(b=2, n=100, c=3, cell=0.1, ws_bytes=1 << 30, **kw):
        a = dict({k: one for k in names}, **kw)
        return lib.pcr_grid_subsample(a["xyz"], a["features"], a["counts"], b, n, c, cell,
                                      a["out_xyz"], a["out_features"], a["out_count"],
                                      a["cell_of"], a["cell_count"], a["origin"], a["dims"],
                                      a["status"], a["ws"], ws_bytes, None)
    for cell in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert call(cell=cell) == -1, cell
        assert b"cell" in lib.pcr_last_error()
    assert call(b=-1) == -1 and call(n=-1) == -1 and call(c=-1) == -1
    assert call(n=0) == -1
    assert call(b=0) == 0
    for k in names:
        if k in ("counts",):
            continue
        assert call(**{k: None}) == -1, k
    need = lib.pcr_grid_subsample_workspace_size(2, 100, 3)
    assert need >= 2 * 100 * 28 and need % 256 == 0
    assert lib.pcr_grid_subsample_workspace_size(0, 100, 3) == 256
    assert call(ws_bytes=need - 1) == -1
    assert b"workspace" in lib.pcr_last_error()
    assert call(b=1 << 16, n=1 << 15) == -1  # b * n reaches 2^31


def test_python_mirrors():
    import torch
    from pcr_amd import io, ops
    x = torch.zeros((2, 3, 8))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.grid_subsample(x, 0.1)
    with pytest.raises(RuntimeError, match="labels"):
        io.grid_sub_sampling(np.zeros((8, 3), F), labels=np.zeros(8, np.int32))
    rng = np.random.default_rng(0)
    clouds = [rng.standard_normal((3, k)).astype(F) for k in (5, 9, 1)]
    xyz, counts = io.pad_clouds(clouds)
    assert xyz.shape == (3, 3, 9) and xyz.dtype == F
    assert counts.dtype == np.int32 and counts.tolist() == [5, 9, 1]
    for q, cl in enumerate(clouds):
        assert np.array_equal(xyz[q, :, :cl.shape[1]], cl)
        assert not xyz[q, :, cl.shape[1]:].any()
    txyz, tcounts = io.pad_clouds([torch.from_numpy(cl) for cl in clouds])
    assert tuple(txyz.shape) == (3, 3, 9) and tcounts.dtype == torch.int32
    assert np.array_equal(txyz.numpy(), xyz) and tcounts.tolist() == [5, 9, 1]
    with pytest.raises(ValueError):
        io.pad_clouds([np.zeros((4, 3), F)])


# -------------------------------------------------------------- contract
@pytest.mark.parametrize("seed,n,c,cell,spread", [
    (1, 1, 0, 0.1, 1.0), (2, 2, 1, 0.1, 1.0), (3, 65, 3, 0.3, 1.0), (4, 1000, 2, 0.25, 1.0),
    (5, 500, 67, 0.5, 1.0), (6, 700, 1, 0.013, 40.0), (7, 300, 0, 3.0, 0.01)])
def test_scalar_run_of_the_header_matches_the_restatement(exe, tmp_path, seed, n, c, cell,
                                                           spread):
    rng = np.random.default_rng(seed)
    xyz, feat = gr.random_cloud(rng, n, c, spread, shift=rng.uniform(-5, 5))
    exp = gr.grid_subsample(xyz, cell, feat)
    got = run_c(exe, tmp_path / "cloud.bin", xyz, cell, feat)
    gr.assert_same(got, exp, "seed %d" % seed)
    assert exp["status"] == 0 and 1 <= exp["count"] <= n
    assert exp["cell_count"].sum() == n


@pytest.mark.parametrize("name", list(gr.edge_clouds()))
def test_edge_clouds_match_the_restatement(exe, tmp_path, name):
    xyz, feat, cell = gr.edge_clouds()[name]
    n = xyz.shape[1]
    exp = gr.grid_subsample(xyz, cell, feat)
    got = run_c(exe, tmp_path / "cloud.bin", xyz, cell, feat)
    gr.assert_same(got, exp, name)
    assert exp["status"] == 0
    if name.startswith("one_cell"):
        assert exp["count"] == 1 and exp["cell_count"][0] == n
    if name == "own_cell":
        assert exp["count"] == n and (exp["cell_count"] == 1).all()
        # every barycentre is its point: x * (float)(1.0 / 1.0)
        order = np.argsort(exp["cell_of"])
        assert np.array_equal(exp["xyz"], xyz[:, order])
    if name == "duplicates":
        assert exp["count"] <= 40 and exp["cell_count"].max() >= 2
    if name == "keys64":
        assert int(exp["dims"][0]) * int(exp["dims"][1]) * int(exp["dims"][2]) > 1 << 32
    if name == "batches":
        assert sorted(exp["cell_count"][:exp["count"]].tolist()) == \
            [1, 7, 8, 9, 31, 32, 33, 40, 41, 64, 73]


def test_ragged_counts_and_statuses(exe, tmp_path):
    rng = np.random.default_rng(20)
    xyz, feat = gr.random_cloud(rng, 50, 2)
    for count, status in ((50, 0), (1, 0), (0, 1), (51, 1), (-3, 1)):
        exp = gr.grid_subsample(xyz, 0.5, feat, count)
        got = run_c(exe, tmp_path / "cloud.bin", xyz, 0.5, feat, count)
        gr.assert_same(got, exp, count)
        assert exp["status"] == status
        if status:
            assert exp["count"] == 0 and not exp["xyz"].any() and (exp["cell_of"] == -1).all()
        else:
            assert exp["cell_count"].sum() == count and (exp["cell_of"][count:] == -1).all()
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[1, 30] = bad
        for count, status in ((50, 2), (31, 2), (30, 0)):  # past the valid count: ignored
            exp = gr.grid_subsample(x, 0.5, feat, count)
            got = run_c(exe, tmp_path / "cloud.bin", x, 0.5, feat, count)
            gr.assert_same(got, exp, (bad, count))
            assert exp["status"] == status
    # a grid finer than 2^20 cells along an axis; the limit itself passes
    two = np.array([[0.0, 1.0], [0.0, 0.0], [0.0, 0.0]], F)
    for cell, status, nx in ((1e-7, 3, 10000001), (2.0 ** -20, 3, (1 << 20) + 1),
                             (2.0 ** -19, 0, (1 << 19) + 1), (1e-30, 3, (1 << 30) + 1)):
        exp = gr.grid_subsample(two, cell)
        got = run_c(exe, tmp_path / "cloud.bin", two, cell)
        gr.assert_same(got, exp, cell)
        assert exp["status"] == status and exp["dims"][0] == nx, (cell, exp["dims"])
    two[0, 1] = 1.0 - 2.0 ** -20
    exp = gr.grid_subsample(two, 2.0 ** -20)
    assert exp["status"] == 0 and exp["dims"][0] == 1 << 20 and exp["count"] == 2


# ---------------------------------------------------------- known answers
def bits(v):
    return int(np.asarray(v, F).view(np.uint32))


def test_three_points_two_cells(exe, tmp_path):
    """dl = 0.1, points x = 0.0, 0.05, 0.25 (y = z = 0): origin 0, NX = 3;
    cell 0 holds points 0 and 1, cell 2 point 2.  Barycentres: (0.0 + 0.05) *
    (float)0.5 = 0.025 exactly in fp32 terms (a halving), and 0.25 * 1."""
    xyz = np.array([[0.0, 0.05, 0.25], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], F)
    feat = np.array([[1.0, 2.0, 10.0]], F)
    for res in (gr.grid_subsample(xyz, 0.1, feat), run_c(exe, tmp_path / "c.bin", xyz, 0.1, feat)):
        assert res["status"] == 0 and res["count"] == 2
        assert res["dims"].tolist() == [3, 1, 1] and res["origin"].tolist() == [0.0, 0.0, 0.0]
        assert res["cell_of"].tolist() == [0, 0, 1] and res["cell_count"].tolist() == [2, 1, 0]
        assert bits(res["xyz"][0, 0]) == bits(F(0.05) * F(0.5))
        assert bits(res["xyz"][0, 1]) == bits(F(0.25))
        assert res["features"][0].tolist() == [1.5, 10.0, 0.0]
        assert not res["xyz"][1:].any() and res["xyz"][0, 2] == 0.0


def test_the_two_barycentre_rules_differ(exe, tmp_path):
    """a sum of 5.0 over 3 points: the coordinate is 5.0f * (float)(1.0 / 3.0)
    = 0x3FD55556 (1.6666667), the feature 5.0f / 3.0f = 0x3FD55555
    (1.6666666)"""
    xyz = np.array([[1.0, 2.0, 2.0], [1.0, 2.0, 2.0], [1.0, 2.0, 2.0]], F)
    feat = xyz[:1].copy()
    for res in (gr.grid_subsample(xyz, 4.0, feat), run_c(exe, tmp_path / "c.bin", xyz, 4.0, feat)):
        assert res["count"] == 1 and res["cell_count"][0] == 3
        assert [bits(v) for v in res["xyz"][:, 0]] == [0x3FD55556] * 3
        assert bits(res["features"][0, 0]) == 0x3FD55555


def test_origin_above_min_is_clamped(exe, tmp_path):
    """min = float32(4.7), dl = float32(0.1): origin = floorf(4.7f * 10.0f) *
    0.1f = 47 * 0.1f = 4.7000003 > min, so (min - origin) / dl floors to -1;
    the index is clamped to 0 and the point shares cell 0 with 4.75"""
    xyz, feat, cell = gr.edge_clouds()["clamp"]
    origin = F(np.floor(F(4.7) * (F(1.0) / F(0.1)))) * F(0.1)
    assert origin > F(4.7) and bits(origin) == 0x40966667
    assert np.floor((F(4.7) - origin) / F(0.1)) == -1.0
    for res in (gr.grid_subsample(xyz, cell, feat),
                run_c(exe, tmp_path / "c.bin", xyz, cell, feat)):
        assert res["status"] == 0 and bits(res["origin"][0]) == 0x40966667
        assert res["cell_of"][0] == 0 and res["cell_of"][1] == 0
        assert (res["cell_of"] >= 0).all() and (res["dims"] >= 1).all()
        assert res["dims"][1] == 1  # all y = min: clamped to one layer, not N = 0


def test_point_on_a_cell_face(exe, tmp_path):
    """dl = 0.25 (exact): x = 0.5 lies on the face between cells 1 and 2 and
    belongs to cell 2 (floor of exactly 2.0); x = 0.49999997 to cell 1"""
    below = np.nextafter(F(0.5), F(0.0))
    xyz = np.array([[0.0, below, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], F)
    for res in (gr.grid_subsample(xyz, 0.25), run_c(exe, tmp_path / "c.bin", xyz, 0.25)):
        assert res["dims"].tolist() == [3, 1, 1]
        assert res["cell_of"].tolist() == [0, 1, 2] and res["count"] == 3


def test_lone_negative_zero_sums_to_positive_zero(exe, tmp_path):
    xyz, feat, cell = gr.edge_clouds()["zeros"]
    for res in (gr.grid_subsample(xyz, cell, feat),
                run_c(exe, tmp_path / "c.bin", xyz, cell, feat)):
        assert res["count"] == 2
        assert bits(res["xyz"][1, 0]) == 0 and bits(res["features"][0, 1]) == 0
        assert bits(res["origin"][0]) == 0x80000000 and bits(res["origin"][2]) == 0
