"""CPU: the point-to-plane ICP's ABI surface, its contract run in plain C loops
on include/pcr_icp_plane.h (gcc) against the numpy restatement
(tests/icp_plane_restate.py), and the conditions the fixtures of the GPU tests
rest on, checked on the restatement alone."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import icp_plane_restate as pr
import icp_restate as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAME = "pcr_icp_point_to_plane"

PROGRAM = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "pcr_math.h"
#include "pcr_rigid.h"
#include "pcr_icp_plane.h"

/* The whole contract for one pair.  File: int n1 n2 max_iters; float
 * max_dist; double rel_fitness rel_rmse; double init[16]; xyz1 [3][n1];
 * xyz2 [3][n2]; normals2 [3][n2]. */
static int N1, N2;
static float *X1, *X2, *NR, TAU2;
static int *CORR;
static int M;
static double FIT, RMSE, SUMS[PCR_ICP_PLANE_NSUM];

static void evaluate(const double *R, const double *t) {
  float T[12];
  double e = 0.0;
  int i, j;
  pcr_rigid_round(R, t, T);
  M = 0;
  for (i = 0; i < PCR_ICP_PLANE_NSUM; i++) SUMS[i] = 0.0;
  for (i = 0; i < N1; i++) {
    float m[3], best = INFINITY;
    int bj = -1;
    pcr_rigid_apply(T, X1[i], X1[N1 + i], X1[2 * N1 + i], m);
    for (j = 0; j < N2; j++) {
      const float d = pcr_sumsq3f(m[0] - X2[j], m[1] - X2[N2 + j], m[2] - X2[2 * N2 + j]);
      if (d < best) {
        best = d;
        bj = j;
      }
    }
    if (bj >= 0 && best <= TAU2) {
      float b[3], n[3];
      int d;
      for (d = 0; d < 3; d++) {
        b[d] = X2[d * N2 + bj];
        n[d] = NR[d * N2 + bj];
      }
      CORR[i] = bj;
      M++;
      e += (double)best;
      pcr_icp_plane_accumulate(m, b, n, SUMS);
    } else {
      CORR[i] = -1;
    }
  }
  FIT = (double)M / N1;
  RMSE = M ? sqrt(e / M) : 0.0;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
  int hd[3], it = 0, status = 2, i, d;
  float md;
  double tol[2], init[16], R[9], t[3];
  if (!f) return 1;
  if (fread(hd, 4, 3, f) != 3 || fread(&md, 4, 1, f) != 1 || fread(tol, 8, 2, f) != 2 ||
      fread(init, 8, 16, f) != 16) return 1;
  N1 = hd[0]; N2 = hd[1];
  X1 = malloc(12 * N1); X2 = malloc(12 * N2); NR = malloc(12 * N2); CORR = malloc(4 * N1);
  if (fread(X1, 4, 3 * N1, f) != (size_t)(3 * N1) || fread(X2, 4, 3 * N2, f) != (size_t)(3 * N2) ||
      fread(NR, 4, 3 * N2, f) != (size_t)(3 * N2))
    return 1;
  TAU2 = md * md;
  for (i = 0; i < 3; i++) {
    for (d = 0; d < 3; d++) R[3 * i + d] = init[4 * i + d];
    t[i] = init[4 * i + 3];
  }
  evaluate(R, t);
  while (it < hd[2]) {
    double pf = FIT, pr = RMSE;
    if (M < PCR_ICP_PLANE_MIN_CORR) { status = 1; break; }
    if (pcr_icp_plane_step(SUMS, R, t)) { status = 3; break; }
    it++;
    evaluate(R, t);
    if (fabs(pf - FIT) < tol[0] && fabs(pr - RMSE) < tol[1]) { status = 0; break; }
  }
  printf("%d %d %d\n", status, it, M);
  for (i = 0; i < N1; i++) printf("%d ", CORR[i]);
  printf("\n");
  for (i = 0; i < 9; i++) printf("%.17g ", R[i]);
  for (i = 0; i < 3; i++) printf("%.17g ", t[i]);
  printf("\n%.17g %.17g\n", FIT, RMSE);
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("icp_plane")
    src = d / "icp_plane_host.c"
    src.write_text(PROGRAM)
    out = d / "icp_plane_host"
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-I", INCLUDE, str(src), "-o",
                           str(out), "-lm"])
    return str(out)


# ------------------------------------------------------------------- ABI
def test_header_library_and_signatures_have_the_entry_point():
    from pcr_amd import _lib
    text = open(os.path.join(INCLUDE, "pcr_amd.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert hasattr(_lib.load(), NAME)
    assert NAME in _lib.SIGNATURES
    assert "pcr_icp_plane_step" in open(os.path.join(INCLUDE, "pcr_icp_plane.h")).read()


def test_argument_checks_need_no_gpu():
    """invalid parameters are refused before anything touches the device"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000  # never dereferenced: every call below is refused or p == 0
    names = ("xyz1", "xyz2", "normals2", "transform", "corr", "num", "fitness", "rmse",
             "iterations", "status")

    def call(p=1, n1=16, n2=16, dist=0.2, iters=10, rf=1e-6, rr=1e-6, **kw):
        a = dict({k: one for k in names}, **kw)
        return lib.pcr_icp_point_to_plane(a["xyz1"], a["xyz2"], a["normals2"], p, n1, n2, None,
                                          None, None, dist, iters, rf, rr, a["transform"],
                                          a["corr"], a["num"], a["fitness"], a["rmse"],
                                          a["iterations"], a["status"], None)
    assert call(p=0) == 0
    assert call(p=-1) == -1
    assert call(n1=0) == -1 and call(n2=0) == -1
    assert call(dist=0.0) == -1 and call(dist=-1.0) == -1 and call(dist=float("nan")) == -1
    assert call(iters=-1) == -1
    assert call(iters=100001) == -1
    assert b"max_iters" in lib.pcr_last_error()
    assert call(rf=-1e-9) == -1 and call(rr=-1e-9) == -1 and call(rr=float("nan")) == -1
    assert call(normals2=None) == -1
    assert b"null pointer" in lib.pcr_last_error()
    for k in names:
        assert call(**{k: None}) == -1, k


class _FakeCuda:
    """Stands in for a device tensor up to ops.icp's argument checks, which
    run before anything is allocated"""

    def __init__(self, shape, dtype):
        import torch
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True
        self.device = torch.device("cuda:0")

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


def test_ops_icp_refuses_a_bad_estimation_and_missing_normals():
    import torch
    from pcr_amd import ops
    x = _FakeCuda((2, 3, 8), torch.float32)
    with pytest.raises(RuntimeError, match="unknown estimation"):
        ops.icp(x, x, estimation="plane")
    with pytest.raises(RuntimeError, match="needs normals2"):
        ops.icp(x, x, estimation="point_to_plane")
    with pytest.raises(RuntimeError, match="normals2 must be"):
        ops.icp(x, x, estimation="point_to_plane", normals2=_FakeCuda((2, 3, 9), torch.float32))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.icp(x, x, estimation="point_to_plane", normals2=torch.zeros((2, 3, 8)))


# -------------------------------------------------------------- contract
# name -> (seed, n1, n2, make_pair keywords, icp keywords); the shapes of the
# GPU cases (tests/test_gpu_icp_plane.py) at sizes a scalar loop affords
CASES = {
    "n6": (1, 6, 6, {}, {}),
    "n5_8": (2, 5, 8, {}, {}),
    "n64": (3, 64, 64, {}, {}),
    "n200_260": (4, 200, 260, dict(degrees=10.0, tnorm=0.05), {}),
    "subset": (5, 150, 120, dict(degrees=1.0, tnorm=0.01), dict(max_dist=0.05)),
    "limit": (6, 64, 64, {}, dict(max_iters=1)),
    "evaluate": (7, 64, 80, {}, dict(max_iters=0)),
    "far": (8, 32, 32, dict(tnorm=10.0), {}),
    # the GPU test's larger shapes: the sums are long enough for their order to show
    "n1100_1024": (9, 1100, 1024, {}, {}),
    "n100_9000": (10, 100, 9000, {}, {}),
    "n1030_8200": (13, 1030, 8200, {}, dict(max_iters=1)),
}
ARGS = dict(max_dist=0.2, max_iters=200, rel_fitness=1e-6, rel_rmse=1e-6)


def run_exe(exe, path, x1, x2, nr, init, args):
    n1, n2 = x1.shape[1], x2.shape[1]
    path.write_bytes(struct.pack("<3if2d", n1, n2, args["max_iters"], args["max_dist"],
                                 args["rel_fitness"], args["rel_rmse"]) +
                     np.ascontiguousarray(init, np.float64).tobytes() + x1.tobytes() +
                     x2.tobytes() + nr.tobytes())
    got = subprocess.check_output([exe, str(path)]).decode().split("\n")
    status, it, num = (int(v) for v in got[0].split())
    v = np.array([float(x) for x in got[2].split()])
    tr = np.eye(4)
    tr[:3, :3], tr[:3, 3] = v[:9].reshape(3, 3), v[9:]
    fit, rmse = (float(x) for x in got[3].split())
    return dict(status=status, iterations=it, num_corr=num,
                corr=np.array(got[1].split(), dtype=np.int32), transform=tr, fitness=fit,
                rmse=rmse)


def compare(got, exp):
    """integer outputs and fitness equal, rmse to 1e-12 relative -> the
    largest transform difference"""
    assert exp["conv_margin"] > 1e-9  # the input condition of the exact comparison
    assert (got["status"], got["iterations"], got["num_corr"]) == \
        (exp["status"], exp["iterations"], exp["num_corr"])
    assert np.array_equal(got["corr"], exp["corr"])
    assert got["fitness"] == exp["fitness"]
    assert abs(got["rmse"] - exp["rmse"]) <= 1e-12 * max(exp["rmse"], 1e-300)
    diff = float(np.abs(got["transform"] - exp["transform"]).max())
    print("gcc versus numpy: largest transform difference %.3e" % diff)
    return diff


@pytest.mark.parametrize("name", list(CASES))
def test_scalar_run_of_the_headers_matches_the_restatement(exe, tmp_path, name):
    """The contract run with the headers' math in plain C loops equals the
    restatement: corr, num_corr, iterations, status and fitness exactly, the
    transform to 1e-9 (the measured largest difference is printed); pairs
    whose every source has its target recover the ground truth to 1e-5."""
    seed, n1, n2, mk, kw = CASES[name]
    x1, x2, nr, gt = pr.make_pair(np.random.default_rng(seed), n1, n2, **mk)
    args = dict(ARGS, **kw)
    exp = pr.icp_pair(x1, x2, nr, None, **args)
    got = run_exe(exe, tmp_path / "pair.bin", x1, x2, nr, np.eye(4), args)
    assert compare(got, exp) <= 1e-9
    status, it, num = got["status"], got["iterations"], got["num_corr"]
    if name in ("n6", "n64", "n200_260"):
        assert status == 0 and 1 <= it <= 10 and num == n1
        assert pr.transform_error(exp["transform"], gt) <= 1e-5
    if name == "n5_8":
        assert (status, it, num) == (1, 0, 5)
    if name == "subset":
        assert status == 0 and num == n2 and (exp["corr"] == -1).sum() == n1 - n2
    if name == "n1100_1024":  # 76 sources have no counterpart
        assert status == 0 and num >= n2
    if name == "n100_9000":
        assert status == 0 and num == n1
        assert pr.transform_error(exp["transform"], gt) <= 1e-5
    if name in ("limit", "n1030_8200"):
        assert (status, it) == (2, 1)
    if name == "evaluate":
        assert (status, it) == (2, 0) and np.array_equal(exp["transform"], np.eye(4))
    if name == "far":
        assert (status, it, num) == (1, 0, 0) and (exp["corr"] == -1).all()
        assert exp["fitness"] == 0.0 and exp["rmse"] == 0.0


def test_scalar_run_from_an_init(exe, tmp_path):
    x1, x2, nr, gt = pr.make_pair(np.random.default_rng(11), 100, 130, degrees=40.0, tnorm=0.5)
    init = gt @ ir.motion(np.random.default_rng(12), 3.0, 0.02)
    exp = pr.icp_pair(x1, x2, nr, init, **ARGS)
    got = run_exe(exe, tmp_path / "pair.bin", x1, x2, nr, init, ARGS)
    assert compare(got, exp) <= 1e-9
    assert got["status"] == 0 and pr.transform_error(exp["transform"], gt) <= 1e-5


def test_planar_target_has_exact_zero_pivots(exe, tmp_path):
    """status 3 with no iteration made, the transform the init in bits"""
    x1, x2, nr = pr.planar_pair(21)
    exp = pr.icp_pair(x1, x2, nr, None, **ARGS)
    assert (exp["status"], exp["iterations"]) == (3, 0) and exp["num_corr"] >= 6
    amat, _ = pr.system(np.eye(3), np.zeros(3), x1.T.copy(), x2.T.copy(), nr.T.copy(),
                        exp["corr"])
    assert (amat[2] == 0.0).all() and (amat[:, 2] == 0.0).all()
    got = run_exe(exe, tmp_path / "pair.bin", x1, x2, nr, np.eye(4), ARGS)
    assert (got["status"], got["iterations"], got["num_corr"]) == (3, 0, exp["num_corr"])
    assert np.array_equal(got["corr"], exp["corr"])
    assert got["transform"].tobytes() == np.eye(4).tobytes()


def test_sampling_case_is_what_the_plane_is_for(exe, tmp_path):
    """Two independent samplings of one surface: the plane step ends at a
    tenth of the point-to-point error or less, in fewer iterations, within
    1e-3 of the ground truth."""
    x1, x2, nr, gt = pr.sampling_pair(31)
    plane = pr.icp_pair(x1, x2, nr, None, **ARGS)
    point = ir.icp_pair(x1, x2, None, **ARGS)
    assert plane["conv_margin"] > 1e-9 and point["conv_margin"] > 1e-9
    e_plane = pr.transform_error(plane["transform"], gt)
    e_point = pr.transform_error(point["transform"], gt)
    print("sampling: plane %d iterations, error %.3e; point %d iterations, error %.3e"
          % (plane["iterations"], e_plane, point["iterations"], e_point))
    assert plane["status"] == 0 and point["status"] == 0
    assert e_plane <= e_point / 10 and e_plane <= 1e-3
    assert plane["iterations"] < point["iterations"]
    got = run_exe(exe, tmp_path / "pair.bin", x1, x2, nr, np.eye(4), ARGS)
    assert compare(got, plane) <= 1e-9


def test_nan_normal_is_status_3():
    x1, x2, nr, _ = pr.make_pair(np.random.default_rng(41), 64, 64, degrees=0.1, tnorm=0.001)
    nr = nr.copy()
    nr[:, 5] = np.nan
    exp = pr.icp_pair(x1, x2, nr, None, **ARGS)
    assert (exp["status"], exp["iterations"]) == (3, 0) and 5 in exp["corr"]
    assert np.array_equal(exp["transform"], np.eye(4))


def test_restatement_empty_clouds():
    x1, x2, nr, _ = pr.make_pair(np.random.default_rng(42), 16, 16)
    e = pr.icp_pair(x1[:, :0], x2, nr, None, **ARGS)
    assert (e["status"], e["iterations"], e["num_corr"], e["fitness"], e["rmse"]) == (1, 0, 0, 0, 0)
    e = pr.icp_pair(x1, x2[:, :0], nr[:, :0], None, **ARGS)
    assert (e["status"], e["num_corr"]) == (1, 0) and (e["corr"] == -1).all()
    e = pr.icp_pair(x1, x2[:, :0], nr[:, :0], None, **dict(ARGS, max_iters=0))
    assert e["status"] == 2
