"""CPU: the point-to-point ICP's ABI surface, its contract run in plain C
loops on include/pcr_rigid.h + pcr_math.h (gcc) against the numpy restatement
(tests/icp_restate.py), the restatement against the ground truth, and the
alignment_rmse meter."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import icp_restate as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAME = "pcr_icp_point_to_point"

PROGRAM = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "pcr_math.h"
#include "pcr_rigid.h"

/* The whole contract for one pair.  File: int n1 n2 max_iters; float
 * max_dist; double rel_fitness rel_rmse; double init[16]; xyz1 [3][n1];
 * xyz2 [3][n2]. */
static int N1, N2;
static float *X1, *X2, TAU2;
static int *CORR;
static int M;
static double FIT, RMSE;

static void evaluate(const double *R, const double *t) {
  float T[12];
  double e = 0.0;
  int i, j;
  pcr_rigid_round(R, t, T);
  M = 0;
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
      CORR[i] = bj;
      M++;
      e += (double)best;
    } else {
      CORR[i] = -1;
    }
  }
  FIT = (double)M / N1;
  RMSE = M ? sqrt(e / M) : 0.0;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
  int hd[3], it = 0, status = 2, i, d, k;
  float md;
  double tol[2], init[16], R[9], t[3], *pa, *pb;
  if (!f) return 1;
  if (fread(hd, 4, 3, f) != 3 || fread(&md, 4, 1, f) != 1 || fread(tol, 8, 2, f) != 2 ||
      fread(init, 8, 16, f) != 16) return 1;
  N1 = hd[0]; N2 = hd[1];
  X1 = malloc(12 * N1); X2 = malloc(12 * N2); CORR = malloc(4 * N1);
  pa = malloc(24 * N1); pb = malloc(24 * N1);
  if (fread(X1, 4, 3 * N1, f) != (size_t)(3 * N1) || fread(X2, 4, 3 * N2, f) != (size_t)(3 * N2))
    return 1;
  TAU2 = md * md;
  for (i = 0; i < 3; i++) {
    for (d = 0; d < 3; d++) R[3 * i + d] = init[4 * i + d];
    t[i] = init[4 * i + 3];
  }
  evaluate(R, t);
  while (it < hd[2]) {
    double pf = FIT, pr = RMSE;
    if (M < 3) { status = 1; break; }
    for (i = 0, k = 0; i < N1; i++)
      if (CORR[i] >= 0) {
        for (d = 0; d < 3; d++) {
          pa[3 * k + d] = X1[d * N1 + i];
          pb[3 * k + d] = X2[d * N2 + CORR[i]];
        }
        k++;
      }
    pcr_rigid_solve_n(pa, pb, k, R, t);
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
    d = tmp_path_factory.mktemp("icp")
    src = d / "icp_host.c"
    src.write_text(PROGRAM)
    out = d / "icp_host"
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
    assert "pcr_rigid_apply" in open(os.path.join(INCLUDE, "pcr_rigid.h")).read()


def test_argument_checks_need_no_gpu():
    """invalid parameters are refused before anything touches the device"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000  # never dereferenced: every call below is refused or p == 0
    names = ("xyz1", "xyz2", "transform", "corr", "num", "fitness", "rmse", "iterations", "status")

    def call(p=1, n1=16, n2=16, dist=0.2, iters=10, rf=1e-6, rr=1e-6, **kw):
        a = dict({k: one for k in names}, **kw)
        return lib.pcr_icp_point_to_point(a["xyz1"], a["xyz2"], p, n1, n2, None, dist, iters, rf,
                                          rr, a["transform"], a["corr"], a["num"], a["fitness"],
                                          a["rmse"], a["iterations"], a["status"], None)
    assert call(p=0) == 0
    assert call(p=-1) == -1
    assert call(n1=0) == -1 and call(n2=0) == -1
    assert call(dist=0.0) == -1 and call(dist=float("nan")) == -1
    assert call(iters=-1) == -1
    assert call(iters=100001) == -1
    assert b"max_iters" in lib.pcr_last_error()
    assert call(rf=-1e-9) == -1 and call(rr=-1e-9) == -1 and call(rr=float("nan")) == -1
    for k in names:
        assert call(**{k: None}) == -1, k


# rejected argument -> the message's tail; `{range}` is the name the range
# checks print, `{null}` the one the pointer check prints
ICP_ERRORS = (
    (dict(n1=0), "{range}: invalid sizes"),
    (dict(dist=0.0), "{range}: max_dist must be positive"),
    (dict(iters=-1), "{range}: max_iters (-1) outside [0, 100000]"),
    (dict(iters=100001), "{range}: max_iters (100001) outside [0, 100000]"),
    (dict(rf=-1e-9), "{range}: negative or NaN tolerance"),
    (dict(rr=float("nan")), "{range}: negative or NaN tolerance"),
    (dict(transform=None), "{null}: null pointer"),
)
# entry point -> (range name, null name): the ragged entry point reports its
# range errors under the dense name
ICP_ENTRY_NAMES = {
    "pcr_icp_point_to_point": ("icp_point_to_point", "icp_point_to_point"),
    "pcr_icp_point_to_point_ragged": ("icp_point_to_point", "icp_point_to_point_ragged"),
    "pcr_icp_point_to_plane": ("icp_point_to_plane", "icp_point_to_plane"),
}


@pytest.mark.parametrize("entry", list(ICP_ENTRY_NAMES))
def test_error_text_of_every_icp_entry_point(entry):
    """the three ICP entry points share one range check: each rejected
    argument leaves exactly the text the entry point gave before the check was
    shared (recorded from that build), under that entry point's own name"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000  # never dereferenced: every call below is refused
    fn = getattr(lib, entry)
    rng, null = ICP_ENTRY_NAMES[entry]

    def call(p=1, n1=16, n2=16, dist=0.2, iters=10, rf=1e-6, rr=1e-6, transform=one):
        head = (one, one) + ((one,) if entry.endswith("plane") else ()) + (p, n1, n2)
        counts = () if entry == "pcr_icp_point_to_point" else (None, None)
        return fn(*head, *counts, None, dist, iters, rf, rr, transform, one, one, one, one, one,
                  one, None)
    for kw, text in ICP_ERRORS:
        assert call(**kw) == -1, (entry, kw)
        assert lib.pcr_last_error() == text.format(range=rng, null=null).encode(), (entry, kw)


def test_cpu_tensors_rejected():
    import torch
    from pcr_amd import ops
    x = torch.zeros((2, 3, 8))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.icp(x, x)


# -------------------------------------------------------------- contract
# name -> (seed, n1, n2, make_pair keywords, icp keywords)
CASES = {
    "n64": (1, 64, 64, {}, {}),
    "n200_260": (2, 200, 260, dict(degrees=10.0, tnorm=0.05), {}),
    "subset": (3, 150, 120, dict(degrees=1.0, tnorm=0.01), dict(max_dist=0.05)),
    "noise": (4, 128, 128, dict(noise=0.004), {}),
    "limit": (5, 64, 64, {}, dict(max_iters=1)),
    "evaluate": (6, 64, 80, {}, dict(max_iters=0)),
    "far": (7, 32, 32, dict(tnorm=10.0), {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_scalar_run_of_the_headers_matches_the_restatement(exe, tmp_path, name):
    """The contract run with the headers' math in plain C loops equals the
    restatement: corr, num_corr, iterations, status exactly, the transform to
    1e-8; noise-free full-overlap pairs recover the ground truth to 1e-5."""
    seed, n1, n2, mk, kw = CASES[name]
    x1, x2, gt = ir.make_pair(np.random.default_rng(seed), n1, n2, **mk)
    args = dict(max_dist=0.2, max_iters=200, rel_fitness=1e-6, rel_rmse=1e-6)
    args.update(kw)
    exp = ir.icp_pair(x1, x2, None, **args)
    if exp["iterations"]:
        assert exp["conv_margin"] > 1e-9  # the input condition of the exact comparison
    path = tmp_path / "pair.bin"
    path.write_bytes(struct.pack("<3if2d", n1, n2, args["max_iters"], args["max_dist"],
                                 args["rel_fitness"], args["rel_rmse"]) +
                     np.eye(4).tobytes() + x1.tobytes() + x2.tobytes())
    got = subprocess.check_output([exe, str(path)]).decode().strip().split("\n")
    status, it, num = (int(v) for v in got[0].split())
    assert (status, it, num) == (exp["status"], exp["iterations"], exp["num_corr"])
    assert np.array_equal(np.array(got[1].split(), dtype=np.int32), exp["corr"])
    v = np.array([float(x) for x in got[2].split()])
    assert np.abs(v[:9].reshape(3, 3) - exp["transform"][:3, :3]).max() <= 1e-8
    assert np.abs(v[9:] - exp["transform"][:3, 3]).max() <= 1e-8
    fit, rmse = (float(x) for x in got[3].split())
    assert fit == exp["fitness"]
    assert abs(rmse - exp["rmse"]) <= 1e-12 * max(exp["rmse"], 1e-300)
    if name in ("n64", "n200_260"):
        assert status == 0 and 1 <= it <= 10
        assert np.abs(exp["transform"] - gt).max() <= 1e-5
        assert num == n1
    if name == "subset":
        assert status == 0 and num == n2 and (exp["corr"] == -1).sum() == n1 - n2
    if name == "noise":
        assert status == 0 and np.abs(exp["transform"] - gt).max() <= 2e-3
    if name == "limit":
        assert (status, it) == (2, 1)
    if name == "evaluate":
        assert (status, it) == (2, 0) and np.array_equal(exp["transform"], np.eye(4))
    if name == "far":
        assert (status, it, num) == (1, 0, 0) and (exp["corr"] == -1).all()
        assert exp["fitness"] == 0.0 and exp["rmse"] == 0.0


def test_restatement_ties_and_non_finite():
    """the lowest index wins a tie; a non-finite distance never wins"""
    a = np.array([[0.25, 0.0, 0.0], [0.0, 0.5, 0.0]], np.float32)
    b = np.array([[np.nan, 0.0, 0.0], [0.0, 0.5, 0.0], [0.25, 0.0, 0.0], [0.25, 0.0, 0.0],
                  [np.inf, 0.0, 0.0], [0.0, 0.5, 0.0]], np.float32)
    ev = ir.evaluate(np.eye(3), np.zeros(3), a, b, 0.2)
    assert ev["corr"].tolist() == [2, 1] and ev["num_corr"] == 2 and ev["rmse"] == 0.0
    ev = ir.evaluate(np.eye(3), np.full(3, np.nan), a, b, 0.2)
    assert ev["corr"].tolist() == [-1, -1] and ev["fitness"] == 0.0 and ev["rmse"] == 0.0


# --------------------------------------------------------------- meters
def test_alignment_rmse_against_numpy():
    import torch
    from pcr_amd.registration import alignment_rmse
    rng = np.random.default_rng(0)
    p, n = 3, 50
    xyz = rng.standard_normal((p, 3, n)).astype(np.float32)
    gt = np.stack([ir.motion(rng, 40.0, 0.5) for _ in range(p)])
    est = np.stack([ir.motion(rng, 41.0, 0.6) for _ in range(p)])
    est[0] = gt[0]
    got = alignment_rmse(torch.from_numpy(xyz), torch.from_numpy(gt), torch.from_numpy(est))
    x = xyz.astype(np.float64)
    exp = np.stack([np.mean(np.linalg.norm(
        (est[q, :3, :3] @ x[q] + est[q, :3, 3:4]) - (gt[q, :3, :3] @ x[q] + gt[q, :3, 3:4]),
        axis=0)) for q in range(p)])
    assert got.dtype == torch.float64 and tuple(got.shape) == (p,)
    assert np.abs(got.numpy() - exp).max() <= 1e-14
    assert got[0].item() == 0.0 and exp[1] > 0.01
