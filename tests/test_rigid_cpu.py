"""CPU: the rigid-transform estimation's ABI surface, its scalar math
(include/pcr_rigid.h compiled stand-alone with gcc, against the known answers
of the sampler and the SVD Kabsch of tests/rigid_restate.py) and the RRE / RTE
meters."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import rigid_restate as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("pcr_rigid_ransac", "pcr_rigid_ransac_workspace_size")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pcr_rigid.h"

static void sampler(void) {
  int t[3], h, bad = 0;
  printf("%08x %08x\n", pcr_rigid_mix(1u), pcr_rigid_mix(0xdeadbeefu));
  printf("%08x %08x %08x\n", pcr_rigid_draw(1u, 0u, 0u, 0u), pcr_rigid_draw(1u, 0u, 0u, 1u),
         pcr_rigid_draw(1u, 0u, 0u, 2u));
  printf("%08x\n", pcr_rigid_draw(12345u, 7u, 999u, 2u));
  for (h = 0; h < 4; h++) {
    pcr_rigid_triple(1u, 0u, (unsigned)h, 100u, t);
    printf("%d %d %d\n", t[0], t[1], t[2]);
  }
  pcr_rigid_triple(12345u, 127u, 65535u, 1024u, t);
  printf("%d %d %d\n", t[0], t[1], t[2]);
  for (h = 0; h < 4096; h++) {
    pcr_rigid_triple(7u, 3u, (unsigned)h, 3u, t);
    if ((1 << t[0] | 1 << t[1] | 1 << t[2]) != 7) bad++;
  }
  printf("%d\n", bad);
}

/* stdin: cases of `m` then m rows ax ay az bx by bz; m == 3 goes through the
 * fp32 3-point entry */
static void solve(void) {
  int m, k, i;
  while (scanf("%d", &m) == 1) {
    double *a = malloc(sizeof(double) * 3 * m), *b = malloc(sizeof(double) * 3 * m);
    double R[9], t[3];
    for (k = 0; k < m; k++) {
      for (i = 0; i < 3; i++) scanf("%lf", &a[3 * k + i]);
      for (i = 0; i < 3; i++) scanf("%lf", &b[3 * k + i]);
    }
    if (m == 3) {
      float fa[9], fb[9];
      for (i = 0; i < 9; i++) {
        fa[i] = (float)a[i];
        fb[i] = (float)b[i];
      }
      pcr_rigid_solve3(fa, fb, R, t);
    } else {
      pcr_rigid_solve_n(a, b, m, R, t);
    }
    for (i = 0; i < 9; i++) printf("%.17g ", R[i]);
    for (i = 0; i < 3; i++) printf("%.17g ", t[i]);
    printf("\n");
    free(a);
    free(b);
  }
}

/* The whole contract for one pair, one scalar loop after the other.  File:
 * int n1 n2 m q hyps refine; unsigned seed; float tau rho; xyz1 [3][n1];
 * xyz2 [3][n2]; idx1 [n1]; idx2 [n1]. */
static const float *X1, *X2;
static const int *I1, *I2;
static int N1, N2;
static void slot(int s, float *a, float *b) {
  int d;
  for (d = 0; d < 3; d++) {
    a[d] = X1[d * N1 + I1[s]];
    b[d] = X2[d * N2 + I2[s]];
  }
}
static int count_inliers(const float *T, int m, float tau2, int *mask) {
  int s, c = 0;
  for (s = 0; s < m; s++) {
    float a[3], b[3];
    int in;
    slot(s, a, b);
    in = pcr_rigid_resid2(T, a[0], a[1], a[2], b[0], b[1], b[2]) <= tau2;
    if (mask) mask[s] = in;
    c += in;
  }
  return c;
}
static void triple_points(unsigned seed, int q, int h, int m, float *a, float *b) {
  int t[3], k;
  pcr_rigid_triple(seed, (unsigned)q, (unsigned)h, (unsigned)m, t);
  for (k = 0; k < 3; k++) slot(t[k], a + 3 * k, b + 3 * k);
}
static int ransac(const char *path) {
  FILE *f = fopen(path, "rb");
  int hd[6], m, q, hyps, refine, h, it, i, s, best = -1, bestscore = -1, status = 0, num = 0;
  unsigned seed;
  float fl[2], tau2, T[12], a[9], b[9];
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  float *x1, *x2;
  int *i1, *i2, *mask, *scores;
  if (!f) return 1;
  if (fread(hd, 4, 6, f) != 6 || fread(&seed, 4, 1, f) != 1 || fread(fl, 4, 2, f) != 2) return 1;
  N1 = hd[0]; N2 = hd[1]; m = hd[2]; q = hd[3]; hyps = hd[4]; refine = hd[5];
  x1 = malloc(12 * N1); x2 = malloc(12 * N2); i1 = malloc(4 * N1); i2 = malloc(4 * N1);
  mask = calloc(N1, 4); scores = malloc(4 * hyps);
  if (fread(x1, 4, 3 * N1, f) != (size_t)(3 * N1) || fread(x2, 4, 3 * N2, f) != (size_t)(3 * N2) ||
      fread(i1, 4, N1, f) != (size_t)N1 || fread(i2, 4, N1, f) != (size_t)N1) return 1;
  X1 = x1; X2 = x2; I1 = i1; I2 = i2;
  tau2 = fl[0] * fl[0];
  for (h = 0; h < hyps; h++) scores[h] = -1;
  if (m < 3) {
    status = 1;
  } else {
    for (h = 0; h < hyps; h++) {
      triple_points(seed, q, h, m, a, b);
      if (!pcr_rigid_edge_ok(a, b, fl[1])) continue;
      pcr_rigid_solve3(a, b, R, t);
      pcr_rigid_round(R, t, T);
      scores[h] = count_inliers(T, m, tau2, NULL);
      if (scores[h] > bestscore) {
        bestscore = scores[h];
        best = h;
      }
    }
    if (best < 0) {
      status = 2;
      R[0] = R[4] = R[8] = 1; R[1] = R[2] = R[3] = R[5] = R[6] = R[7] = 0;
      t[0] = t[1] = t[2] = 0;
    } else {
      triple_points(seed, q, best, m, a, b);
      pcr_rigid_solve3(a, b, R, t);
      pcr_rigid_round(R, t, T);
      for (it = 0; it < refine; it++) {
        double *pa, *pb;
        int c = count_inliers(T, m, tau2, mask), k = 0;
        if (c < 3) break;
        pa = malloc(24 * c); pb = malloc(24 * c);
        for (s = 0; s < m; s++)
          if (mask[s]) {
            float u[3], v[3];
            slot(s, u, v);
            for (i = 0; i < 3; i++) { pa[3 * k + i] = u[i]; pb[3 * k + i] = v[i]; }
            k++;
          }
        pcr_rigid_solve_n(pa, pb, c, R, t);
        pcr_rigid_round(R, t, T);
        free(pa); free(pb);
      }
      num = count_inliers(T, m, tau2, mask);
    }
  }
  printf("%d %d %d\n", status, best, num);
  for (h = 0; h < hyps; h++) printf("%d ", scores[h]);
  printf("\n");
  for (s = 0; s < N1; s++) printf("%d ", mask[s]);
  printf("\n");
  for (i = 0; i < 9; i++) printf("%.17g ", R[i]);
  for (i = 0; i < 3; i++) printf("%.17g ", t[i]);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "sampler")) sampler();
  else if (argc > 1 && !strcmp(argv[1], "solve")) solve();
  else if (argc > 2 && !strcmp(argv[1], "ransac")) return ransac(argv[2]);
  else return 2;
  return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rigid")
    src = d / "rigid_host.c"
    src.write_text(PROGRAM)
    out = d / "rigid_host"
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-I", INCLUDE, str(src), "-o",
                           str(out), "-lm"])
    return str(out)


# ------------------------------------------------------------------- ABI
def test_header_library_and_signatures_have_the_entry_points():
    from pcr_amd import _lib
    text = open(os.path.join(INCLUDE, "pcr_amd.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.pcr_rigid_ransac_workspace_size(0, 0, 0) == 256
    assert lib.pcr_rigid_ransac_workspace_size(128, 1024, 1000) >= 128 * 4 * 8


def test_argument_checks_need_no_gpu():
    """invalid parameters are refused before anything touches the device"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000  # never dereferenced: every call below is refused or p == 0
    ptrs = dict(xyz1=one, xyz2=one, idx1=one, idx2=one, count=one, transform=one, inliers=one,
                num=one, best=one, status=one, ws=one)

    def call(p=1, hyps=8, tau=0.1, rho=0.9, refine=1, ws_bytes=1 << 20, **kw):
        a = dict(ptrs, **kw)
        return lib.pcr_rigid_ransac(a["xyz1"], a["xyz2"], p, 16, 16, a["idx1"], a["idx2"],
                                    a["count"], hyps, tau, rho, refine, 1, a["transform"],
                                    a["inliers"], a["num"], a["best"], None, a["status"], a["ws"],
                                    ws_bytes, None)
    assert call(p=0) == 0
    assert call(hyps=0) == -1
    assert call(tau=0.0) == -1
    assert call(tau=float("nan")) == -1
    assert call(rho=1.0) == -1
    assert call(rho=-0.1) == -1
    assert call(refine=-1) == -1
    assert call(ws_bytes=0) == -1
    assert b"workspace" in lib.pcr_last_error()
    for k in ("xyz1", "xyz2", "idx1", "idx2", "count", "transform", "inliers", "num", "best",
              "status", "ws"):
        assert call(**{k: None}) == -1, k


def test_cpu_tensors_rejected():
    import torch
    from pcr_amd import ops
    x = torch.zeros((1, 3, 8))
    i = torch.zeros((1, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.rigid_ransac(x, x, i, i, torch.zeros((1,), dtype=torch.int32))


# ------------------------------------------------------------------ math
def test_sampler_known_answers(exe):
    got = subprocess.check_output([exe, "sampler"]).decode().split("\n")
    assert got[0] == "688990c0 e628c683"
    assert got[1] == "b98a617e c0951f9f dbb74c9e"
    assert got[2] == "6ebb060f"
    assert got[3:7] == ["86 78 46", "43 79 14", "39 79 1", "92 50 21"]
    assert got[7] == "473 187 518"
    assert got[8] == "0"  # m = 3: always a permutation of (0, 1, 2)
    # the restatement's sampler agrees
    assert [int(v) for v in rr.mix(np.array([1, 0xDEADBEEF]))] == [0x688990C0, 0xE628C683]
    assert rr.triples(1, 0, np.arange(4), 100).tolist() == [[86, 78, 46], [43, 79, 14],
                                                            [39, 79, 1], [92, 50, 21]]
    assert rr.triples(12345, 127, 65535, 1024).tolist() == [[473, 187, 518]]


def _rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def _solve_cases():
    """name -> (a, b, well_posed); all values fp32-representable"""
    rng = np.random.default_rng(5)
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)
    cases = {}
    a = f(rng.uniform(-1, 1, (3, 3)))
    cases["triple"] = (a, f(a @ _rot(rng).T + [0.3, -0.2, 0.5]), True)
    a = f(np.c_[rng.uniform(-1, 1, (4, 2)), np.zeros(4)] @ _rot(rng).T)
    cases["coplanar4"] = (a, f(a @ _rot(rng).T + [0.1, 0.2, -0.3]), True)
    d = np.array([0.5, -0.25, 0.75])
    a = f(np.outer([-1.0, 0.5, 2.0], d) + [0.125, 0.25, 0.5])
    cases["collinear"] = (a, f(a + [1.0, 0.0, -1.0]), False)
    a = f(rng.uniform(-1, 1, (6, 3)))
    cases["reflected"] = (a, f(a * [1.0, 1.0, -1.0]), True)
    a = f(rng.uniform(-1, 1, (3, 3)))
    cases["identical_points"] = (f(np.tile(a[:1], (3, 1))), f(np.tile(a[1:2], (3, 1))), False)
    a = f(rng.uniform(-1, 1, (40, 3)))
    cases["noisy40"] = (a, f(a @ _rot(rng).T + rng.normal(0, 0.01, (40, 3))), True)
    return cases


def test_solve_is_a_proper_rotation_and_matches_the_svd(exe):
    cases = _solve_cases()
    text = ""
    for a, b, _ in cases.values():
        text += "%d\n" % len(a) + "".join(
            " ".join("%.17g" % v for v in np.r_[a[k], b[k]]) + "\n" for k in range(len(a)))
    got = subprocess.run([exe, "solve"], input=text.encode(), stdout=subprocess.PIPE,
                         check=True).stdout.decode().strip().split("\n")
    assert len(got) == len(cases)
    for (name, (a, b, well)), line in zip(cases.items(), got):
        v = np.array([float(x) for x in line.split()])
        r, t = v[:9].reshape(3, 3), v[9:]
        assert np.isfinite(v).all(), name
        assert abs(np.linalg.det(r) - 1.0) <= 1e-12, name
        assert np.abs(r @ r.T - np.eye(3)).max() <= 1e-12, name
        if well:
            sv = rr.cov_singular_values(a, b)
            # the input condition of the 1e-10 bound: the eigen-gap of the
            # problem (sigma2 +- sigma3 for a proper / reflected set)
            gap = sv[1] + (sv[2] if np.linalg.det((a - a.mean(0)).T @ (b - b.mean(0))) >= 0
                           else -sv[2])
            assert gap / sv[0] >= 1e-3, (name, sv)
            er, et = rr.kabsch(a, b)
            assert np.abs(r - er).max() <= 1e-10, name
            assert np.abs(t - et).max() <= 1e-10, name
        else:
            # any minimiser: the residual equals the SVD's
            er, et = rr.kabsch(a, b)
            res = np.linalg.norm(a @ r.T + t - b)
            assert abs(res - np.linalg.norm(a @ er.T + et - b)) <= 1e-10, name


def synthetic_pair(rng, n1, n2, m, outliers, noise=0.0):
    """source points in the unit ball, target = R a + t in fp32, a fraction
    replaced by uniform outliers; correspondences through shuffled indices"""
    a = rng.standard_normal((n1, 3))
    a *= (rng.uniform(0, 1, (n1, 1)) ** (1 / 3)) / np.linalg.norm(a, axis=1, keepdims=True)
    r, t = _rot(rng), rng.uniform(-0.5, 0.5, 3)
    i1 = rng.permutation(n1)[:m]
    i2 = rng.permutation(n2)[:m]
    xyz2 = rng.uniform(-1, 1, (n2, 3))
    tgt = a[i1].astype(np.float32).astype(np.float64) @ r.T + t + rng.normal(0, 1, (m, 3)) * noise
    bad = rng.uniform(0, 1, m) < outliers
    tgt[bad] = rng.uniform(-1, 1, (int(bad.sum()), 3))
    xyz2[i2] = tgt
    idx1 = np.full(n1, -1, np.int32)
    idx2 = np.full(n1, -1, np.int32)
    idx1[:m], idx2[:m] = i1, i2
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = r, t
    return (np.ascontiguousarray(a.T, dtype=np.float32),
            np.ascontiguousarray(xyz2.T, dtype=np.float32), idx1, idx2, gt)


@pytest.mark.parametrize("n1,n2,m,hyps,rho,refine,seed", [
    (80, 90, 64, 256, 0.9, 2, 1), (300, 310, 300, 128, 0.9, 2, 2), (10, 8, 3, 8, 0.9, 1, 3),
    (40, 40, 2, 4, 0.9, 1, 4), (129, 140, 129, 64, 0.0, 3, 5)])
def test_scalar_run_of_the_header_matches_the_restatement(exe, tmp_path, n1, n2, m, hyps, rho,
                                                          refine, seed):
    """The contract run with the header's math in plain C loops equals the
    restatement: scores, best hypothesis, mask exactly (no residual within
    1e-5 of the threshold), the transform to 1e-8."""
    rng = np.random.default_rng(seed)
    x1, x2, i1, i2, gt = synthetic_pair(rng, n1, n2, m, 0.55)
    tau, q = 0.02, 2
    path = tmp_path / "pair.bin"
    path.write_bytes(struct.pack("<6iI2f", n1, n2, m, q, hyps, refine, seed, tau, rho) +
                     x1.tobytes() + x2.tobytes() + i1.tobytes() + i2.tobytes())
    got = subprocess.check_output([exe, "ransac", str(path)]).decode().strip().split("\n")
    exp = rr.ransac_pair(x1, x2, i1, i2, m, q, hyps, tau, rho, refine, seed)
    assert exp["margin"] > 1e-5
    status, best, num = (int(v) for v in got[0].split())
    assert (status, best, num) == (exp["status"], exp["best_hyp"], exp["num_inliers"])
    assert np.array_equal(np.array(got[1].split(), dtype=np.int32), exp["scores"])
    assert np.array_equal(np.array(got[2].split(), dtype=np.int32), exp["inliers"])
    v = np.array([float(x) for x in got[3].split()])
    assert np.abs(v[:9].reshape(3, 3) - exp["transform"][:3, :3]).max() <= 1e-8
    assert np.abs(v[9:] - exp["transform"][:3, 3]).max() <= 1e-8
    if status == 0 and m >= 30:
        assert np.abs(exp["transform"] - gt).max() <= 1e-5
    if rho == 0.0:
        assert (exp["scores"] >= 0).all()


# --------------------------------------------------------------- meters
def test_rre_rte_against_numpy():
    import torch
    from pcr_amd.registration import apply_transform, rre_rte
    rng = np.random.default_rng(0)
    gt = np.tile(np.eye(4), (4, 1, 1))
    est = gt.copy()
    for i in range(4):
        gt[i, :3, :3], gt[i, :3, 3] = _rot(rng), rng.uniform(-1, 1, 3)
    est[0] = gt[0]                                        # gt = est
    c, s = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    est[1, :3, :3] = gt[1, :3, :3] @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    est[1, :3, 3] = gt[1, :3, 3] + [0.3, 0.0, 0.4]        # 30 degrees, 0.5 away
    est[2, :3, :3] = gt[2, :3, :3] * (1.0 + 1e-9)         # trace above 3: the clamp
    est[2, :3, 3] = gt[2, :3, 3]
    est[3, :3, :3] = gt[3, :3, :3] @ np.diag([-1.0, -1.0, 1.0]) * (1.0 + 1e-9)  # below -1
    est[3, :3, 3] = gt[3, :3, 3]
    rre, rte = rre_rte(torch.from_numpy(gt), torch.from_numpy(est))
    erre, erte = rr.rre_rte(gt, est)
    assert rre.dtype == torch.float64 and tuple(rre.shape) == (4,)
    # acos near 1 turns one ulp of the trace into 1e-6 degrees: gt = est is
    # held to 1e-5 degrees, the well-conditioned and the clamped cases to 1e-9
    assert np.abs(rre.numpy() - erre)[1:].max() <= 1e-9
    assert np.abs(rte.numpy() - erte).max() <= 1e-12
    assert rre[0].item() <= 1e-5 and erre[0] <= 1e-5 and rte[0].item() == 0.0
    assert abs(rre[1].item() - 30.0) <= 1e-9 and abs(rte[1].item() - 0.5) <= 1e-12
    assert rre[2].item() == 0.0 and rre[3].item() == 180.0
    # fp32 transforms are accepted
    rre32, _ = rre_rte(torch.from_numpy(gt.astype(np.float32)),
                       torch.from_numpy(est.astype(np.float32)))
    assert abs(rre32[1].item() - 30.0) <= 1e-3
    xyz = rng.standard_normal((4, 3, 7))
    got = apply_transform(torch.from_numpy(xyz.astype(np.float32)), torch.from_numpy(gt))
    exp = gt[:, :3, :3] @ xyz.astype(np.float32).astype(np.float64) + gt[:, :3, 3:4]
    assert got.dtype == torch.float64 and np.abs(got.numpy() - exp).max() <= 1e-14
