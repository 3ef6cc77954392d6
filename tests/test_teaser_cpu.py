"""CPU: the TEASER-style robust registration's ABI surface, its contract run in
plain C loops on include/pcr_teaser.h + pcr_rigid.h (gcc) against the numpy
restatement (tests/teaser_restate.py), the restatement's own conditions (the
planted set is the clique, the ground truth is reached, the greedy search
meets the exact maximum on small graphs), and known answers of the header's
weight update and vote."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import teaser_restate as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("pcr_teaser", "pcr_teaser_workspace_size")
KERNELS = (b"teaser_graph_kernel", b"teaser_rank_kernel", b"teaser_clique_kernel",
           b"teaser_solve_kernel")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pcr_teaser.h"

/* teaser <file>: the whole contract for one pair.  File: int n1 n2 m max_iters
 * seeds inlier_selection; double noise_bound cbar2 gnc_factor cost_threshold;
 * xyz1 [3][n1]; xyz2 [3][n2]; idx1 [n1]; idx2 [n1].
 * weight <file>: double r2 mu nu2 -> the weight.
 * vote <file>: int K; double rho; K doubles -> the estimate. */
static int N1, N2;
static float *X1, *X2;
static int *I1, *I2;
static const double *SORT_X;
static double SORT_RHO;

static int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

static void slot(int s, float *a, float *b) {
  const int ia = clampi(I1[s], N1 - 1), ib = clampi(I2[s], N2 - 1);
  int d;
  for (d = 0; d < 3; d++) {
    a[d] = X1[d * N1 + ia];
    b[d] = X2[d * N2 + ib];
  }
}

static int by_value_then_number(const void *pa, const void *pb) {
  const int ea = *(const int *)pa, eb = *(const int *)pb;
  const double va = pcr_teaser_endpoint(SORT_X, ea, SORT_RHO);
  const double vb = pcr_teaser_endpoint(SORT_X, eb, SORT_RHO);
  if (va < vb) return -1;
  if (va > vb) return 1;
  return ea < eb ? -1 : ea > eb;
}

static double vote(const double *X, int K, double rho) {
  int *ord = malloc(8 * K), e;
  double t;
  for (e = 0; e < 2 * K; e++) ord[e] = e;
  SORT_X = X;
  SORT_RHO = rho;
  qsort(ord, 2 * K, sizeof(int), by_value_then_number);
  t = pcr_teaser_vote(X, K, ord, rho);
  free(ord);
  return t;
}

static int run_teaser(FILE *f) {
  int hd[6], m, max_iters, seeds, K = 0, status = 0, iters = 0, ninl = 0, i, j, k, d, r, S;
  double par[4], beta, rho, nu2, R[9], t[3] = {0, 0, 0}, out[16];
  float *A, *B;
  unsigned char *adj, *P;
  int *deg, *order, *C, *best, *inl;
  if (fread(hd, 4, 6, f) != 6 || fread(par, 8, 4, f) != 4) return 1;
  N1 = hd[0]; N2 = hd[1]; m = hd[2]; max_iters = hd[3]; seeds = hd[4];
  X1 = malloc(12 * N1); X2 = malloc(12 * N2); I1 = malloc(4 * N1); I2 = malloc(4 * N1);
  if (fread(X1, 4, 3 * N1, f) != (size_t)(3 * N1) || fread(X2, 4, 3 * N2, f) != (size_t)(3 * N2) ||
      fread(I1, 4, N1, f) != (size_t)N1 || fread(I2, 4, N1, f) != (size_t)N1) return 1;
  m = m < 0 ? 0 : m > N1 ? N1 : m;
  beta = 2.0 * (par[0] * __builtin_sqrt(par[1]));
  rho = par[0] * __builtin_sqrt(par[1]);
  nu2 = beta * beta;
  A = malloc(12 * (m + 1)); B = malloc(12 * (m + 1));
  for (i = 0; i < m; i++) slot(i, A + 3 * i, B + 3 * i);
  C = malloc(4 * (m + 1)); best = malloc(4 * (m + 1)); inl = calloc(N1, 4);
  if (hd[5]) {
    adj = calloc((size_t)m * m + 1, 1); P = malloc(m + 1);
    deg = calloc(m + 1, 4); order = malloc(4 * (m + 1));
    for (i = 0; i < m; i++)
      for (j = 0; j < m; j++)
        if (i != j && pcr_teaser_edge(A + 3 * i, B + 3 * i, A + 3 * j, B + 3 * j, beta)) {
          adj[(size_t)i * m + j] = 1;
          deg[i]++;
        }
    for (i = 0; i < m; i++) {
      int rank = 0;
      for (j = 0; j < m; j++) rank += deg[j] > deg[i] || (deg[j] == deg[i] && j < i);
      order[rank] = i;
    }
    S = seeds == 0 ? m : seeds < m ? seeds : m;
    for (r = 0; r < S; r++) {
      int n = 0, v = order[r];
      C[n++] = v;
      memcpy(P, adj + (size_t)v * m, m);
      for (;;) {
        int u = -1;
        for (k = 0; k < m; k++)
          if (P[order[k]]) {
            u = order[k];
            break;
          }
        if (u < 0) break;
        C[n++] = u;
        for (k = 0; k < m; k++) P[k] &= adj[(size_t)u * m + k];
      }
      if (n > K) {
        K = n;
        memcpy(best, C, 4 * n);
      }
    }
    /* ascending slots */
    for (i = 1; i < K; i++) {
      const int v = best[i];
      for (j = i; j > 0 && best[j - 1] > v; j--) best[j] = best[j - 1];
      best[j] = v;
    }
  } else {
    for (i = 0; i < m; i++) best[K++] = i;
  }
  pcr_teaser_identity(out);
  if (K < PCR_TEASER_MIN_CLIQUE) {
    status = 1;
  } else {
    const long T = (long)K * (K - 1) / 2;
    double *U = malloc(24 * T), *V = malloc(24 * T), *w = malloc(8 * T), *r2 = malloc(8 * T);
    double mu = 0.0, prev = __builtin_inf(), mx = 0.0, *X = malloc(8 * K);
    long n = 0, c;
    for (i = 0; i < K; i++)
      for (j = i + 1; j < K; j++, n++) {
        pcr_teaser_tim(A + 3 * best[i], B + 3 * best[i], A + 3 * best[j], B + 3 * best[j],
                       U + 3 * n, V + 3 * n);
        w[n] = 1.0;
      }
    status = 3;
    while (iters < max_iters) {
      double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cost = 0.0, diff;
      for (c = 0; c < T; c++) pcr_teaser_accumulate(U + 3 * c, V + 3 * c, w[c], H);
      pcr_teaser_rotation(H, R);
      iters++;
      for (c = 0; c < T; c++) r2[c] = pcr_teaser_r2(U + 3 * c, V + 3 * c, R);
      if (iters == 1) {
        for (c = 0; c < T; c++)
          if (r2[c] > mx || r2[c] != r2[c]) mx = r2[c];
        if (!(mx < __builtin_inf())) {
          status = 2;
          break;
        }
        mu = pcr_teaser_mu0(mx, nu2);
        if (!(mu > 0.0 && mu < __builtin_inf())) {
          status = 0;
          break;
        }
      }
      for (c = 0; c < T; c++) {
        cost += w[c] * r2[c];
        w[c] = pcr_teaser_weight(r2[c], mu, nu2);
      }
      mu *= par[2];
      diff = __builtin_fabs(cost - prev);
      prev = cost;
      if (diff < par[3]) {
        status = 0;
        break;
      }
    }
    if (status != 2) {
      for (d = 0; d < 3; d++) {
        for (k = 0; k < K; k++) X[k] = pcr_teaser_axis(R, A + 3 * best[k], B + 3 * best[k], d);
        t[d] = vote(X, K, rho);
      }
      for (k = 0; k < K; k++) {
        int ok = 1;
        for (d = 0; d < 3; d++)
          ok &= __builtin_fabs(pcr_teaser_axis(R, A + 3 * best[k], B + 3 * best[k], d) - t[d]) <= rho;
        inl[best[k]] = ok;
        ninl += ok;
      }
      pcr_teaser_report(R, t, out);
    }
  }
  printf("%d %d %d %d\n", status, K, ninl, iters);
  for (i = 0; i < N1; i++) printf("%d ", i < K ? best[i] : -1);
  printf("\n");
  for (i = 0; i < N1; i++) printf("%d ", inl[i]);
  printf("\n");
  for (i = 0; i < 16; i++) printf("%.17g ", out[i]);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  FILE *f = argc > 2 ? fopen(argv[2], "rb") : NULL;
  double v[3], rho, *X;
  int K;
  if (!f) return 1;
  if (!strcmp(argv[1], "teaser")) return run_teaser(f);
  if (!strcmp(argv[1], "weight")) {
    if (fread(v, 8, 3, f) != 3) return 1;
    printf("%.17g\n", pcr_teaser_weight(v[0], v[1], v[2]));
    return 0;
  }
  if (!strcmp(argv[1], "vote")) {
    if (fread(&K, 4, 1, f) != 1 || fread(&rho, 8, 1, f) != 1) return 1;
    X = malloc(8 * K);
    if (fread(X, 8, K, f) != (size_t)K) return 1;
    printf("%.17g\n", vote(X, K, rho));
    return 0;
  }
  return 1;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("teaser")
    src = d / "teaser_host.c"
    src.write_text(PROGRAM)
    out = d / "teaser_host"
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-I", INCLUDE, str(src), "-o",
                           str(out), "-lm"])
    return str(out)


# ------------------------------------------------------------------- ABI
def test_header_library_and_signatures_have_the_entry_points():
    from pcr_amd import _lib
    text = open(os.path.join(INCLUDE, "pcr_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text)
        assert hasattr(_lib.load(), name)
        assert name in _lib.SIGNATURES
    assert '#include "pcr_rigid.h"' in open(os.path.join(INCLUDE, "pcr_teaser.h")).read()
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in KERNELS:
        assert kernel in blob, kernel


def test_argument_checks_need_no_gpu():
    """invalid parameters are refused before anything touches the device"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000  # never dereferenced: every call below is refused or p == 0
    names = ("xyz1", "xyz2", "idx1", "idx2", "count", "transform", "clique", "clique_size",
             "inliers", "num_inliers", "iterations", "status", "ws")

    def call(p=1, n1=16, n2=16, noise=0.02, cbar2=1.0, factor=1.4, iters=100, thr=1e-12, seeds=0,
             select=1, ws_bytes=1 << 30, **kw):
        a = dict({k: one for k in names}, **kw)
        return lib.pcr_teaser(a["xyz1"], a["xyz2"], p, n1, n2, a["idx1"], a["idx2"], a["count"],
                              noise, cbar2, factor, iters, thr, seeds, select, a["transform"],
                              a["clique"], a["clique_size"], a["inliers"], a["num_inliers"],
                              a["iterations"], a["status"], a["ws"], ws_bytes, None)
    nan = float("nan")
    assert call(p=0) == 0
    assert call(p=-1) == -1 and call(n1=0) == -1 and call(n2=0) == -1
    assert call(n1=4097) == -1
    assert b"4096" in lib.pcr_last_error()
    assert call(p=0, n1=4096) == 0
    assert call(noise=0.0) == -1 and call(noise=-0.02) == -1 and call(noise=nan) == -1
    assert call(cbar2=0.0) == -1 and call(cbar2=-1.0) == -1 and call(cbar2=nan) == -1
    assert call(factor=1.0) == -1 and call(factor=0.5) == -1 and call(factor=nan) == -1
    assert call(iters=0) == -1 and call(iters=1001) == -1 and call(iters=-3) == -1
    assert b"max_iters" in lib.pcr_last_error()
    assert call(p=0, iters=1) == 0 and call(p=0, iters=1000) == 0
    assert call(thr=-1e-12) == -1 and call(thr=nan) == -1
    assert call(p=0, thr=0.0) == 0
    assert call(seeds=-1) == -1
    for k in names:
        assert call(**{k: None}) == -1, k
    # per pair n1 * ceil(n1 / 64) * 8 bytes of bit rows and two ints per slot;
    # the total rounded up to 256
    size = lib.pcr_teaser_workspace_size
    assert size(1, 16) == 256  # 16 * (8 + 8)
    assert size(1, 64) == 1024 and size(1, 65) == 65 * 24 + 256 - 65 * 24 % 256
    assert size(128, 1024) == 128 * (1024 * 16 * 8 + 8192)
    assert size(3, 4096) == 3 * 4096 * (64 * 8 + 8)
    assert size(0, 16) == 256 and size(1, 4097) == 256
    need = size(1, 16)
    assert call(ws_bytes=need - 1) == -1
    assert b"workspace" in lib.pcr_last_error()


def test_cpu_tensors_rejected():
    import torch
    from pcr_amd import ops
    from pcr_amd.registration import PairExtractor, register_pairs, teaser_pairs
    x = torch.zeros((2, 3, 8))
    i = torch.zeros((2, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.teaser(x, x, i, i, i[:, 0].contiguous())
    f = torch.zeros((2, 8, 4))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        teaser_pairs(x, x, f, f)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        register_pairs(x, x, f, f, solver="teaser")
    with pytest.raises(RuntimeError, match="'ransac', 'fgr' or 'teaser'"):
        register_pairs(x, x, f, f, solver="teaser++")
    assert "solver" in PairExtractor.register.__doc__ and "teaser" in PairExtractor.register.__doc__


# -------------------------------------------------------------- contract
# name -> (seed, n1, n2, make_pair keywords, teaser keywords)
CASES = {
    "clean": (1, 64, 64, {}, {}),
    "wrong30": (2, 130, 160, dict(wrong=0.3), {}),
    "wrong55": (3, 200, 200, dict(wrong=0.55, degrees=120.0), {}),
    "wrong90": (4, 300, 300, dict(wrong=0.9), {}),
    "noisy": (5, 150, 150, dict(wrong=0.4, noise=0.02), {}),
    "noisy_all": (6, 120, 120, dict(wrong=0.3, noise=0.01), dict(inlier_selection=False)),
    "all_slots": (7, 100, 100, dict(wrong=0.3), dict(inlier_selection=False)),
    "limit": (7, 100, 100, dict(wrong=0.3), dict(inlier_selection=False, max_iters=3)),
    "capped": (8, 160, 160, dict(wrong=0.5), dict(seeds=5)),
    "loose": (9, 90, 90, dict(wrong=0.5, noise=0.06), dict(noise_bound=0.05, cbar2=1.5,
                                                            gnc_factor=1.2, cost_threshold=1e-9)),
    "two": (10, 64, 64, dict(m=2), {}),
    "one": (11, 64, 64, dict(m=1), {}),
    "none": (12, 64, 64, dict(m=0), {}),
    "all_wrong": (13, 40, 400, dict(wrong=1.0), dict(noise_bound=0.001)),
}
PLANTED = ("clean", "wrong30", "wrong55", "wrong90")


def run_c(exe, path, x1, x2, i1, i2, m, kw):
    kw = dict(tr.DEFAULTS, **kw)
    path.write_bytes(struct.pack("<6i4d", x1.shape[1], x2.shape[1], m, kw["max_iters"],
                                 kw["seeds"], int(kw["inlier_selection"]), kw["noise_bound"],
                                 kw["cbar2"], kw["gnc_factor"], kw["cost_threshold"]) +
                     x1.tobytes() + x2.tobytes() + i1.tobytes() + i2.tobytes())
    got = subprocess.check_output([exe, "teaser", str(path)]).decode().strip().split("\n")
    status, k, ninl, iters = (int(v) for v in got[0].split())
    return dict(status=status, clique_size=k, num_inliers=ninl, iterations=iters,
                clique=np.array(got[1].split(), dtype=np.int32),
                inliers=np.array(got[2].split(), dtype=np.int32),
                transform=np.array([float(v) for v in got[3].split()]).reshape(4, 4))


def assert_pair_matches(got, exp):
    for k in ("status", "clique_size", "num_inliers", "iterations"):
        assert got[k] == exp[k], k
    assert np.array_equal(got["clique"], exp["clique"])
    assert np.array_equal(got["inliers"], exp["inliers"])
    assert np.abs(got["transform"] - exp["transform"]).max() <= 1e-8
    assert np.array_equal(got["transform"][3], [0.0, 0.0, 0.0, 1.0])


@pytest.mark.parametrize("name", list(CASES))
def test_scalar_run_of_the_headers_matches_the_restatement(exe, tmp_path, name):
    """The contract run with the headers' math in plain C loops equals the
    restatement: clique, clique_size, inliers, num_inliers, iterations and
    status exactly, the transform to 1e-8 (fp64 solves on O(1) data), under
    the condition that the restatement summed upwards and downwards agrees to
    1e-11 and in every exact output.  Planted pairs (noise-free inliers): the
    clique is the planted set and the ground truth is reached to 1e-5 (the
    fp32 rounding of the targets)."""
    seed, n1, n2, mk, kw = CASES[name]
    x1, x2, i1, i2, m, gt, planted = tr.make_pair(np.random.default_rng(seed), n1, n2, **mk)
    exp = tr.teaser_pair(x1, x2, i1, i2, m, **kw)
    down = tr.teaser_pair(x1, x2, i1, i2, m, -1, **kw)
    for k in tr.KEYS[1:]:
        assert np.array_equal(exp[k], down[k]), k
    assert np.abs(exp["transform"] - down["transform"]).max() <= 1e-11
    got = run_c(exe, tmp_path / "pair.bin", x1, x2, i1, i2, m, kw)
    assert_pair_matches(got, exp)
    rre, rte = tr.rre_rte(gt[None], got["transform"][None])
    print("%s: K %d, inliers %d, iterations %d, status %d, RRE %.3g deg, RTE %.3g" % (
        name, got["clique_size"], got["num_inliers"], got["iterations"], got["status"], rre[0],
        rte[0]))
    k = got["clique_size"]
    assert (got["clique"][:k] >= 0).all() and (np.diff(got["clique"][:k]) > 0).all()
    assert (got["clique"][k:] == -1).all()
    assert got["num_inliers"] == got["inliers"].sum() <= k
    assert (got["inliers"][got["clique"][:k]].sum()) == got["num_inliers"]
    if name in PLANTED:
        assert np.array_equal(got["clique"][:k], planted)
        assert got["status"] == 0 and np.abs(got["transform"] - gt).max() <= 1e-5
        # every TIM of a noise-free clique is far inside the bound: one solve
        assert got["iterations"] == 1 and got["num_inliers"] == k
    if name in ("noisy", "noisy_all", "all_slots", "loose"):
        assert got["status"] == 0 and got["iterations"] > 3  # the GNC loop ran
    if name in ("all_slots", "limit", "noisy_all"):
        assert k == m and np.array_equal(got["clique"][:k], np.arange(m))
    if name == "all_slots":
        # GNC-TLS alone at 30 % wrong matches: the wrong TIMs end with weight
        # 0, so the rotation is the planted set's; on one axis a wrong match
        # can lie within rho of the consensus and pull its mean, so the
        # translation is only within rho; the inliers are the planted set
        assert np.array_equal(np.nonzero(got["inliers"])[0], planted)
        assert np.abs(got["transform"][:3, :3] - gt[:3, :3]).max() <= 1e-5
        assert np.abs(got["transform"][:3, 3] - gt[:3, 3]).max() <= 0.02
    if name == "limit":
        assert got["status"] == 3 and got["iterations"] == 3
        assert not np.array_equal(got["transform"], np.eye(4))
    if name == "capped":
        full = tr.teaser_pair(x1, x2, i1, i2, m)
        assert 3 <= k <= full["clique_size"]
    if name in ("two", "one", "none", "all_wrong"):
        assert got["status"] == 1 and got["iterations"] == 0 and got["num_inliers"] == 0
        assert np.array_equal(got["transform"], np.eye(4))
    if name in ("two", "one", "none"):
        assert k == m
    if name == "all_wrong":
        assert k < 3


def test_bad_pairs(exe, tmp_path):
    """a NaN point is an isolated vertex (the clique avoids it); with every
    slot taken it reaches the TIMs: status 2.  Coincident clouds are a complete
    graph whose rotation is the solve's identity."""
    x1, x2, i1, i2, m, gt, planted = tr.make_pair(np.random.default_rng(20), 32, 32)
    nan1 = x1.copy()
    nan1[1, 5] = np.nan
    same1, same2 = np.full_like(x1, 0.25), np.full_like(x2, -0.5)
    for a, b, kw, status in ((nan1, x2, {}, 0), (nan1, x2, dict(inlier_selection=False), 2),
                             (same1, same2, {}, 0), (x1, same2, {}, 1)):
        exp = tr.teaser_pair(a, b, i1, i2, m, **kw)
        got = run_c(exe, tmp_path / "pair.bin", a, b, i1, i2, m, kw)
        assert exp["status"] == status
        assert_pair_matches(got, exp)
        if status == 2:
            assert got["iterations"] == 1 and got["num_inliers"] == 0
            assert np.array_equal(got["transform"], np.eye(4))
    exp = tr.teaser_pair(nan1, x2, i1, i2, m)
    assert exp["clique_size"] == 31 and 5 not in exp["clique"]
    exp = tr.teaser_pair(same1, same2, i1, i2, m)
    assert exp["clique_size"] == 32 and exp["num_inliers"] == 32
    assert np.array_equal(exp["transform"][:3, :3], np.eye(3))
    assert np.array_equal(exp["transform"][:3, 3], [-0.75, -0.75, -0.75])


def test_greedy_search_meets_the_exact_maximum_on_small_graphs():
    """planted pairs of at most 40 slots: the bounded search's clique is as
    large as the exact maximum clique (Bron-Kerbosch)"""
    for seed, n, wrong in ((30, 12, 0.5), (31, 24, 0.7), (32, 40, 0.55), (33, 40, 0.9),
                           (34, 33, 0.3)):
        x1, x2, i1, i2, m, gt, planted = tr.make_pair(np.random.default_rng(seed), n, 3 * n,
                                                      wrong=wrong)
        a32 = np.ascontiguousarray(x1[:, i1[:m]].T)
        b32 = np.ascontiguousarray(x2[:, i2[:m]].T)
        adj = tr.graph(a32, b32, tr.bounds(0.02, 1.0)[0])
        assert np.array_equal(adj, adj.T)
        got = tr.greedy_clique(adj)
        assert adj[np.ix_(got, got)].sum() == len(got) * (len(got) - 1)  # a clique
        assert len(got) == tr.max_clique_size(adj) >= len(planted)
    # the exact search itself on known graphs: a 5-cycle, K4 plus a pendant, no edges
    ring = np.zeros((5, 5), bool)
    for i in range(5):
        ring[i, (i + 1) % 5] = ring[(i + 1) % 5, i] = True
    k4 = np.zeros((5, 5), bool)
    k4[:4, :4] = ~np.eye(4, dtype=bool)
    k4[3, 4] = k4[4, 3] = True
    assert tr.max_clique_size(ring) == 2 and tr.max_clique_size(k4) == 4
    assert tr.max_clique_size(np.zeros((3, 3), bool)) == 1
    assert tr.greedy_clique(k4) == [0, 1, 2, 3]


# ------------------------------------------------------------ scalar math
def test_weight_update_known_answers(exe, tmp_path):
    """nu^2 = 4, mu = 1: the band is [2, 8]; inside it sqrt(nu^2 mu (mu + 1) /
    r^2) - mu"""
    path = tmp_path / "w.bin"

    def weight(r2, mu, nu2):
        path.write_bytes(struct.pack("<3d", r2, mu, nu2))
        return float(subprocess.check_output([exe, "weight", str(path)]))
    assert weight(8.0, 1.0, 4.0) == 0.0 and weight(100.0, 1.0, 4.0) == 0.0
    assert weight(2.0, 1.0, 4.0) == 1.0 and weight(0.0, 1.0, 4.0) == 1.0
    assert weight(4.5, 1.0, 4.0) == np.sqrt(8.0 / 4.5) - 1.0
    assert weight(4.0, 1.0, 4.5) == 0.5  # sqrt(9 / 4) - 1
    assert weight(3.0, 3.0, 1.0) == 0.0  # the upper end at mu = 3: 4 / 3
    assert weight(0.75, 3.0, 1.0) == 1.0  # the lower end: 3 / 4
    assert weight(1.0, 3.0, 1.0) == np.sqrt(12.0) - 3.0
    rng = np.random.default_rng(40)
    for _ in range(50):
        r2, mu, nu2 = rng.uniform(0, 3), rng.uniform(0.01, 50), rng.uniform(0.1, 2)
        assert weight(r2, mu, nu2) == float(tr.weights(np.float64(r2), mu, nu2))


def test_vote_known_answers(exe, tmp_path):
    path = tmp_path / "v.bin"

    def vote(x, rho):
        x = np.asarray(x, np.float64)
        path.write_bytes(struct.pack("<id", len(x), rho) + x.tobytes())
        got = float(subprocess.check_output([exe, "vote", str(path)]))
        assert got == tr.vote(x, rho) == tr.vote(x, rho, -1)
        return got
    # three agreeing measurements and an outlier: the mean of the three
    assert vote([1.0, 1.25, 0.75, 9.0], 0.5) == 1.0
    # two clusters: the larger
    assert vote([0.0, 0.0, 4.0, 4.0, 4.0], 1.0) == 4.0
    # two clusters of equal size and spread: equal costs, the earliest midpoint
    # (the lower cluster) wins
    assert vote([4.0, 0.0, 4.0, 0.0], 1.0) == 0.0
    # tied endpoints: equal measurements, and X_0 + rho == X_2 - rho
    assert vote([2.0, 2.0, 2.0], 0.25) == 2.0
    assert vote([0.0, 0.0, 2.0], 1.0) == 0.0
    assert vote([0.0, 2.0, 2.0], 1.0) == 2.0
    # a chain 0, 1, 2 at rho = 1, midpoints -0.5, 0.5, 1, 1.5, 2.5: the sets {0, 1}
    # and {1, 2} cost 1.5, all three cost 2; the earlier of the two pairs wins
    assert vote([0.0, 1.0, 2.0], 1.0) == 0.5
    rng = np.random.default_rng(41)
    for _ in range(20):
        k = int(rng.integers(3, 30))
        x = np.round(rng.normal(0, 1, k) * 4) / 4  # many exact ties
        vote(x, float(rng.choice([0.125, 0.25, 0.5, 1.0])))
