"""CPU: the Fast Global Registration's ABI surface, its contract run in plain C
loops on include/pcr_fgr.h + pcr_rigid.h (gcc) against the numpy restatement
(tests/fgr_restate.py), and the header's Cholesky solve and step rotation
against numpy and scipy."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fgr_restate as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("pcr_fgr", "pcr_fgr_workspace_size")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pcr_fgr.h"

/* fgr <file>: the whole contract for one pair.  File: int n1 n2 m q
 * max_tuples trials_per_corr iterations decrease_mu absolute_scale; unsigned
 * seed; float tuple_scale; double max_corr_dist division_factor; xyz1 [3][n1];
 * xyz2 [3][n2]; idx1 [n1]; idx2 [n1].
 * chol <file>: 36 + 6 doubles -> x and the failure flag.
 * delta <file>: 6 doubles -> Rd, td. */
static int N1, N2;
static float *X1, *X2;
static int *I1, *I2;

static int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

static void slot(int s, float *a, float *b) {
  const int ia = clampi(I1[s], N1 - 1), ib = clampi(I2[s], N2 - 1);
  int d;
  for (d = 0; d < 3; d++) {
    a[d] = X1[d * N1 + ia];
    b[d] = X2[d * N2 + ib];
  }
}

static double scale_of(const float *x, int n, const double *m, double s) {
  int i;
  for (i = 0; i < n; i++) {
    const double v = pcr_fgr_norm(x[i], x[n + i], x[2 * n + i], m);
    if (v > s || v != v) s = v;
  }
  return s;
}

static int run_fgr(FILE *f) {
  int hd[9], m, q, max_tuples, iters, kcap, *L, K = 0, status = 0, it, i, d, k;
  unsigned seed;
  float rho;
  double par[2], m1[3], m2[3], s = 0.0, dn, mu = 0.0, R[9], t[3], out[16];
  long long H, h, num_trials;
  if (fread(hd, 4, 9, f) != 9 || fread(&seed, 4, 1, f) != 1 || fread(&rho, 4, 1, f) != 1 ||
      fread(par, 8, 2, f) != 2) return 1;
  N1 = hd[0]; N2 = hd[1]; m = hd[2]; q = hd[3]; max_tuples = hd[4]; iters = hd[6];
  X1 = malloc(12 * N1); X2 = malloc(12 * N2); I1 = malloc(4 * N1); I2 = malloc(4 * N1);
  if (fread(X1, 4, 3 * N1, f) != (size_t)(3 * N1) || fread(X2, 4, 3 * N2, f) != (size_t)(3 * N2) ||
      fread(I1, 4, N1, f) != (size_t)N1 || fread(I2, 4, N1, f) != (size_t)N1) return 1;
  m = m < 0 ? 0 : m > N1 ? N1 : m;
  kcap = max_tuples ? 3 * max_tuples : N1;
  L = malloc(4 * (kcap + 3));
  if (max_tuples == 0) {
    for (i = 0; i < m; i++) L[K++] = i;
    num_trials = 0;
  } else {
    H = (long long)hd[5] * m;
    num_trials = H;
    for (h = 0; m >= 3 && h < H; h++) {
      int s3[3];
      float a[9], b[9];
      pcr_rigid_triple(seed, (unsigned)q, (unsigned)h, (unsigned)m, s3);
      for (k = 0; k < 3; k++) slot(s3[k], a + 3 * k, b + 3 * k);
      if (!pcr_rigid_edge_ok(a, b, rho)) continue;
      for (k = 0; k < 3; k++) L[K++] = s3[k];
      if (K == 3 * max_tuples) {
        num_trials = h + 1;
        break;
      }
    }
  }
  pcr_fgr_identity(out);
  if (K < PCR_FGR_MIN_CORR) {
    status = 1;
  } else {
    for (d = 0; d < 3; d++) {
      m1[d] = pcr_fgr_sum(X1 + d * N1, N1) / (double)N1;
      m2[d] = pcr_fgr_sum(X2 + d * N2, N2) / (double)N2;
    }
    s = scale_of(X2, N2, m2, scale_of(X1, N1, m1, 0.0));
    if (!(s > 0.0 && s < __builtin_inf())) status = 2;
  }
  if (!status) {
    double *P = malloc(24 * K), *Q0 = malloc(24 * K);
    dn = hd[8] ? 1.0 : s;
    mu = hd[8] ? s : 1.0;
    for (i = 0; i < K; i++) {
      float a[3], b[3];
      slot(L[i], a, b);
      pcr_fgr_unit(a, m1, dn, P + 3 * i);
      pcr_fgr_unit(b, m2, dn, Q0 + 3 * i);
    }
    for (i = 0; i < 9; i++) R[i] = i % 4 == 0 ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
    for (it = 0; it < iters; it++) {
      double sums[PCR_FGR_NSUM];
      for (i = 0; i < PCR_FGR_NSUM; i++) sums[i] = 0.0;
      for (i = 0; i < K; i++) pcr_fgr_accumulate(P + 3 * i, Q0 + 3 * i, R, t, mu, sums);
      if (pcr_fgr_step(sums, R, t)) {
        status = 3;
        break;
      }
      if (hd[7] && it % 4 == 0 && mu > par[0]) mu /= par[1];
    }
    pcr_fgr_report(R, t, m1, m2, dn, out);
  }
  printf("%d %d %lld\n", status, K, num_trials);
  for (i = 0; i < kcap; i++) printf("%d ", i < K ? L[i] : -1);
  printf("\n%.17g\n", mu);
  for (i = 0; i < 16; i++) printf("%.17g ", out[i]);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  FILE *f = argc > 2 ? fopen(argv[2], "rb") : NULL;
  double v[42], x[6] = {0, 0, 0, 0, 0, 0}, Rd[9], td[3];
  int i;
  if (!f) return 1;
  if (!strcmp(argv[1], "fgr")) return run_fgr(f);
  if (!strcmp(argv[1], "chol")) {
    if (fread(v, 8, 42, f) != 42) return 1;
    i = pcr_fgr_cholesky_solve(v, v + 36, x);
    printf("%d", i);
    for (i = 0; i < 6; i++) printf(" %.17g", x[i]);
    printf("\n");
    return 0;
  }
  if (!strcmp(argv[1], "delta")) {
    if (fread(v, 8, 6, f) != 6) return 1;
    pcr_fgr_delta(v, Rd, td);
    for (i = 0; i < 9; i++) printf("%.17g ", Rd[i]);
    for (i = 0; i < 3; i++) printf("%.17g ", td[i]);
    printf("\n");
    return 0;
  }
  return 1;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("fgr")
    src = d / "fgr_host.c"
    src.write_text(PROGRAM)
    out = d / "fgr_host"
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
    assert '#include "pcr_rigid.h"' in open(os.path.join(INCLUDE, "pcr_fgr.h")).read()
    assert b"fgr_tuple_kernel" in open(_lib.LIB_PATH, "rb").read()


def test_argument_checks_need_no_gpu():
    """invalid parameters are refused before anything touches the device"""
    from pcr_amd import _lib
    lib = _lib.load()
    one = 0x1000  # never dereferenced: every call below is refused or p == 0
    names = ("xyz1", "xyz2", "idx1", "idx2", "count", "transform", "slots", "num_corr",
             "num_trials", "mu", "status", "ws")

    def call(p=1, n1=16, n2=16, dist=0.08, iters=64, div=1.4, dec=1, scale=0.95, tuples=1000,
             trials=100, absolute=0, ws_bytes=1 << 30, **kw):
        a = dict({k: one for k in names}, **kw)
        return lib.pcr_fgr(a["xyz1"], a["xyz2"], p, n1, n2, a["idx1"], a["idx2"], a["count"], dist,
                           iters, div, dec, scale, tuples, trials, absolute, 0, a["transform"],
                           a["slots"], a["num_corr"], a["num_trials"], a["mu"], a["status"],
                           a["ws"], ws_bytes, None)
    assert call(p=0) == 0
    assert call(p=-1) == -1 and call(n1=0) == -1 and call(n2=0) == -1
    assert call(iters=-1) == -1 and call(iters=100001) == -1
    assert b"iterations" in lib.pcr_last_error()
    assert call(div=1.0) == -1 and call(div=0.5) == -1 and call(div=float("nan")) == -1
    assert call(scale=-0.1) == -1 and call(scale=1.0) == -1 and call(scale=float("nan")) == -1
    assert call(tuples=-1) == -1
    assert call(dist=-1.0) == -1 and call(dist=float("nan")) == -1
    assert call(trials=-1) == -1
    assert call(n1=1 << 20, trials=1 << 11) == -1  # H would pass 2^31 - 1
    assert b"2^31" in lib.pcr_last_error()
    for k in names:
        assert call(**{k: None}) == -1, k
    need = lib.pcr_fgr_workspace_size(1, 16, 1000)
    assert need >= 6 * 3000 * 4 and need % 256 == 0
    assert lib.pcr_fgr_workspace_size(1, 16, 0) == 512  # 6 * 16 floats, rounded up
    assert lib.pcr_fgr_workspace_size(0, 16, 1000) == 256
    assert call(ws_bytes=need - 1) == -1
    assert b"workspace" in lib.pcr_last_error()


def test_cpu_tensors_rejected():
    import torch
    from pcr_amd import ops
    from pcr_amd.registration import fgr_pairs, register_pairs
    x = torch.zeros((2, 3, 8))
    i = torch.zeros((2, 8), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.fgr(x, x, i, i, i[:, 0].contiguous())
    f = torch.zeros((2, 8, 4))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        fgr_pairs(x, x, f, f)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        register_pairs(x, x, f, f, solver="fgr")
    with pytest.raises(RuntimeError, match="unknown solver"):
        register_pairs(x, x, f, f, solver="teaserpp")


# -------------------------------------------------------------- contract
# name -> (seed, n1, n2, make_pair keywords, fgr keywords)
CASES = {
    "clean_list": (1, 64, 64, {}, dict(max_tuples=0)),
    "clean_tuples": (2, 200, 260, dict(degrees=120.0), dict(max_tuples=50)),
    "wrong_cap": (3, 256, 256, dict(wrong=0.3), dict(max_tuples=100, seed=7)),
    "exhausted": (4, 48, 48, dict(wrong=0.7), dict(trials_per_corr=20)),
    "absolute": (5, 600, 700, dict(wrong=0.2), dict(max_tuples=0, absolute_scale=True)),
    "fixed_mu": (6, 100, 100, dict(wrong=0.2), dict(max_tuples=0, decrease_mu=False)),
    "one_step": (7, 64, 64, {}, dict(max_tuples=0, iterations=1)),
    "no_step": (8, 64, 64, {}, dict(max_tuples=0, iterations=0)),
    "nine": (9, 64, 64, dict(m=9), dict(max_tuples=0)),
    "two": (10, 64, 64, dict(m=2), {}),
    "none": (11, 64, 64, dict(m=0), {}),
}


def run_c(exe, path, x1, x2, i1, i2, m, q, kw):
    kw = dict(fr.DEFAULTS, **kw)
    path.write_bytes(struct.pack("<9iIf2d", x1.shape[1], x2.shape[1], m, q, kw["max_tuples"],
                                 kw["trials_per_corr"], kw["iterations"], int(kw["decrease_mu"]),
                                 int(kw["absolute_scale"]), kw["seed"], kw["tuple_scale"],
                                 kw["max_corr_dist"], kw["division_factor"]) +
                     x1.tobytes() + x2.tobytes() + i1.tobytes() + i2.tobytes())
    got = subprocess.check_output([exe, "fgr", str(path)]).decode().strip().split("\n")
    status, k, trials = (int(v) for v in got[0].split())
    return dict(status=status, num_corr=k, num_trials=trials,
                slots=np.array(got[1].split(), dtype=np.int32), mu=float(got[2]),
                transform=np.array([float(v) for v in got[3].split()]).reshape(4, 4))


def assert_pair_matches(got, exp):
    assert (got["status"], got["num_corr"], got["num_trials"]) == \
        (exp["status"], exp["num_corr"], exp["num_trials"])
    assert np.array_equal(got["slots"], exp["slots"])
    assert got["mu"] == exp["mu"]
    assert np.abs(got["transform"] - exp["transform"]).max() <= 1e-8
    assert np.array_equal(got["transform"][3], [0.0, 0.0, 0.0, 1.0])


@pytest.mark.parametrize("name", list(CASES))
def test_scalar_run_of_the_headers_matches_the_restatement(exe, tmp_path, name):
    """The contract run with the headers' math in plain C loops equals the
    restatement: slots, num_corr, num_trials, status and mu exactly, the
    transform to 1e-8 (two fp64 solves on O(1) data), under the condition that
    the restatement summed upwards and downwards agrees to 1e-11; pairs whose
    matches are all correct recover the ground truth to 1e-5."""
    seed, n1, n2, mk, kw = CASES[name]
    q = seed % 3  # the sampler takes the pair's index
    x1, x2, i1, i2, m, gt = fr.make_pair(np.random.default_rng(seed), n1, n2, **mk)
    exp = fr.fgr_pair(x1, x2, i1, i2, m, q, **kw)
    down = fr.fgr_pair(x1, x2, i1, i2, m, q, -1, **kw)
    assert exp["status"] == down["status"]
    assert np.abs(exp["transform"] - down["transform"]).max() <= 1e-11
    got = run_c(exe, tmp_path / "pair.bin", x1, x2, i1, i2, m, q, kw)
    assert_pair_matches(got, exp)
    rre, rte = fr.rre_rte(gt[None], got["transform"][None])
    print("%s: K %d, trials %d, mu %.6g, RRE %.3g deg, RTE %.3g" % (
        name, got["num_corr"], got["num_trials"], got["mu"], rre[0], rte[0]))
    if name in ("clean_list", "clean_tuples"):
        assert got["status"] == 0 and np.abs(got["transform"] - gt).max() <= 1e-5
    if name == "clean_list":
        assert got["num_corr"] == n1 and got["num_trials"] == 0
        assert np.array_equal(got["slots"], np.arange(n1))
    if name in ("clean_tuples", "wrong_cap"):
        cap = kw["max_tuples"]
        assert got["num_corr"] == 3 * cap and got["num_trials"] < 100 * n1
        assert (got["slots"] >= 0).all()
    if name == "exhausted":
        assert got["num_trials"] == 20 * n1 and 10 <= got["num_corr"] < 3000
        assert (got["slots"][got["num_corr"]:] == -1).all()
    if name == "absolute":
        # mu starts at the scale (about 1: unit ball) and stops below 0.08
        assert got["status"] == 0 and 0.08 / 1.4 < got["mu"] <= 0.08
    if name == "fixed_mu":
        assert got["mu"] == 1.0
    if name == "one_step":
        assert got["mu"] == 1.0 / 1.4 and not np.array_equal(got["transform"], np.eye(4))
    if name == "no_step":
        # the identity loop transform: the centroids' difference
        assert got["mu"] == 1.0 and np.array_equal(got["transform"][:3, :3], np.eye(3))
    if name in ("nine", "two", "none"):
        assert got["status"] == 1 and got["mu"] == 0.0
        assert np.array_equal(got["transform"], np.eye(4))
        assert got["num_trials"] == {"nine": 0, "two": 200, "none": 0}[name]
        assert got["num_corr"] == {"nine": 9, "two": 0, "none": 0}[name]


def test_bad_pairs(exe, tmp_path):
    """non-finite or coincident clouds: status 2; a cloud that is one point:
    a singular first step, status 3 with the centroids' difference"""
    x1, x2, i1, i2, m, gt = fr.make_pair(np.random.default_rng(20), 32, 32)
    kw = dict(max_tuples=0)
    nan1 = x1.copy()
    nan1[1, 5] = np.nan
    same1, same2 = np.full_like(x1, 0.25), np.full_like(x2, -0.5)
    for a, b, status in ((nan1, x2, 2), (same1, same2, 2), (x1, same2, 3)):
        exp = fr.fgr_pair(a, b, i1, i2, m, 0, **kw)
        got = run_c(exe, tmp_path / "pair.bin", a, b, i1, i2, m, 0, kw)
        assert exp["status"] == status
        assert_pair_matches(got, exp)
    assert got["mu"] == 1.0 and np.array_equal(got["transform"][:3, :3], np.eye(3))
    # with the tuple test no triple of such a pair passes: status 1
    for a, b in ((nan1 * np.nan, x2), (same1, same2)):
        exp = fr.fgr_pair(a, b, i1, i2, m, 0)
        got = run_c(exe, tmp_path / "pair.bin", a, b, i1, i2, m, 0, {})
        assert exp["status"] == 1 and got["num_trials"] == 3200
        assert_pair_matches(got, exp)


def test_ordered_sum_is_the_header_order(exe, tmp_path):
    """the centroid of a cloud with widely spread magnitudes depends on the
    order of its sum; the restatement's order is the header's (mu under
    absolute_scale is the scale, bit for bit)"""
    rng = np.random.default_rng(30)
    x1, x2, i1, i2, m, gt = fr.make_pair(rng, 1500, 1500)
    x1 = (x1 * np.exp(rng.uniform(-12, 3, x1.shape))).astype(np.float32)
    kw = dict(max_tuples=0, absolute_scale=True, iterations=0)
    exp = fr.fgr_pair(x1, x2, i1, i2, m, 0, **kw)
    got = run_c(exe, tmp_path / "pair.bin", x1, x2, i1, i2, m, 0, kw)
    assert got["mu"] == exp["mu"] and exp["mu"] > 1.0
    assert fr.ordered_sum(x1[0]) != float(np.sum(x1[0].astype(np.float64)[::-1]))


# ------------------------------------------------------------ scalar math
def test_cholesky_solve_known_answers(exe, tmp_path):
    rng = np.random.default_rng(40)
    path = tmp_path / "sys.bin"
    for _ in range(20):
        b = rng.standard_normal((6, 8))
        amat, g = b @ b.T, rng.standard_normal(6)
        path.write_bytes(amat.tobytes() + g.tobytes())
        got = [float(v) for v in subprocess.check_output([exe, "chol", str(path)]).split()]
        assert got[0] == 0
        want = np.linalg.solve(amat, g)
        # relative to the solution, times the condition number of the system
        assert np.abs(np.array(got[1:]) - want).max() <= \
            1e-15 * np.linalg.cond(amat) * max(1.0, np.abs(want).max()) * 10
    # singular (rank 5), indefinite and non-finite systems fail
    b = rng.standard_normal((6, 5))
    sing = b @ b.T
    sing[:, 5], sing[5, :] = 0.0, 0.0
    indef = np.diag([1.0, 2.0, -1.0, 1.0, 1.0, 1.0])
    nan = np.eye(6)
    nan[2, 2] = np.nan
    inf = np.eye(6)
    inf[4, 4] = np.inf
    for amat in (sing, indef, nan, inf, np.zeros((6, 6))):
        path.write_bytes(amat.tobytes() + np.ones(6).tobytes())
        got = subprocess.check_output([exe, "chol", str(path)]).split()
        assert int(got[0]) == 1


def test_delta_is_a_proper_rotation_in_scipy_order(exe, tmp_path):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(41)
    path = tmp_path / "delta.bin"
    for scale in (1e-9, 1e-3, 0.5, 3.0):
        d = rng.uniform(-1, 1, 6) * scale
        path.write_bytes(d.tobytes())
        got = np.array([float(v) for v in
                        subprocess.check_output([exe, "delta", str(path)]).split()])
        rd = got[:9].reshape(3, 3)
        assert np.abs(rd @ rd.T - np.eye(3)).max() <= 1e-15 * 8
        assert abs(np.linalg.det(rd) - 1.0) <= 1e-15 * 8
        # extrinsic x, y, z: Rz Ry Rx
        assert np.abs(rd - Rotation.from_euler("xyz", d[:3]).as_matrix()).max() <= 1e-15 * 8
        assert np.abs(rd - fr.euler(d[:3])).max() <= 1e-15 * 8
        assert np.array_equal(got[9:], d[3:])
