/*
 * pcr_teaser.h -- scalar math of the batched TEASER-style robust registration
 * (csrc/teaser.hip), shared by the HIP kernels (device) and
 * host C (tests compile it with gcc).  Like pcr_fgr.h it includes pcr_rigid.h,
 * for the fp64 edge length (pcr_rigid_dist) and the rotation solve
 * (pcr_rigid_from_cov): fixed sequences of IEEE-754 fp64 operations, compiled
 * with -ffp-contract=off.
 *
 *   graph     pcr_teaser_edge: the pairwise-consistency test of two slots
 *   rotation  pcr_teaser_tim: one translation-invariant measurement;
 *             pcr_teaser_r2: its squared residual under R; pcr_teaser_mu0,
 *             _weight: the GNC-TLS schedule's start and the weight update;
 *             pcr_teaser_accumulate: w u v^T; pcr_teaser_rotation: R from the
 *             nine sums
 *   vote      pcr_teaser_axis: X_k on one axis; pcr_teaser_endpoint;
 *             pcr_teaser_vote_lanes, _vote_at: a midpoint's estimate and cost;
 *             pcr_teaser_vote: the winner over a sorted endpoint list (host)
 *   report    pcr_teaser_report, pcr_teaser_identity: the 4 x 4
 */
#ifndef PCR_TEASER_H
#define PCR_TEASER_H

#include "pcr_rigid.h"

#if defined(__clang__)
#define PCR_TEASER_UNROLL _Pragma("unroll")
#else
#define PCR_TEASER_UNROLL
#endif

#define PCR_TEASER_MIN_CLIQUE 3   /* a smaller clique: status 1 */
#define PCR_TEASER_MAX_N1 4096    /* the graph is n1 * n1 bits per pair */
#define PCR_TEASER_MAX_ITERS 1000 /* every iteration walks K (K - 1) / 2 TIMs */

/* ---- graph ---- */
/* slots i and j are consistent: | |a_j - a_i| - |b_j - b_i| | <= beta.
 * Symmetric bit for bit (the lengths square the differences); a NaN never
 * joins. */
PCR_HD int pcr_teaser_edge(const float *ai, const float *bi, const float *aj, const float *bj,
                           double beta) {
  const double d = pcr_rigid_dist(aj, ai) - pcr_rigid_dist(bj, bi);
  return __builtin_fabs(d) <= beta;
}

/* ---- rotation ---- */
/* u = a_j - a_i, v = b_j - b_i in fp64 from the fp32 points */
PCR_HD void pcr_teaser_tim(const float *ai, const float *bi, const float *aj, const float *bj,
                           double *u, double *v) {
  u[0] = (double)aj[0] - (double)ai[0];
  u[1] = (double)aj[1] - (double)ai[1];
  u[2] = (double)aj[2] - (double)ai[2];
  v[0] = (double)bj[0] - (double)bi[0];
  v[1] = (double)bj[1] - (double)bi[1];
  v[2] = (double)bj[2] - (double)bi[2];
}

/* |v - R u|^2 (R row-major) */
PCR_HD double pcr_teaser_r2(const double *u, const double *v, const double *R) {
  const double e0 = v[0] - ((R[0] * u[0] + R[1] * u[1]) + R[2] * u[2]);
  const double e1 = v[1] - ((R[3] * u[0] + R[4] * u[1]) + R[5] * u[2]);
  const double e2 = v[2] - ((R[6] * u[0] + R[7] * u[1]) + R[8] * u[2]);
  return (e0 * e0 + e1 * e1) + e2 * e2;
}

/* the first iteration's mu from the largest squared residual */
PCR_HD double pcr_teaser_mu0(double max_r2, double nu2) {
  return 1.0 / ((2.0 * max_r2) / nu2 - 1.0);
}

/* the GNC-TLS weight of a squared residual at mu (> 0) */
PCR_HD double pcr_teaser_weight(double r2, double mu, double nu2) {
  const double hi = ((mu + 1.0) / mu) * nu2;
  const double lo = (mu / (mu + 1.0)) * nu2;
  if (r2 >= hi) return 0.0;
  if (r2 <= lo) return 1.0;
  return __builtin_sqrt(((nu2 * mu) * (mu + 1.0)) / r2) - mu;
}

/* H += w u v^T (row-major: H[3 i + j] sums w u_i v_j) */
PCR_HD void pcr_teaser_accumulate(const double *u, const double *v, double w, double *H) {
  const double wu0 = w * u[0], wu1 = w * u[1], wu2 = w * u[2];
  H[0] += wu0 * v[0];
  H[1] += wu0 * v[1];
  H[2] += wu0 * v[2];
  H[3] += wu1 * v[0];
  H[4] += wu1 * v[1];
  H[5] += wu1 * v[2];
  H[6] += wu2 * v[0];
  H[7] += wu2 * v[1];
  H[8] += wu2 * v[2];
}

/* the rotation with v ~ R u from H: pcr_rigid_from_cov with zero centroids */
PCR_HD void pcr_teaser_rotation(const double *H, double *R) {
  const double zero[3] = {0.0, 0.0, 0.0};
  double t[3];
  pcr_rigid_from_cov(zero, zero, H, R, t);
}

/* ---- vote ---- */
/* X_k on one axis: b - (R a) there; row: that axis' row of R, bx: b there */
PCR_HD double pcr_teaser_axis_row(const double *row, const float *a, float bx) {
  return (double)bx - ((row[0] * (double)a[0] + row[1] * (double)a[1]) + row[2] * (double)a[2]);
}

PCR_HD double pcr_teaser_axis(const double *R, const float *a, const float *b, int axis) {
  return pcr_teaser_axis_row(R + 3 * axis, a, b[axis]);
}

/* endpoint e of the 2 K: X_k - rho at e = 2 k, X_k + rho at e = 2 k + 1 */
PCR_HD double pcr_teaser_endpoint(const double *X, int e, double rho) {
  return (e & 1) ? X[e >> 1] + rho : X[e >> 1] - rho;
}

/* the midpoint of two consecutive endpoints */
PCR_HD double pcr_teaser_midpoint(double lo, double hi) { return 0.5 * (lo + hi); }

/* PCR_TEASER_VOTE_LANES midpoints m[] at once, X read once for all of them
 * (the kernel's threads take their endpoints in such groups).  Per midpoint:
 * the consensus set {k : |X_k - m| <= rho}, its mean (sum in ascending k) into
 * xhat[], and into cost[] the sum over k, ascending, of min((X_k - xhat)^2,
 * rho^2).  An empty set: xhat = m and the cost is +inf. */
#define PCR_TEASER_VOTE_LANES 4
PCR_HD void pcr_teaser_vote_lanes(const double *X, int K, const double *m, double rho,
                                  double *xhat, double *cost) {
  const double rho2 = rho * rho;
  double s[PCR_TEASER_VOTE_LANES], c[PCR_TEASER_VOTE_LANES];
  int n[PCR_TEASER_VOTE_LANES], j, k;
  PCR_TEASER_UNROLL
  for (j = 0; j < PCR_TEASER_VOTE_LANES; j++) {
    s[j] = 0.0;
    c[j] = 0.0;
    n[j] = 0;
  }
  for (k = 0; k < K; k++) {
    const double x = X[k];
    PCR_TEASER_UNROLL
    for (j = 0; j < PCR_TEASER_VOTE_LANES; j++) {
      if (__builtin_fabs(x - m[j]) <= rho) {
        s[j] += x;
        n[j]++;
      }
    }
  }
  PCR_TEASER_UNROLL
  for (j = 0; j < PCR_TEASER_VOTE_LANES; j++) xhat[j] = n[j] ? s[j] / (double)n[j] : m[j];
  for (k = 0; k < K; k++) {
    const double x = X[k];
    PCR_TEASER_UNROLL
    for (j = 0; j < PCR_TEASER_VOTE_LANES; j++) {
      const double d = x - xhat[j], d2 = d * d;
      c[j] += d2 < rho2 ? d2 : rho2;
    }
  }
  PCR_TEASER_UNROLL
  for (j = 0; j < PCR_TEASER_VOTE_LANES; j++) cost[j] = n[j] ? c[j] : __builtin_inf();
}

/* one midpoint: lane 0 of the above */
PCR_HD double pcr_teaser_vote_at(const double *X, int K, double m, double rho, double *xhat) {
  double mm[PCR_TEASER_VOTE_LANES], x[PCR_TEASER_VOTE_LANES], c[PCR_TEASER_VOTE_LANES];
  int j;
  PCR_TEASER_UNROLL
  for (j = 0; j < PCR_TEASER_VOTE_LANES; j++) mm[j] = m;
  pcr_teaser_vote_lanes(X, K, mm, rho, x, c);
  *xhat = x[0];
  return c[0];
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* The vote over `ord`, the 2 K endpoint numbers sorted by value, then by
 * number: the estimate of the midpoint of lowest cost, the earliest on ties. */
static inline double pcr_teaser_vote(const double *X, int K, const int *ord, double rho) {
  double best = __builtin_inf(), est = 0.0;
  int j, have = 0;
  for (j = 0; j + 1 < 2 * K; j++) {
    double x;
    const double m = pcr_teaser_midpoint(pcr_teaser_endpoint(X, ord[j], rho),
                                         pcr_teaser_endpoint(X, ord[j + 1], rho));
    const double c = pcr_teaser_vote_at(X, K, m, rho, &x);
    if (!have || c < best) {
      best = c;
      est = x;
      have = 1;
    }
  }
  return est;
}
#endif

/* ---- report ---- */
PCR_HD void pcr_teaser_report(const double *R, const double *t, double *out) {
  int i;
  for (i = 0; i < 3; i++) {
    out[4 * i] = R[3 * i];
    out[4 * i + 1] = R[3 * i + 1];
    out[4 * i + 2] = R[3 * i + 2];
    out[4 * i + 3] = t[i];
  }
  out[12] = 0.0;
  out[13] = 0.0;
  out[14] = 0.0;
  out[15] = 1.0;
}

PCR_HD void pcr_teaser_identity(double *out) {
  int i;
  for (i = 0; i < 16; i++) out[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

#endif /* PCR_TEASER_H */
