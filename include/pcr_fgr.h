/*
 * pcr_fgr.h -- scalar math of the batched Fast Global Registration
 * (csrc/fgr.hip), shared by the HIP kernels (device) and host
 * C (tests compile it with gcc).  Like pcr_rigid.h, which it includes for the
 * triple sampler and the edge-length check: fixed sequences of IEEE-754 fp64
 * operations, compiled with -ffp-contract=off.
 *
 *   normalise  pcr_fgr_norm / _unit: the distance of an fp32 point to a
 *              centroid and the point in normalised units; pcr_fgr_sum: the
 *              ordered fp64 sum the centroids are made of (host)
 *   terms      pcr_fgr_move, _weight, _accumulate: one correspondence's
 *              moved point, line-process weight and its 16 moment terms
 *   step       pcr_fgr_assemble: A (6 x 6) and g from the 16 sums;
 *              pcr_fgr_cholesky_solve with its failure rule; pcr_fgr_delta:
 *              Rz Ry Rx and the translation of a step; pcr_fgr_compose;
 *              pcr_fgr_step: all four
 *   report     pcr_fgr_report: the inverse in original units, 4 x 4
 */
#ifndef PCR_FGR_H
#define PCR_FGR_H

#include "pcr_rigid.h"

#if defined(__clang__)
#define PCR_FGR_UNROLL _Pragma("unroll")
#else
#define PCR_FGR_UNROLL
#endif

#if defined(__HIP__)
#define PCR_FGR_SIN(x) sin(x)
#define PCR_FGR_COS(x) cos(x)
#else
#define PCR_FGR_SIN(x) __builtin_sin(x)
#define PCR_FGR_COS(x) __builtin_cos(x)
#endif

#define PCR_FGR_MIN_CORR 10 /* fewer correspondences: status 1 */
#define PCR_FGR_NSUM 16     /* moment sums per iteration */
#define PCR_FGR_THREADS 512 /* partial sums of pcr_fgr_sum = threads of the kernel */
#define PCR_FGR_MAX_ITERS 100000

/* ---- normalise ---- */
/* |x - m| of an fp32 point */
PCR_HD double pcr_fgr_norm(float x, float y, float z, const double *m) {
  const double dx = (double)x - m[0];
  const double dy = (double)y - m[1];
  const double dz = (double)z - m[2];
  return __builtin_sqrt(dx * dx + dy * dy + dz * dz);
}

/* (x - m) / d */
PCR_HD void pcr_fgr_unit(const float *x, const double *m, double d, double *out) {
  out[0] = ((double)x[0] - m[0]) / d;
  out[1] = ((double)x[1] - m[1]) / d;
  out[2] = ((double)x[2] - m[2]) / d;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* The fp64 sum of x[0 .. n) in the order of the kernel's workgroup sum:
 * partial j < PCR_FGR_THREADS takes i = j, j + PCR_FGR_THREADS, ... in
 * ascending order; every 64 consecutive partials meet in the xor butterfly
 * (offsets 32, 16, ... 1); the results are added in ascending order. */
static inline double pcr_fgr_sum(const float *x, int n) {
  double part[PCR_FGR_THREADS], tmp[64], s = 0.0;
  int i, j, w, off;
  for (j = 0; j < PCR_FGR_THREADS; j++) {
    part[j] = 0.0;
    for (i = j; i < n; i += PCR_FGR_THREADS) part[j] += (double)x[i];
  }
  for (w = 0; w < PCR_FGR_THREADS / 64; w++) {
    double *v = part + 64 * w;
    for (off = 32; off > 0; off >>= 1) {
      for (j = 0; j < 64; j++) tmp[j] = v[j] + v[j ^ off];
      for (j = 0; j < 64; j++) v[j] = tmp[j];
    }
    s = w ? s + v[0] : v[0];
  }
  return s;
}
#endif

/* ---- terms ---- */
/* q = R q0 + t (R row-major) */
PCR_HD void pcr_fgr_move(const double *R, const double *t, const double *q0, double *q) {
  int i;
  PCR_FGR_UNROLL
  for (i = 0; i < 3; i++)
    q[i] = ((R[3 * i] * q0[0] + R[3 * i + 1] * q0[1]) + R[3 * i + 2] * q0[2]) + t[i];
}

/* the line-process weight (mu / (r.r + mu))^2 */
PCR_HD double pcr_fgr_weight(const double *r, double mu) {
  const double w = mu / (((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + mu);
  return w * w;
}

/* Adds one correspondence (p, q0: normalised source / target point) under
 * T = (R, t) to the 16 sums
 *   [0] w   [1..3] w q   [4..9] w q q^T (xx xy xz yy yz zz)
 *   [10..12] w (r x q)   [13..15] w r,      q = R q0 + t, r = p - q */
PCR_HD void pcr_fgr_accumulate(const double *p, const double *q0, const double *R, const double *t,
                               double mu, double *sums) {
  double q[3], r[3], wq[3], w;
  pcr_fgr_move(R, t, q0, q);
  r[0] = p[0] - q[0];
  r[1] = p[1] - q[1];
  r[2] = p[2] - q[2];
  w = pcr_fgr_weight(r, mu);
  wq[0] = w * q[0];
  wq[1] = w * q[1];
  wq[2] = w * q[2];
  sums[0] += w;
  sums[1] += wq[0];
  sums[2] += wq[1];
  sums[3] += wq[2];
  sums[4] += wq[0] * q[0];
  sums[5] += wq[0] * q[1];
  sums[6] += wq[0] * q[2];
  sums[7] += wq[1] * q[1];
  sums[8] += wq[1] * q[2];
  sums[9] += wq[2] * q[2];
  sums[10] += w * (r[1] * q[2] - r[2] * q[1]);
  sums[11] += w * (r[2] * q[0] - r[0] * q[2]);
  sums[12] += w * (r[0] * q[1] - r[1] * q[0]);
  sums[13] += w * r[0];
  sums[14] += w * r[1];
  sums[15] += w * r[2];
}

/* ---- step ---- */
/* A = sum w J^T J (row-major 6 x 6) and g = sum w J^T r for J = [[q]x, -I]:
 * A = [[sum w (|q|^2 I - q q^T), [sum w q]x], [-[sum w q]x, (sum w) I]],
 * g = (sum w (r x q), -sum w r). */
PCR_HD void pcr_fgr_assemble(const double *s, double *A, double *g) {
  const double tr = (s[4] + s[7]) + s[9];
  int i;
  PCR_FGR_UNROLL
  for (i = 0; i < 36; i++) A[i] = 0.0;
  A[0] = tr - s[4];
  A[7] = tr - s[7];
  A[14] = tr - s[9];
  A[1] = A[6] = -s[5];
  A[2] = A[12] = -s[6];
  A[8] = A[13] = -s[8];
  /* [v]x = [[0, -vz, vy], [vz, 0, -vx], [-vy, vx, 0]], v = sum w q */
  A[4] = A[24] = -s[3];
  A[5] = A[30] = s[2];
  A[9] = A[19] = s[3];
  A[11] = A[31] = -s[1];
  A[15] = A[20] = -s[2];
  A[16] = A[26] = s[1];
  A[21] = A[28] = A[35] = s[0];
  g[0] = s[10];
  g[1] = s[11];
  g[2] = s[12];
  g[3] = -s[13];
  g[4] = -s[14];
  g[5] = -s[15];
}

/* Solves A x = g for a symmetric positive definite A (row-major 6 x 6; its
 * lower triangle is read and overwritten by the factor L, row by row, every
 * dot product in ascending k).  Returns 1 when a pivot is not finite and
 * positive (x is then meaningless: the arithmetic runs on, there is no early
 * exit), else 0. */
PCR_HD int pcr_fgr_cholesky_solve(double *A, const double *g, double *x) {
  double y[6];
  int i, j, k, bad = 0;
  PCR_FGR_UNROLL
  for (i = 0; i < 6; i++) {
    PCR_FGR_UNROLL
    for (j = 0; j < 6; j++) {
      if (j <= i) {
        double s = A[6 * i + j];
        PCR_FGR_UNROLL
        for (k = 0; k < 6; k++)
          if (k < j) s -= A[6 * i + k] * A[6 * j + k];
        if (j == i) {
          bad |= !(s > 0.0 && s < __builtin_inf());
          A[6 * i + i] = __builtin_sqrt(s);
        } else {
          A[6 * i + j] = s / A[6 * j + j];
        }
      }
    }
  }
  PCR_FGR_UNROLL
  for (i = 0; i < 6; i++) {
    double s = g[i];
    PCR_FGR_UNROLL
    for (k = 0; k < 6; k++)
      if (k < i) s -= A[6 * i + k] * y[k];
    y[i] = s / A[6 * i + i];
  }
  PCR_FGR_UNROLL
  for (i = 5; i >= 0; i--) {
    double s = y[i];
    PCR_FGR_UNROLL
    for (k = 5; k >= 0; k--)
      if (k > i) s -= A[6 * k + i] * x[k];
    x[i] = s / A[6 * i + i];
  }
  return bad;
}

/* d[0..3): angles about x, y, z -> Rd = Rz Ry Rx (row-major); td = d[3..6) */
PCR_HD void pcr_fgr_delta(const double *d, double *Rd, double *td) {
  const double sa = PCR_FGR_SIN(d[0]), ca = PCR_FGR_COS(d[0]);
  const double sb = PCR_FGR_SIN(d[1]), cb = PCR_FGR_COS(d[1]);
  const double sc = PCR_FGR_SIN(d[2]), cc = PCR_FGR_COS(d[2]);
  Rd[0] = cc * cb;
  Rd[1] = cc * sb * sa - sc * ca;
  Rd[2] = cc * sb * ca + sc * sa;
  Rd[3] = sc * cb;
  Rd[4] = sc * sb * sa + cc * ca;
  Rd[5] = sc * sb * ca - cc * sa;
  Rd[6] = -sb;
  Rd[7] = cb * sa;
  Rd[8] = cb * ca;
  td[0] = d[3];
  td[1] = d[4];
  td[2] = d[5];
}

/* T <- Delta T: R <- Rd R, t <- Rd t + td */
PCR_HD void pcr_fgr_compose(const double *Rd, const double *td, double *R, double *t) {
  double Rn[9], tn[3];
  int i, j;
  PCR_FGR_UNROLL
  for (i = 0; i < 3; i++) {
    PCR_FGR_UNROLL
    for (j = 0; j < 3; j++)
      Rn[3 * i + j] = (Rd[3 * i] * R[j] + Rd[3 * i + 1] * R[3 + j]) + Rd[3 * i + 2] * R[6 + j];
    tn[i] = ((Rd[3 * i] * t[0] + Rd[3 * i + 1] * t[1]) + Rd[3 * i + 2] * t[2]) + td[i];
  }
  PCR_FGR_UNROLL
  for (i = 0; i < 9; i++) R[i] = Rn[i];
  PCR_FGR_UNROLL
  for (i = 0; i < 3; i++) t[i] = tn[i];
}

/* One Gauss-Newton step from the 16 sums: delta = -A^-1 g, T <- Delta T.
 * Returns 1 (T untouched) when the Cholesky factorisation fails. */
PCR_HD int pcr_fgr_step(const double *sums, double *R, double *t) {
  double A[36], g[6], x[6], Rd[9], td[3];
  int i;
  pcr_fgr_assemble(sums, A, g);
  if (pcr_fgr_cholesky_solve(A, g, x)) return 1;
  PCR_FGR_UNROLL
  for (i = 0; i < 6; i++) x[i] = -x[i];
  pcr_fgr_delta(x, Rd, td);
  pcr_fgr_compose(Rd, td, R, t);
  return 0;
}

/* ---- report ---- */
/* T = (R, t) moves the normalised target onto the normalised source; the
 * reported transform moves the source onto the target in original units:
 * R_out = R^T, t_out = m2 - R^T (d t + m1).  out: row-major 4 x 4. */
PCR_HD void pcr_fgr_report(const double *R, const double *t, const double *m1, const double *m2,
                           double d, double *out) {
  double v[3];
  int i;
  PCR_FGR_UNROLL
  for (i = 0; i < 3; i++) v[i] = d * t[i] + m1[i];
  PCR_FGR_UNROLL
  for (i = 0; i < 3; i++) {
    out[4 * i] = R[i];
    out[4 * i + 1] = R[3 + i];
    out[4 * i + 2] = R[6 + i];
    out[4 * i + 3] = m2[i] - ((R[i] * v[0] + R[3 + i] * v[1]) + R[6 + i] * v[2]);
  }
  out[12] = 0.0;
  out[13] = 0.0;
  out[14] = 0.0;
  out[15] = 1.0;
}

PCR_HD void pcr_fgr_identity(double *out) {
  int i;
  PCR_FGR_UNROLL
  for (i = 0; i < 16; i++) out[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

#endif /* PCR_FGR_H */
