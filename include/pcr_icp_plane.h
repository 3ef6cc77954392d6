/*
 * pcr_icp_plane.h -- scalar math of the batched point-to-plane ICP
 * (csrc/icp_plane.hip), shared by the HIP kernel (device) and
 * host C (tests compile it with gcc).  Like pcr_fgr.h, whose 6 x 6 Cholesky,
 * pcr_fgr_delta and pcr_fgr_compose it reuses (together they are Open3D's
 * TransformVector6dToMatrix4d update): fixed sequences of IEEE-754 fp64
 * operations, compiled with -ffp-contract=off.
 *
 *   terms  pcr_icp_plane_accumulate: one correspondence's residual
 *          r = (m - b) . n, its Jacobian row J = (m x n, n) and its 27 terms
 *   step   pcr_icp_plane_assemble: A = sum J J^T (6 x 6) and g = sum J r from
 *          the 27 sums; pcr_icp_plane_step: assemble, pcr_fgr_cholesky_solve
 *          with its failure rule, x = -x, pcr_fgr_delta, pcr_fgr_compose
 */
#ifndef PCR_ICP_PLANE_H
#define PCR_ICP_PLANE_H

#include "pcr_fgr.h"

#define PCR_ICP_PLANE_MIN_CORR 6 /* fewer correspondences: status 1 */
#define PCR_ICP_PLANE_NSUM 27    /* sums per iteration */

/* ---- terms ---- */
/* Adds one correspondence to the 27 sums
 *   [0..21) the upper triangle of J J^T in row order (00 01 .. 05 11 .. 55):
 *           entry (i, j >= i) is sum i (11 - i) / 2 + j
 *   [21..27) J r
 * m: the fp32 moved source point Evaluate searched with, b: its target, n:
 * the target's normal, all widened to fp64; r = (m - b) . n, J = (m x n, n). */
PCR_HD void pcr_icp_plane_accumulate(const float *m, const float *b, const float *n,
                                     double *sums) {
  const double m0 = (double)m[0], m1 = (double)m[1], m2 = (double)m[2];
  const double n0 = (double)n[0], n1 = (double)n[1], n2 = (double)n[2];
  const double r = ((m0 - (double)b[0]) * n0 + (m1 - (double)b[1]) * n1) + (m2 - (double)b[2]) * n2;
  double J[6];
  int i, j;
  J[0] = m1 * n2 - m2 * n1;
  J[1] = m2 * n0 - m0 * n2;
  J[2] = m0 * n1 - m1 * n0;
  J[3] = n0;
  J[4] = n1;
  J[5] = n2;
  PCR_FGR_UNROLL
  for (i = 0; i < 6; i++) {
    PCR_FGR_UNROLL
    for (j = 0; j < 6; j++)
      if (j >= i) sums[i * (11 - i) / 2 + j] += J[i] * J[j];
  }
  PCR_FGR_UNROLL
  for (i = 0; i < 6; i++) sums[21 + i] += J[i] * r;
}

/* ---- step ---- */
/* A (row-major 6 x 6, the lower triangle mirrored) and g from the 27 sums */
PCR_HD void pcr_icp_plane_assemble(const double *s, double *A, double *g) {
  int i, j;
  PCR_FGR_UNROLL
  for (i = 0; i < 6; i++) {
    PCR_FGR_UNROLL
    for (j = 0; j < 6; j++)
      if (j >= i) A[6 * i + j] = A[6 * j + i] = s[i * (11 - i) / 2 + j];
  }
  PCR_FGR_UNROLL
  for (i = 0; i < 6; i++) g[i] = s[21 + i];
}

/* One Gauss-Newton step from the 27 sums: x = -A^-1 g, T <- Delta(x) T.
 * Returns 1 (T untouched) when the Cholesky factorisation meets a pivot that
 * is not finite and positive. */
PCR_HD int pcr_icp_plane_step(const double *sums, double *R, double *t) {
  double A[36], g[6], x[6], Rd[9], td[3];
  int i;
  pcr_icp_plane_assemble(sums, A, g);
  if (pcr_fgr_cholesky_solve(A, g, x)) return 1;
  PCR_FGR_UNROLL
  for (i = 0; i < 6; i++) x[i] = -x[i];
  pcr_fgr_delta(x, Rd, td);
  pcr_fgr_compose(Rd, td, R, t);
  return 0;
}

#endif /* PCR_ICP_PLANE_H */
