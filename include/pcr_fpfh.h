/*
 * pcr_fpfh.h -- scalar math of the batched FPFH descriptors (csrc/fpfh.hip;
 * DESIGN.md 4.8f), shared by the HIP kernels (device) and host C (tests
 * compile it with gcc).  Like pcr_gridsub.h: fixed sequences of IEEE-754
 * operations, in fp32 unless said otherwise, compiled with
 * -ffp-contract=off; every fused multiply-add is written out.
 *
 * The algorithm is Open3D's ComputeFPFHFeature with a hybrid search
 * (KDTreeSearchParamHybrid(radius, max_nn)): per point i the neighbour set
 * N(i) is what the search returns without the point itself.  Open3D is not
 * installed and works in double; this is a restatement in fp32 whose order is
 * the contract (parity against Open3D is unpinned, as for the normals).
 *
 *   N(i)    slots s = 0 .. min(k, n) - 1 of the ascending neighbour lists, in
 *           ascending s; slot (j, d) belongs when pcr_fpfh_in_set: 0 <= j < n,
 *           j != i, 0 < d <= radius * radius (fp32 product; a NaN d fails).
 *           m = |N(i)|
 *   pair    pcr_fpfh_pair(p_i, n_i, p_j, n_j) -> (f0, f1, f2): Open3D's
 *           ComputePairFeatures.  Its test acos|a1| > acos|a2| is |a1| < |a2|.
 *           f0 = atan2 in fp64 (pcr_fpfh_atan2_d on pcr_atan_d) of the fp32 dot
 *           products, rounded once to fp32.  Degenerate pairs give (0, 0, 0)
 *           and are binned like any other
 *   bins    pcr_fpfh_bins: floor(11 (f0 + pi) / 2 pi), floor(11 (f1 + 1) / 2),
 *           floor(11 (f2 + 1) / 2), clamped to [0, 10], a NaN to 0; channels
 *           h0, 11 + h1, 22 + h2
 *   spfh    pcr_fpfh_spfh: (float)count_c * (100.0f / (float)m); 0 when m = 0
 *   fpfh    acc_c = sum over N(i) in ascending slot of spfh[j][c] / d, from
 *           0.0f; S_g = the sum of group g's 11 acc in ascending channel, from
 *           0.0f; pcr_fpfh_value: acc_c * (100.0f / S_g) + spfh[i][c], a
 *           multiply and an add; with S_g == 0 the scale is left out
 */
#ifndef PCR_FPFH_H
#define PCR_FPFH_H

#include "pcr_math.h"

#define PCR_FPFH_BINS 11
#define PCR_FPFH_CHANNELS 33
#define PCR_FPFH_MAX_K 128

/* (float)pi and 2 * (float)pi */
#define PCR_FPFH_PI_F 3.14159274101257324f
#define PCR_FPFH_2PI_F 6.28318548202514648f

/* ---- neighbour set ---- */
PCR_HD int pcr_fpfh_in_set(int j, float d, int i, int n, float r2) {
  return j >= 0 && j < n && j != i && d > 0.0f && d <= r2;
}

/* ---- pair feature ---- */
/* atan2(y, x) in fp64 on pcr_atan_d: the quadrant from the signs (signed zeros
 * as C's atan2), a NaN argument gives NaN */
PCR_HD double pcr_fpfh_atan2_d(double y, double x) {
  double r;
  if (x != x || y != y) return x + y;
  if (y == 0.0)
    r = __builtin_signbit(x) ? PCR_PI : 0.0;
  else if (x == 0.0)
    r = PCR_PIO2;
  else {
    r = pcr_atan_d(__builtin_fabs(y) / __builtin_fabs(x));
    if (x < 0.0) r = PCR_PI - r;
  }
  return __builtin_signbit(y) ? -r : r;
}

/* a x b, every product and difference rounded on its own */
PCR_HD void pcr_fpfh_cross(const float a[3], const float b[3], float o[3]) {
  const float p0 = a[1] * b[2], q0 = a[2] * b[1];
  const float p1 = a[2] * b[0], q1 = a[0] * b[2];
  const float p2 = a[0] * b[1], q2 = a[1] * b[0];
  o[0] = p0 - q0;
  o[1] = p1 - q1;
  o[2] = p2 - q2;
}

/* f = {f0, f1, f2} of the pair (i, j) */
PCR_HD void pcr_fpfh_pair(const float pi[3], const float ni[3], const float pj[3],
                          const float nj[3], float f[3]) {
  float dp[3], n1[3], n2[3], v[3], w[3], f3, a1, a2, vn, y, x;
  int a, swap;
  f[0] = f[1] = f[2] = 0.0f;
  for (a = 0; a < 3; a++) dp[a] = pj[a] - pi[a];
  f3 = __builtin_sqrtf(pcr_sumsq3f(dp[0], dp[1], dp[2]));
  if (f3 == 0.0f) return;
  a1 = pcr_dot3f(ni[0], ni[1], ni[2], dp[0], dp[1], dp[2]) / f3;
  a2 = pcr_dot3f(nj[0], nj[1], nj[2], dp[0], dp[1], dp[2]) / f3;
  swap = __builtin_fabsf(a1) < __builtin_fabsf(a2);
  for (a = 0; a < 3; a++) {
    n1[a] = swap ? nj[a] : ni[a];
    n2[a] = swap ? ni[a] : nj[a];
    dp[a] = swap ? -dp[a] : dp[a];
  }
  pcr_fpfh_cross(dp, n1, v);
  vn = __builtin_sqrtf(pcr_sumsq3f(v[0], v[1], v[2]));
  if (vn == 0.0f) return;
  for (a = 0; a < 3; a++) v[a] = v[a] / vn;
  pcr_fpfh_cross(n1, v, w);
  y = pcr_dot3f(w[0], w[1], w[2], n2[0], n2[1], n2[2]);
  x = pcr_dot3f(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2]);
  f[0] = (float)pcr_fpfh_atan2_d((double)y, (double)x);
  f[1] = pcr_dot3f(v[0], v[1], v[2], n2[0], n2[1], n2[2]);
  f[2] = swap ? -a2 : a1;
}

/* ---- bins ---- */
/* floor(t) clamped to [0, 10]; a NaN gives 0 */
PCR_HD int pcr_fpfh_bin(float t) {
  const float q = __builtin_floorf(t);
  return q >= 10.0f ? 10 : (q > 0.0f ? (int)q : 0);
}

/* the three channels a pair feature counts in */
PCR_HD void pcr_fpfh_bins(const float f[3], int ch[3]) {
  ch[0] = pcr_fpfh_bin((11.0f * (f[0] + PCR_FPFH_PI_F)) / PCR_FPFH_2PI_F);
  ch[1] = PCR_FPFH_BINS + pcr_fpfh_bin((11.0f * (f[1] + 1.0f)) * 0.5f);
  ch[2] = 2 * PCR_FPFH_BINS + pcr_fpfh_bin((11.0f * (f[2] + 1.0f)) * 0.5f);
}

/* ---- SPFH ---- */
PCR_HD float pcr_fpfh_spfh(int count, int m) {
  return m > 0 ? (float)count * (100.0f / (float)m) : 0.0f;
}

/* ---- FPFH ---- */
/* one term of acc: acc + spfh_j / d */
PCR_HD float pcr_fpfh_add(float acc, float spfh_j, float d) { return acc + spfh_j / d; }

/* S_g of 11 consecutive acc */
PCR_HD float pcr_fpfh_group_sum(const float *acc) {
  float s = 0.0f;
  int c;
  for (c = 0; c < PCR_FPFH_BINS; c++) s = s + acc[c];
  return s;
}

PCR_HD float pcr_fpfh_value(float acc, float group_sum, float spfh_i) {
  float t = acc;
  if (group_sum != 0.0f) t = acc * (100.0f / group_sum);
  return t + spfh_i;
}

#endif /* PCR_FPFH_H */
