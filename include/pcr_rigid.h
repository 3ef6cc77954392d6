/*
 * pcr_rigid.h -- scalar math of the batched rigid-transform estimation
 * (RANSAC + Kabsch/Horn, csrc/rigid.hip), shared by the HIP kernels (device)
 * and host C (tests compile it with gcc).  Like pcr_math.h: fixed sequences of
 * IEEE-754 operations, compiled with -ffp-contract=off, every intended FMA
 * written out.
 *
 *   sampler   pcr_rigid_mix / _draw / _triple: uint32 arithmetic only, the
 *             same three distinct slots everywhere
 *   edge      pcr_rigid_edge_ok: Open3D's CorrespondenceCheckerBasedOnEdgeLength
 *             on fp64 lengths of the fp32 points
 *   solve     pcr_rigid_from_cov: least-squares R, t (b ~ R a + t) from the
 *             centroids and the centred cross-covariance by Horn's quaternion
 *             method (largest eigenvector of a symmetric 4 x 4 by cyclic
 *             Jacobi sweeps): det R = +1 by construction, no NaN on
 *             degenerate input; pcr_rigid_solve3 feeds it three pairs
 *   score     pcr_rigid_apply: the fp32 fmaf chain that moves a point;
 *             pcr_rigid_resid2: the squared residual of one slot under it
 */
#ifndef PCR_RIGID_H
#define PCR_RIGID_H

#ifndef PCR_HD /* as pcr_math.h */
#if defined(__HIP__)
#define PCR_HD static inline __host__ __device__
#else
#define PCR_HD static inline
#endif
#endif

#ifndef PCR_RIGID_SWEEPS
#define PCR_RIGID_SWEEPS 10 /* cyclic Jacobi sweeps of the 4 x 4 */
#endif

/* ---- sampler ---- */
PCR_HD unsigned pcr_rigid_mix(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

PCR_HD unsigned pcr_rigid_draw(unsigned seed, unsigned q, unsigned h, unsigned j) {
  return pcr_rigid_mix(pcr_rigid_mix(pcr_rigid_mix(seed ^ 0x9e3779b9u) + q) + 3u * h + j);
}

/* three distinct slots of [0, m), m >= 3 */
PCR_HD void pcr_rigid_triple(unsigned seed, unsigned q, unsigned h, unsigned m, int *out) {
  unsigned a = pcr_rigid_draw(seed, q, h, 0u) % m;
  unsigned b = pcr_rigid_draw(seed, q, h, 1u) % (m - 1u);
  unsigned c = pcr_rigid_draw(seed, q, h, 2u) % (m - 2u);
  unsigned lo, hi;
  if (b >= a) b++;
  lo = a < b ? a : b;
  hi = a < b ? b : a;
  if (c >= lo) c++;
  if (c >= hi) c++;
  out[0] = (int)a;
  out[1] = (int)b;
  out[2] = (int)c;
}

/* ---- edge-length check ---- */
PCR_HD double pcr_rigid_dist(const float *p, const float *q) {
  const double dx = (double)p[0] - (double)q[0];
  const double dy = (double)p[1] - (double)q[1];
  const double dz = (double)p[2] - (double)q[2];
  return __builtin_sqrt(dx * dx + dy * dy + dz * dz);
}

/* a, b: three points each, [slot][xyz].  rho = 0 disables the ratio test;
 * an edge of zero length in either cloud always rejects. */
PCR_HD int pcr_rigid_edge_ok(const float *a, const float *b, float rho) {
  const double r = (double)rho;
  int e;
  for (e = 0; e < 3; e++) {
    const int i = e, j = e == 2 ? 0 : e + 1;
    const double la = pcr_rigid_dist(a + 3 * i, a + 3 * j);
    const double lb = pcr_rigid_dist(b + 3 * i, b + 3 * j);
    if (!(la > 0.0) || !(lb > 0.0)) return 0;
    if (la < r * lb || lb < r * la) return 0;
  }
  return 1;
}

/* ---- solve ---- */
/* One Jacobi rotation of the symmetric 4 x 4 `n` in the (p, q) plane,
 * accumulated into the eigenvector columns of `v`. */
PCR_HD void pcr_rigid_jacobi_rot(double n[4][4], double v[4][4], int p, int q) {
  const double apq = n[p][q];
  double theta, t, c, s, app, aqq;
  int k;
  if (apq == 0.0) return;
  theta = (n[q][q] - n[p][p]) / (2.0 * apq);
  /* |theta| large: theta * theta may reach +inf, t -> 0; never NaN */
  t = 1.0 / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  c = 1.0 / __builtin_sqrt(t * t + 1.0);
  s = t * c;
  app = n[p][p];
  aqq = n[q][q];
  n[p][p] = app - t * apq;
  n[q][q] = aqq + t * apq;
  n[p][q] = 0.0;
  n[q][p] = 0.0;
  for (k = 0; k < 4; k++) {
    if (k != p && k != q) {
      const double akp = n[k][p], akq = n[k][q];
      const double np_ = c * akp - s * akq;
      const double nq_ = s * akp + c * akq;
      n[k][p] = np_;
      n[p][k] = np_;
      n[k][q] = nq_;
      n[q][k] = nq_;
    }
  }
  for (k = 0; k < 4; k++) {
    const double vkp = v[k][p], vkq = v[k][q];
    v[k][p] = c * vkp - s * vkq;
    v[k][q] = s * vkp + c * vkq;
  }
}

/* ca, cb: centroids; s: centred cross-covariance sum_k a'_k b'_k^T, row-major
 * (s[3 i + j] = sum a'_i b'_j; any positive scale).  Writes R (row-major) and
 * t with b ~ R a + t. */
PCR_HD void pcr_rigid_from_cov(const double *ca, const double *cb, const double *s, double *R,
                               double *t) {
  const double sxx = s[0], sxy = s[1], sxz = s[2];
  const double syx = s[3], syy = s[4], syz = s[5];
  const double szx = s[6], szy = s[7], szz = s[8];
  double n[4][4], v[4][4];
  double w, x, y, z, nn, best;
  int i, j, sweep, bi;
  n[0][0] = sxx + syy + szz;
  n[1][1] = sxx - syy - szz;
  n[2][2] = -sxx + syy - szz;
  n[3][3] = -sxx - syy + szz;
  n[0][1] = n[1][0] = syz - szy;
  n[0][2] = n[2][0] = szx - sxz;
  n[0][3] = n[3][0] = sxy - syx;
  n[1][2] = n[2][1] = sxy + syx;
  n[1][3] = n[3][1] = szx + sxz;
  n[2][3] = n[3][2] = syz + szy;
  for (i = 0; i < 4; i++)
    for (j = 0; j < 4; j++) v[i][j] = i == j ? 1.0 : 0.0;
  for (sweep = 0; sweep < PCR_RIGID_SWEEPS; sweep++) {
    pcr_rigid_jacobi_rot(n, v, 0, 1);
    pcr_rigid_jacobi_rot(n, v, 0, 2);
    pcr_rigid_jacobi_rot(n, v, 0, 3);
    pcr_rigid_jacobi_rot(n, v, 1, 2);
    pcr_rigid_jacobi_rot(n, v, 1, 3);
    pcr_rigid_jacobi_rot(n, v, 2, 3);
  }
  bi = 0;
  best = n[0][0];
  for (i = 1; i < 4; i++) {
    /* strict: the first of equal eigenvalues; a NaN never wins */
    if (n[i][i] > best) {
      best = n[i][i];
      bi = i;
    }
  }
  w = v[0][bi];
  x = v[1][bi];
  y = v[2][bi];
  z = v[3][bi];
  nn = w * w + x * x + y * y + z * z;
  if (!(nn > 0.5 && nn < 2.0)) { /* non-finite input: the identity rotation */
    w = 1.0;
    x = y = z = 0.0;
    nn = 1.0;
  }
  nn = 1.0 / __builtin_sqrt(nn);
  w *= nn;
  x *= nn;
  y *= nn;
  z *= nn;
  R[0] = w * w + x * x - y * y - z * z;
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = w * w - x * x + y * y - z * z;
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = w * w - x * x - y * y + z * z;
  for (i = 0; i < 3; i++)
    t[i] = cb[i] - (R[3 * i] * ca[0] + R[3 * i + 1] * ca[1] + R[3 * i + 2] * ca[2]);
}

/* Least squares over m pairs a[k], b[k] ([k][xyz], doubles), ascending k:
 * centroids, centred cross-covariance, pcr_rigid_from_cov. */
PCR_HD void pcr_rigid_solve_n(const double *a, const double *b, int m, double *R, double *t) {
  double ca[3] = {0.0, 0.0, 0.0}, cb[3] = {0.0, 0.0, 0.0}, s[9];
  int i, j, k;
  for (k = 0; k < m; k++)
    for (i = 0; i < 3; i++) {
      ca[i] += a[3 * k + i];
      cb[i] += b[3 * k + i];
    }
  for (i = 0; i < 3; i++) {
    ca[i] /= (double)(m > 0 ? m : 1);
    cb[i] /= (double)(m > 0 ? m : 1);
  }
  for (i = 0; i < 9; i++) s[i] = 0.0;
  for (k = 0; k < m; k++)
    for (i = 0; i < 3; i++)
      for (j = 0; j < 3; j++) s[3 * i + j] += (a[3 * k + i] - ca[i]) * (b[3 * k + j] - cb[j]);
  pcr_rigid_from_cov(ca, cb, s, R, t);
}

/* The 3-point solve of one hypothesis: fp32 points, [slot][xyz]. */
PCR_HD void pcr_rigid_solve3(const float *a, const float *b, double *R, double *t) {
  double da[9], db[9];
  int i;
  for (i = 0; i < 9; i++) {
    da[i] = (double)a[i];
    db[i] = (double)b[i];
  }
  pcr_rigid_solve_n(da, db, 3, R, t);
}

/* R, t (fp64) -> the 12 fp32 values the scoring chain uses: R row-major, t */
PCR_HD void pcr_rigid_round(const double *R, const double *t, float *T) {
  int i;
  for (i = 0; i < 9; i++) T[i] = (float)R[i];
  for (i = 0; i < 3; i++) T[9 + i] = (float)t[i];
}

/* ---- score ---- */
/* coordinate r of the point a moved by T (pcr_rigid_round): one fp32 fmaf chain */
PCR_HD float pcr_rigid_apply1(const float *T, int r, float ax, float ay, float az) {
  return __builtin_fmaf(T[3 * r], ax,
                        __builtin_fmaf(T[3 * r + 1], ay, __builtin_fmaf(T[3 * r + 2], az, T[9 + r])));
}

/* the moved point: what the residual subtracts the target from, and what the
 * ICP (csrc/icp.hip) searches the target cloud with */
PCR_HD void pcr_rigid_apply(const float *T, float ax, float ay, float az, float *out) {
  out[0] = pcr_rigid_apply1(T, 0, ax, ay, az);
  out[1] = pcr_rigid_apply1(T, 1, ax, ay, az);
  out[2] = pcr_rigid_apply1(T, 2, ax, ay, az);
}

/* squared residual of one slot under T (pcr_rigid_round); inlier: <= tau * tau */
PCR_HD float pcr_rigid_resid2(const float *T, float ax, float ay, float az, float bx, float by,
                              float bz) {
  const float dx = pcr_rigid_apply1(T, 0, ax, ay, az) - bx;
  const float dy = pcr_rigid_apply1(T, 1, ax, ay, az) - by;
  const float dz = pcr_rigid_apply1(T, 2, ax, ay, az) - bz;
  return dx * dx + dy * dy + dz * dz;
}

#endif /* PCR_RIGID_H */
