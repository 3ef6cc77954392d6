/*
 * pcr_hybrid.h -- scalar math of the batched hybrid (radius + max_nn)
 * neighbour search (csrc/hybrid_search.hip), shared by the HIP
 * kernels (device) and host C (tests compile it with gcc).  Like pcr_fpfh.h:
 * fixed sequences of IEEE-754 operations in fp32, compiled with
 * -ffp-contract=off; every fused multiply-add is written out.
 *
 * The search is Open3D's KDTreeSearchParamHybrid(radius, max_nn) of a cloud
 * against itself.  For a cloud with valid points p_0 .. p_{m-1}:
 *
 *   distance  pcr_hybrid_dist(p_i, p_j): t = p_i - p_j, fmaf(tz, tz, fmaf(ty,
 *             ty, tx * tx)) -- bit for bit the KNN's distance
 *   radius    r2 = radius * radius (fp32); j is within the radius of i when
 *             pcr_hybrid_in_radius: d <= r2 (a NaN or infinite d fails)
 *   row       the valid j within the radius of i (j = i included), ascending
 *             by pcr_hybrid_key (bits of d, j): ties go to the lower index;
 *             cut to the first k
 *   empty     an unfilled slot holds (+inf, -1): PCR_HYBRID_EMPTY as a key,
 *             above every key of a point within a finite radius
 *
 * That rule is the whole contract; it knows nothing of cells.  The grid below
 * is how the kernels avoid looking at every pair, and it is built so that it
 * cannot change the result (DESIGN.md 4.8g has the argument in full):
 *
 *   bounds    mn_d / mx_d over the valid points whose three coordinates are
 *             finite (pcr_hybrid_finite3); the other points are in no cell
 *   grid      pcr_hybrid_grid: origin = mn, side = max(radius * (1 + 2^-8),
 *             largest extent / G), inv = 1.0f / side, dims_d = the cell of
 *             mx_d + 1 <= G <= PCR_HYBRID_MAX_DIM.  One cell (dims 1, 1, 1)
 *             when there is no finite point, when an extent or the side is
 *             not finite, or when r2 < 2^-100
 *   cell      pcr_hybrid_cell: min(max(floorf((p - origin) * inv), 0), dims -
 *             1); monotone in p, and two points with d <= r2 are at most one
 *             cell apart along every axis
 */
#ifndef PCR_HYBRID_H
#define PCR_HYBRID_H

#include "pcr_math.h"

#define PCR_HYBRID_MAX_K 128
/* in-radius keys a wave of the query kernel buffers per query; a query with
 * more than this within its radius selects by passes over its cells instead */
#define PCR_HYBRID_WAVE_CAP 512
/* cells per axis, at most */
#define PCR_HYBRID_MAX_DIM 32
/* side >= radius * (1 + 2^-8) */
#define PCR_HYBRID_MARGIN 1.00390625f
/* below this r2 the grid is one cell (2^-100: far above the subnormals, so
 * every rounding in the exactness argument is a relative one) */
#define PCR_HYBRID_MIN_R2 7.8886090522101181e-31f

/* (+inf, -1) */
#define PCR_HYBRID_EMPTY 0x7F800000FFFFFFFFull

/* ---- distance and selection ---- */
PCR_HD float pcr_hybrid_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float tx = ax - bx, ty = ay - by, tz = az - bz;
  return __builtin_fmaf(tz, tz, __builtin_fmaf(ty, ty, tx * tx));
}

PCR_HD int pcr_hybrid_in_radius(float d, float r2) { return d <= r2; }

PCR_HD unsigned pcr_hybrid_bits(float v) {
  unsigned u;
  __builtin_memcpy(&u, &v, 4);
  return u;
}

/* d >= +0 and not NaN for a point within the radius, so the bits order as d */
PCR_HD unsigned long long pcr_hybrid_key(float d, int j) {
  return ((unsigned long long)pcr_hybrid_bits(d) << 32) | (unsigned long long)(unsigned)j;
}

PCR_HD float pcr_hybrid_key_dist(unsigned long long key) {
  const unsigned u = (unsigned)(key >> 32);
  float v;
  __builtin_memcpy(&v, &u, 4);
  return v;
}

PCR_HD int pcr_hybrid_key_index(unsigned long long key) { return (int)(unsigned)key; }

/* ---- grid ---- */
PCR_HD int pcr_hybrid_finite(float v) { return v - v == 0.0f; }

PCR_HD int pcr_hybrid_finite3(float x, float y, float z) {
  return pcr_hybrid_finite(x) && pcr_hybrid_finite(y) && pcr_hybrid_finite(z);
}

/* G for clouds of n points: the smallest g with 2 g^3 >= n, at most
 * PCR_HYBRID_MAX_DIM (a grid bounded by the extent holds about two points per
 * cell; one bounded by the radius is coarser) */
PCR_HD int pcr_hybrid_gmax(int n) {
  int g = 1;
  while (g < PCR_HYBRID_MAX_DIM && 2 * g * g * g < n) g++;
  return g;
}

PCR_HD int pcr_hybrid_cell(float p, float origin, float inv, int dim) {
  float q;
  if (dim <= 1) return 0;
  q = __builtin_floorf((p - origin) * inv);
  if (!(q > 0.0f)) return 0; /* a NaN too */
  return q < (float)(dim - 1) ? (int)q : dim - 1;
}

/* origin[3], *inv and dims[3] from the bounds of the finite valid points
 * (any = 0: there is none), the radius and G */
PCR_HD void pcr_hybrid_grid(const float *mn, const float *mx, int any, float radius, int gmax,
                            float *origin, float *inv, int *dims) {
  const float r2 = radius * radius;
  float ext = 0.0f, side, side_e, iv;
  int d;
  for (d = 0; d < 3; d++) {
    origin[d] = 0.0f;
    dims[d] = 1;
  }
  *inv = 0.0f;
  if (!any) return;
  for (d = 0; d < 3; d++) {
    const float e = mx[d] - mn[d];
    if (e > ext) ext = e; /* finite bounds: e >= 0, or +inf when it overflows */
  }
  side = radius * PCR_HYBRID_MARGIN;
  side_e = ext / (float)gmax;
  if (side_e > side) side = side_e;
  if (!pcr_hybrid_finite(ext) || !pcr_hybrid_finite(side) || !(r2 >= PCR_HYBRID_MIN_R2)) return;
  iv = 1.0f / side;
  if (!pcr_hybrid_finite(iv)) return;
  *inv = iv;
  for (d = 0; d < 3; d++) {
    origin[d] = mn[d];
    dims[d] = pcr_hybrid_cell(mx[d], mn[d], iv, gmax) + 1;
  }
}

#endif /* PCR_HYBRID_H */
