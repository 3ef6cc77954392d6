/*
 * pcr_gridsub.h -- scalar math of the batched grid subsampling
 * (csrc/gridsub.hip), shared by the HIP kernels (device) and
 * host C (tests compile it with gcc).  Like pcr_fgr.h: fixed sequences of
 * IEEE-754 operations, here in fp32, compiled with -ffp-contract=off.
 *
 * The reference is KPConv's grid subsampling
 * (cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:24-31,
 * 53-56, 87-94 and cpp_utils/cloud/cloud.h:120-123).  For a cloud with valid
 * points p_0 .. p_{m-1} and cell size dl > 0:
 *
 *   bounds   min_d / max_d over the valid points (pcr_gridsub_ord: an order
 *            in which -0.0 < +0.0, so they do not depend on the scan order)
 *   grid     pcr_gridsub_grid: origin_d = floorf(min_d * (1.0f / dl)) * dl,
 *            N_d = max(0, floorf((max_d - origin_d) / dl)) + 1
 *   cell     pcr_gridsub_index: i_d = max(0, floorf((p_d - origin_d) / dl));
 *            pcr_gridsub_key: ix + NX * (iy + NY * iz), unsigned 64 bit
 *   sums     every cell (a distinct key) adds its points to an fp32
 *            accumulator that starts at 0.0f, in ASCENDING POINT INDEX
 *   means    pcr_gridsub_xyz_mean: S * (float)(1.0 / (double)count), the
 *            reference's point * (1.0 / count); pcr_gridsub_feat_mean:
 *            S / (float)count, its f / count.  They differ: a sum of 5.0 over
 *            3 points is 1.6666667 as a coordinate and 1.6666666 as a feature.
 *   order    cells are output in ascending key
 *
 * Deviations from the reference, all deliberate:
 *   - origin can round above min (min = float32(4.7), dl = float32(0.1):
 *     origin 4.7000003, index -1).  The reference casts the -1 to size_t
 *     (undefined behaviour; on x86 it aliases a far cell); here the index and
 *     N_d are clamped at 0.
 *   - the reference outputs cells in the iteration order of an unordered_map
 *     (unspecified); here the order is ascending key.  Parity with the
 *     reference holds as a set of cells.
 *   - the reference keeps whichever of -0.0 / +0.0 its scan meets first as a
 *     zero minimum; here it is -0.0.  Only the sign of a zero origin changes.
 */
#ifndef PCR_GRIDSUB_H
#define PCR_GRIDSUB_H

#include "pcr_math.h"

/* per-cloud status */
#define PCR_GRIDSUB_OK 0
#define PCR_GRIDSUB_COUNT 1     /* valid count outside [1, n] */
#define PCR_GRIDSUB_NONFINITE 2 /* a non-finite coordinate among the valid points */
#define PCR_GRIDSUB_TOO_FINE 3  /* some N_d > 2^20 (or an origin that is not finite) */

/* N_d <= 2^20: keys stay below 2^60 and the fp32 quotients are exact integers */
#define PCR_GRIDSUB_MAX_DIM (1 << 20)
/* N_d is reported saturated at 2^30 + 1 */
#define PCR_GRIDSUB_SAT_DIM (1 << 30)

/* ---- bounds ---- */
/* finite floats (and the infinities) as unsigned integers of the same order,
 * -0.0 below +0.0 */
PCR_HD unsigned pcr_gridsub_ord(float v) {
  unsigned u;
  __builtin_memcpy(&u, &v, 4);
  return (u >> 31) ? ~u : (u ^ 0x80000000u);
}

PCR_HD float pcr_gridsub_unord(unsigned u) {
  float v;
  u = (u >> 31) ? (u ^ 0x80000000u) : ~u;
  __builtin_memcpy(&v, &u, 4);
  return v;
}

PCR_HD int pcr_gridsub_finite(float v) { return v - v == 0.0f; }

/* ---- grid ---- */
PCR_HD float pcr_gridsub_origin(float mn, float dl) {
  const float inv = 1.0f / dl;
  return __builtin_floorf(mn * inv) * dl;
}

/* max(0, floorf((p - origin) / dl)) as the fp32 value it is computed in */
PCR_HD float pcr_gridsub_cellf(float p, float origin, float dl) {
  const float q = __builtin_floorf((p - origin) / dl);
  return q > 0.0f ? q : 0.0f; /* a NaN gives 0 too */
}

/* the index of a valid point of a cloud with status 0 (below 2^20) */
PCR_HD int pcr_gridsub_index(float p, float origin, float dl) {
  return (int)pcr_gridsub_cellf(p, origin, dl);
}

/* origin[3] and dims[3] from the bounds; returns the status (0 or 3) */
PCR_HD int pcr_gridsub_grid(const float *mn, const float *mx, float dl, float *origin,
                            int *dims) {
  int d, status = PCR_GRIDSUB_OK;
  for (d = 0; d < 3; d++) {
    float q;
    origin[d] = pcr_gridsub_origin(mn[d], dl);
    q = pcr_gridsub_cellf(mx[d], origin[d], dl);
    dims[d] = (q < (float)PCR_GRIDSUB_SAT_DIM ? (int)q : PCR_GRIDSUB_SAT_DIM) + 1;
    if (!pcr_gridsub_finite(origin[d]) || dims[d] > PCR_GRIDSUB_MAX_DIM)
      status = PCR_GRIDSUB_TOO_FINE;
  }
  return status;
}

/* ---- cell ---- */
PCR_HD unsigned long long pcr_gridsub_key(int ix, int iy, int iz, int nx, int ny) {
  return (unsigned long long)ix +
         (unsigned long long)nx * ((unsigned long long)iy + (unsigned long long)ny *
                                                                (unsigned long long)iz);
}

/* bits needed for the keys 0 .. nx * ny * nz - 1 (0 for a single cell) */
PCR_HD int pcr_gridsub_key_bits(int nx, int ny, int nz) {
  unsigned long long last =
      (unsigned long long)nx * (unsigned long long)ny * (unsigned long long)nz - 1ull;
  int bits = 0;
  while (bits < 64 && (last >> bits) != 0ull) bits++;
  return bits;
}

/* ---- means ---- */
PCR_HD float pcr_gridsub_xyz_mean(float sum, int count) {
  return sum * (float)(1.0 / (double)count);
}

PCR_HD float pcr_gridsub_feat_mean(float sum, int count) { return sum / (float)count; }

#endif /* PCR_GRIDSUB_H */
