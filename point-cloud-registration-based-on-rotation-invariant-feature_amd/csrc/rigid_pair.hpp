// rigid_pair.hpp -- what the registration solvers (rigid.hip, icp.hip,
// fgr.hip, teaser.hip) share: a pair's clouds and correspondence rows as the
// kernels address them, the 4 x 4 stores and the ordered fp64 workgroup sum.
#pragma once

#include "common.hpp"
#include "pcr_rigid.h"

namespace pcr {

struct RigidPair {
  const float *a, *b;  // the pair's clouds, [3][n1] / [3][n2]
  const int *i1, *i2;  // its correspondence rows
  int n1, n2, m;       // m: valid slots
};

__device__ inline RigidPair rigid_pair(const float* xyz1, const float* xyz2, int n1, int n2,
                                       const int* idx1, const int* idx2, const int* count,
                                       int q) {
  RigidPair pr;
  pr.a = xyz1 + (size_t)q * 3 * n1;
  pr.b = xyz2 + (size_t)q * 3 * n2;
  pr.i1 = idx1 + (size_t)q * n1;
  pr.i2 = idx2 + (size_t)q * n1;
  pr.n1 = n1;
  pr.n2 = n2;
  pr.m = min(max(count[q], 0), n1);
  return pr;
}

// slot s < m -> its source and target point; indices are clamped into the
// clouds, so a malformed correspondence row cannot read out of bounds
__device__ inline void rigid_slot(const RigidPair& pr, int s, float* a, float* b) {
  const int ia = min(max(pr.i1[s], 0), pr.n1 - 1);
  const int ib = min(max(pr.i2[s], 0), pr.n2 - 1);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    a[d] = pr.a[(size_t)d * pr.n1 + ia];
    b[d] = pr.b[(size_t)d * pr.n2 + ib];
  }
}

__device__ inline void rigid_triple_points(const RigidPair& pr, unsigned seed, int q, int h,
                                           float (&a)[9], float (&b)[9]) {
  int sl[3];
  pcr_rigid_triple(seed, (unsigned)q, (unsigned)h, (unsigned)pr.m, sl);
#pragma unroll
  for (int k = 0; k < 3; k++) rigid_slot(pr, sl[k], a + 3 * k, b + 3 * k);
}

// R, t -> the row-major 4 x 4 at tq, last row 0 0 0 1 (one thread)
__device__ inline void rigid_store_transform(double* tq, const double (&R)[9],
                                             const double (&t)[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    tq[4 * i] = R[3 * i];
    tq[4 * i + 1] = R[3 * i + 1];
    tq[4 * i + 2] = R[3 * i + 2];
    tq[4 * i + 3] = t[i];
  }
  tq[12] = 0.0;
  tq[13] = 0.0;
  tq[14] = 0.0;
  tq[15] = 1.0;
}

// the identity 4 x 4 at tq (the workgroup's first 16 threads, one entry each)
__device__ inline void rigid_store_identity(double* tq) {
  const int tid = threadIdx.x;
  if (tid < 16) tq[tid] = (tid % 5 == 0) ? 1.0 : 0.0;
}

// Sum of v[0..N) over the workgroup of NW waves, the same bits in every
// thread: the butterfly over the wave, then the waves in order.
template <int NW, int N>
__device__ inline void block_sum_d(double (&v)[N], double (*red_s)[16]) {
  static_assert(N <= 16, "row of red_s");
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < N; i++) v[i] = wave_sum_d(v[i]);
  if ((tid & (kWave - 1)) == 0) {
#pragma unroll
    for (int i = 0; i < N; i++) red_s[tid >> 6][i] = v[i];
  }
  lds_barrier();
#pragma unroll
  for (int i = 0; i < N; i++) {
    double s = red_s[0][i];
    for (int w = 1; w < NW; w++) s += red_s[w][i];
    v[i] = s;
  }
  lds_barrier();
}

}  // namespace pcr
