// icp_plane.hip -- batched point-to-plane ICP for gfx950 (Open3D's
// TransformationEstimationPointToPlane inside registration_icp): the
// refinement the scan chain's target normals call for.  The contract is
// DESIGN.md 4.8i, the scalar math include/pcr_icp_plane.h (on pcr_fgr.h's
// Cholesky, delta and compose), pcr_rigid.h and pcr_sumsq3f.
//
//   icp_plane_kernel  the loop of icp_loop.hpp around the Gauss-Newton step.
//     One pass per iteration: after the scan a thread writes corr, gathers
//     the chosen target's three normal components from global memory (the
//     normals never enter LDS) and adds the point's 27 Gauss-Newton terms to
//     M and E in the same pass.  The 29 sums go through block_sum_d twice
//     (its rows hold 16).  Wave 0 solves (pcr_icp_plane_step) and hands the
//     Cholesky's verdict on with R, t.  counts1 / counts2 (either may be
//     NULL) bound the points and the targets; the strides only choose whether
//     the target stays in LDS.
#include "common.hpp"
#include "icp_loop.hpp"
#include "pcr_icp_plane.h"
#include "rigid_pair.hpp"

namespace pcr {

constexpr int kIPSums = 2 + PCR_ICP_PLANE_NSUM;  // M, E and the Gauss-Newton sums
constexpr int kIPRed = 16;                       // sums per block_sum_d call: a row of red_s

// acc[O ..) through block_sum_d, kIPRed sums at a time
template <int O>
__device__ inline void icp_plane_sum(double (&acc)[kIPSums], double (*red_s)[16]) {
  constexpr int N = kIPSums - O < kIPRed ? kIPSums - O : kIPRed;
  double v[N];
#pragma unroll
  for (int i = 0; i < N; i++) v[i] = acc[O + i];
  block_sum_d<kIW>(v, red_s);
  // the sums are pinned here: only wave 0 reads most of them, and additions
  // sunk into its branch would leave every wave's partials live until then
#pragma unroll
  for (int i = 0; i < N; i++) {
    asm volatile("" : "+v"(v[i]));
    acc[O + i] = v[i];
  }
  if constexpr (O + N < kIPSums) icp_plane_sum<O + N>(acc, red_s);
}

__global__ __launch_bounds__(kIT) void icp_plane_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2,
    const float* __restrict__ normals2, int n1, int n2, const int* __restrict__ counts1,
    const int* __restrict__ counts2, const double* __restrict__ init, float tau2, int max_iters,
    double rel_fitness, double rel_rmse, int cap, double* __restrict__ transform,
    int* __restrict__ corr, int* __restrict__ num_corr, double* __restrict__ fitness,
    double* __restrict__ rmse, int* __restrict__ iterations, int* __restrict__ status) {
  const IcpLds L = icp_lds(cap);
  float* const tg = L.tg;
  const int q = blockIdx.x, tid = threadIdx.x;
  const float* A = xyz1 + (size_t)q * 3 * n1;
  const float* B = xyz2 + (size_t)q * 3 * n2;
  const float* N = normals2 + (size_t)q * 3 * n2;
  int* cq = corr + (size_t)q * n1;
  int v1 = n1, v2 = n2;
  ragged_valid(q, v1, v2, RaggedCounts{counts1, counts2});
  // an empty source: no evaluation, the init comes back with status 1
  const bool empty = v1 == 0;
  const bool whole = n2 <= cap;  // the target stays in LDS
  const int tiles = (v1 + kITile - 1) / kITile;
  for (int i = v1 + tid; i < n1; i += kIT) cq[i] = -1;  // corr past the source's points

  double R[9], t[3];
  float T[12];
  icp_start(init, q, R, t);
  pcr_rigid_round(R, t, T);
  if (whole) {
    icp_stage(tg, cap, B, n2, 0, v2);
    lds_barrier();
  }

  double M = 0.0, pfit = 0.0, prmse = 0.0;
  int it = 0, st = empty ? 1 : 2;
  for (; !empty; it++) {  // at most max_iters + 1 evaluations
    // ---- Evaluate(T) and the Gauss-Newton sums of its correspondences
    double acc[kIPSums];  // M, E, the 27 sums
#pragma unroll
    for (int i = 0; i < kIPSums; i++) acc[i] = 0.0;
    for (int tile = 0; tile < tiles; tile++) {
      const int s0 = tile * kITile;
      float m[kIP][3], bd[kIP];
      int bj[kIP];
#pragma unroll
      for (int k = 0; k < kIP; k++) {
        const int i = s0 + k * kIT + tid;
        if (i < v1) {
          pcr_rigid_apply(T, A[i], A[(size_t)n1 + i], A[(size_t)2 * n1 + i], m[k]);
        } else {
          m[k][0] = m[k][1] = m[k][2] = __builtin_nanf("");
        }
        bd[k] = __builtin_inff();
        bj[k] = -1;
      }
      // k = 0 is the thread's lowest point
      icp_nearest(tg, cap, whole, B, n2, v2, s0 + tid < v1, m, bd, bj);
#pragma unroll
      for (int k = 0; k < kIP; k++) {
        const int i = s0 + k * kIT + tid;
        // bj < v2 <= n2 by the scan's bound: the gathers stay inside the pair
        if (!(bj[k] >= 0 && bj[k] < v2 && bd[k] <= tau2)) bj[k] = -1;
        if (bj[k] >= 0) {
          float b[3], nm[3];
#pragma unroll
          for (int d = 0; d < 3; d++) {
            b[d] = whole ? tg[d * cap + bj[k]] : B[(size_t)d * n2 + bj[k]];
            nm[d] = N[(size_t)d * n2 + bj[k]];
          }
          acc[0] += 1.0;
          acc[1] += (double)bd[k];
          pcr_icp_plane_accumulate(m[k], b, nm, acc + 2);
        }
        if (i < v1) cq[i] = bj[k];
      }
    }
    // M, E and the 27 sums through block_sum_d, kIPRed at a time
    icp_plane_sum<0>(acc, L.red_s);
    M = acc[0];
    const int end = icp_verdict<PCR_ICP_PLANE_MIN_CORR>(M, acc[1], v1, it, max_iters, rel_fitness,
                                                        rel_rmse, pfit, prmse);
    if (end >= 0) {
      st = end;
      break;
    }
    // ---- the step: wave 0 solves, T stays as evaluated when the pivots fail
    if (tid < kWave) {
      const int bad = pcr_icp_plane_step(acc + 2, R, t);
      if (tid == 0) icp_publish<true>(L.sol_s, R, t, bad);
    }
    lds_barrier();
    if (icp_fetch<true>(L.sol_s, R, t)) {
      st = 3;
      break;
    }
    pcr_rigid_round(R, t, T);
  }

  if (tid == 0)
    icp_store(q, R, t, M, pfit, prmse, it, st, transform, num_corr, fitness, rmse, iterations,
              status);
}

}  // namespace pcr

using namespace pcr;

extern "C" pcr_status pcr_icp_point_to_plane(
    const float* xyz1, const float* xyz2, const float* normals2, int p, int n1, int n2,
    const int* counts1, const int* counts2, const double* init, float max_dist, int max_iters,
    double rel_fitness, double rel_rmse, double* transform, int* corr, int* num_corr,
    double* fitness, double* rmse, int* iterations, int* status, void* stream) {
  if (icp_check("icp_point_to_plane", p, n1, n2, max_dist, max_iters, rel_fitness, rel_rmse) !=
      PCR_OK)
    return PCR_ERR_INVALID;
  if (p == 0) return PCR_OK;
  PCR_REQUIRE(xyz1 && xyz2 && normals2 && transform && corr && num_corr && fitness && rmse &&
                  iterations && status,
              "icp_point_to_plane: null pointer");
  icp_launch(icp_plane_kernel, p, n2, stream, xyz1, xyz2, normals2, n1, n2, counts1, counts2, init,
             max_dist * max_dist, max_iters, rel_fitness, rel_rmse, icp_cap(n2), transform, corr,
             num_corr, fitness, rmse, iterations, status);
  return launch_status("icp_point_to_plane");
}
