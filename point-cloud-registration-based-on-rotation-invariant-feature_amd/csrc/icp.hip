// icp.hip -- batched point-to-point ICP for gfx950: the reference's
// register_one_pair(func='icp') (utils/open3d_func.py:63-72, Open3D
// registration_icp on the CPU, one pair at a time), as a solver of its own or
// as the refinement of pcr_rigid_ransac's transform.  The contract is
// DESIGN.md 4.8b, the scalar math include/pcr_rigid.h + pcr_sumsq3f.
//
//   icp_kernel  the loop of icp_loop.hpp around the Kabsch step: M, E, the
//     centroid sums and, in a second pass, the centred cross-covariance of
//     the correspondences; wave 0 solves (pcr_rigid_from_cov).  kResident
//     (n1 <= one tile): the source points, their nearest target and its
//     coordinates stay in registers between the evaluation and the
//     covariance pass, and corr is written once at the end; larger n1 keeps
//     the nearest index in corr and re-reads the points.  Ragged pairs come
//     as the RG pack of common.hpp.
#include "common.hpp"
#include "icp_loop.hpp"
#include "pcr_rigid.h"
#include "rigid_pair.hpp"

namespace pcr {

template <bool kResident, typename... RG>
__global__ __launch_bounds__(kIT) void icp_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n1, int n2,
    const double* __restrict__ init, float tau2, int max_iters, double rel_fitness,
    double rel_rmse, int cap, double* __restrict__ transform, int* __restrict__ corr,
    int* __restrict__ num_corr, double* __restrict__ fitness, double* __restrict__ rmse,
    int* __restrict__ iterations, int* __restrict__ status, RG... rg) {
  const IcpLds L = icp_lds(cap);
  float* const tg = L.tg;
  const int q = blockIdx.x, tid = threadIdx.x;
  const float* A = xyz1 + (size_t)q * 3 * n1;
  const float* B = xyz2 + (size_t)q * 3 * n2;
  int* cq = corr + (size_t)q * n1;
  int v1 = n1, v2 = n2;
  ragged_valid(q, v1, v2, rg...);
  // an empty source: no evaluation, the init comes back with status 1
  const bool empty = sizeof...(RG) != 0 && v1 == 0;
  const bool whole = n2 <= cap;  // the target stays in LDS
  const int tiles = kResident ? 1 : (v1 + kITile - 1) / kITile;
  if (sizeof...(RG) != 0 && (!kResident || empty)) {  // corr past the source's points
    for (int i = v1 + tid; i < n1; i += kIT) cq[i] = -1;
  }

  double R[9], t[3];
  float T[12];
  icp_start(init, q, R, t);
  pcr_rigid_round(R, t, T);
  if (whole) {
    icp_stage(tg, cap, B, n2, 0, v2);
    lds_barrier();
  }

  // kResident: the tile's points, their nearest target and its coordinates
  float a[kIP][3], b[kIP][3];
  int bj[kIP];
  double M = 0.0, pfit = 0.0, prmse = 0.0;
  int it = 0, st = empty ? 1 : 2;
  if (empty) {
#pragma unroll
    for (int k = 0; k < kIP; k++) bj[k] = -1;
  }
  for (; !empty; it++) {  // at most max_iters + 1 evaluations
    // ---- Evaluate(T): nearest targets, M, E and the centroid sums
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int tile = 0; tile < tiles; tile++) {
      const int s0 = tile * kITile;
      float m[kIP][3], bd[kIP];
#pragma unroll
      for (int k = 0; k < kIP; k++) {
        const int i = s0 + k * kIT + tid;
        if (i < v1) {
#pragma unroll
          for (int d = 0; d < 3; d++) a[k][d] = A[(size_t)d * n1 + i];
          pcr_rigid_apply(T, a[k][0], a[k][1], a[k][2], m[k]);
        } else {
          a[k][0] = a[k][1] = a[k][2] = 0.0f;
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
        if (!(bj[k] >= 0 && bd[k] <= tau2)) bj[k] = -1;
        if (bj[k] >= 0) {
#pragma unroll
          for (int d = 0; d < 3; d++)
            b[k][d] = whole ? tg[d * cap + bj[k]] : B[(size_t)d * n2 + bj[k]];
          acc[0] += 1.0;
          acc[1] += (double)bd[k];
#pragma unroll
          for (int d = 0; d < 3; d++) {
            acc[2 + d] += (double)a[k][d];
            acc[5 + d] += (double)b[k][d];
          }
        }
        if (!kResident && i < v1) cq[i] = bj[k];
      }
    }
    block_sum_d<kIW>(acc, L.red_s);
    M = acc[0];
    const int end = icp_verdict<3>(M, acc[1], v1, it, max_iters, rel_fitness, rel_rmse, pfit,
                                   prmse);
    if (end >= 0) {
      st = end;
      break;
    }
    // ---- least squares over the correspondences, from the original points
    double ca[3], cb[3], cov[9];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      ca[d] = acc[2 + d] / M;
      cb[d] = acc[5 + d] / M;
    }
#pragma unroll
    for (int i = 0; i < 9; i++) cov[i] = 0.0;
    for (int tile = 0; tile < tiles; tile++) {
#pragma unroll
      for (int k = 0; k < kIP; k++) {
        if (!kResident) {
          const int i = tile * kITile + k * kIT + tid;
          bj[k] = i < v1 ? cq[i] : -1;  // this thread's own store
          if (bj[k] >= 0) {
#pragma unroll
            for (int d = 0; d < 3; d++) {
              a[k][d] = A[(size_t)d * n1 + i];
              b[k][d] = B[(size_t)d * n2 + bj[k]];
            }
          }
        }
        if (bj[k] >= 0) {
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
              cov[3 * i + j] += ((double)a[k][i] - ca[i]) * ((double)b[k][j] - cb[j]);
        }
      }
    }
    block_sum_d<kIW>(cov, L.red_s);
    if (tid < kWave) {
      pcr_rigid_from_cov(ca, cb, cov, R, t);
      if (tid == 0) icp_publish(L.sol_s, R, t);
    }
    lds_barrier();
    icp_fetch(L.sol_s, R, t);
    pcr_rigid_round(R, t, T);
  }

  if (kResident) {
#pragma unroll
    for (int k = 0; k < kIP; k++) {
      const int i = k * kIT + tid;
      if (i < n1) cq[i] = bj[k];
    }
  }
  if (tid == 0)
    icp_store(q, R, t, M, pfit, prmse, it, st, transform, num_corr, fitness, rmse, iterations,
              status);
}

}  // namespace pcr

using namespace pcr;

// Both entry points: the checks, then icp_kernel<kResident, RG...> by the
// stride n1.  The paths follow the strides; the result does not depend on
// them.
template <typename... RG>
static pcr_status icp_run(const char* name, const char* what, const float* xyz1,
                          const float* xyz2, int p, int n1, int n2, const double* init,
                          float max_dist, int max_iters, double rel_fitness, double rel_rmse,
                          double* transform, int* corr, int* num_corr, double* fitness,
                          double* rmse, int* iterations, int* status, void* stream, RG... rg) {
  if (icp_check(name, p, n1, n2, max_dist, max_iters, rel_fitness, rel_rmse) != PCR_OK)
    return PCR_ERR_INVALID;
  if (p == 0) return PCR_OK;
  PCR_REQUIRE(xyz1 && xyz2 && transform && corr && num_corr && fitness && rmse && iterations &&
                  status,
              "%s: null pointer", what);
  const auto kernel = n1 <= kITile ? icp_kernel<true, RG...> : icp_kernel<false, RG...>;
  icp_launch(kernel, p, n2, stream, xyz1, xyz2, n1, n2, init, max_dist * max_dist, max_iters,
             rel_fitness, rel_rmse, icp_cap(n2), transform, corr, num_corr, fitness, rmse,
             iterations, status, rg...);
  return launch_status(what);
}

extern "C" pcr_status pcr_icp_point_to_point(const float* xyz1, const float* xyz2, int p, int n1,
                                             int n2, const double* init, float max_dist,
                                             int max_iters, double rel_fitness, double rel_rmse,
                                             double* transform, int* corr, int* num_corr,
                                             double* fitness, double* rmse, int* iterations,
                                             int* status, void* stream) {
  return icp_run("icp_point_to_point", "icp_point_to_point", xyz1, xyz2, p, n1, n2, init,
                 max_dist, max_iters, rel_fitness, rel_rmse, transform, corr, num_corr, fitness,
                 rmse, iterations, status, stream);
}

// the range errors carry the dense entry point's name
extern "C" pcr_status pcr_icp_point_to_point_ragged(
    const float* xyz1, const float* xyz2, int p, int n1, int n2, const int* counts1,
    const int* counts2, const double* init, float max_dist, int max_iters, double rel_fitness,
    double rel_rmse, double* transform, int* corr, int* num_corr, double* fitness, double* rmse,
    int* iterations, int* status, void* stream) {
  return icp_run("icp_point_to_point", "icp_point_to_point_ragged", xyz1, xyz2, p, n1, n2, init,
                 max_dist, max_iters, rel_fitness, rel_rmse, transform, corr, num_corr, fitness,
                 rmse, iterations, status, stream, RaggedCounts{counts1, counts2});
}
