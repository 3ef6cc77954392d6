// icp.hip -- batched point-to-point ICP for gfx950: the reference's
// register_one_pair(func='icp') (utils/open3d_func.py:63-72, Open3D
// registration_icp on the CPU, one pair at a time), as a solver of its own or
// as the refinement of pcr_rigid_ransac's transform.  The contract is
// DESIGN.md 4.8b, the scalar math include/pcr_rigid.h + pcr_sumsq3f.
//
//   icp_kernel  one workgroup per pair runs the whole iteration loop (bounded
//     by the uniform max_iters, no host round trip).  The target cloud lies in
//     LDS as three planes x / y / z padded with NaN to a multiple of kIPad; it
//     is staged once when it fits one chunk of kIChunk points and re-staged
//     chunk by chunk otherwise.  A thread owns kIP source points per tile of
//     kIT * kIP (point i = tile + k * kIT + tid): it moves them by the current
//     transform and scans the chunk kIPad targets at a time -- their
//     ds_read_b128 (four targets of one plane, the same address in every lane:
//     a broadcast) all issued before the first is scored, then independent
//     distance chains, strict `<` in ascending j, so the lowest index wins a
//     tie and a NaN never wins.  M, E, the centroid sums
//     and the centred cross-covariance are per-thread fp64 sums in ascending
//     point order, a fixed shuffle butterfly, the waves in order (the scheme
//     of rigid_refit_kernel): no float atomics, the same bits every run.
//     Wave 0 solves (pcr_rigid_from_cov) and hands R, t to the others through
//     LDS.  kResident (n1 <= one tile): the source points, their nearest
//     target and its coordinates stay in registers between the evaluation
//     and the covariance pass, and corr is written once at the end; larger
//     n1 keeps the nearest index in corr and re-reads the points.
//     Ragged pairs (the RG pack of common.hpp): the valid
//     lengths v1 / v2 bound the points and the targets, the strides n1 / n2
//     choose the paths.  The thread that owns point i, the order of its sums
//     and the ascending strict-`<` target scan depend on i and j alone, so a
//     pair gives the bits of the dense kernel on the pair trimmed to v1 / v2
//     whichever path either takes.
#include "common.hpp"
#include "icp_scan.hpp"
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
  extern __shared__ __attribute__((aligned(16))) char icp_smem[];
  float* tg = (float*)icp_smem;  // [3][cap]
  double(*red_s)[16] = (double(*)[16])(icp_smem + (size_t)cap * 12);
  double* sol_s = (double*)(red_s + kIW);  // R[9], t[3]
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
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++)
      R[3 * i + j] = init ? init[(size_t)q * 16 + 4 * i + j] : (i == j ? 1.0 : 0.0);
    t[i] = init ? init[(size_t)q * 16 + 4 * i + 3] : 0.0;
  }
  pcr_rigid_round(R, t, T);
  if (whole) {
    icp_stage(tg, cap, B, n2, 0, v2);
    lds_barrier();
  }

  // kResident: the tile's points, their nearest target and its coordinates
  float a[kIP][3], b[kIP][3];
  int bj[kIP];
  double M = 0.0, E = 0.0, pfit = 0.0, prmse = 0.0;
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
      const bool any = s0 + tid < v1;  // k = 0 is the thread's lowest point
      if (whole) {
        if (any) icp_scan(tg, cap, 0, v2, m, bd, bj);
      } else {
        for (int c0 = 0; c0 < v2; c0 += cap) {
          const int len = min(cap, v2 - c0);
          lds_barrier();
          icp_stage(tg, cap, B, n2, c0, len);
          lds_barrier();
          if (any) icp_scan(tg, cap, c0, len, m, bd, bj);
        }
      }
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
    block_sum_d<kIW>(acc, red_s);
    M = acc[0];
    E = acc[1];
    const double fit = M / (double)v1;
    const double rm = M > 0.0 ? __builtin_sqrt(E / M) : 0.0;
    const bool conv = it > 0 && __builtin_fabs(pfit - fit) < rel_fitness &&
                      __builtin_fabs(prmse - rm) < rel_rmse;
    pfit = fit;
    prmse = rm;
    // every exit is uniform: the sums are the same bits in every thread
    if (conv) {
      st = 0;
      break;
    }
    if (it >= max_iters) break;
    if (M < 3.0) {
      st = 1;
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
    block_sum_d<kIW>(cov, red_s);
    if (tid < kWave) {
      pcr_rigid_from_cov(ca, cb, cov, R, t);
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 9; i++) sol_s[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; i++) sol_s[9 + i] = t[i];
      }
    }
    lds_barrier();
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = sol_s[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = sol_s[9 + i];
    pcr_rigid_round(R, t, T);
  }

  if (kResident) {
#pragma unroll
    for (int k = 0; k < kIP; k++) {
      const int i = k * kIT + tid;
      if (i < n1) cq[i] = bj[k];
    }
  }
  if (tid == 0) {
    double* tq = transform + (size_t)q * 16;
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
    num_corr[q] = (int)M;
    fitness[q] = pfit;
    rmse[q] = prmse;
    iterations[q] = it;
    status[q] = st;
  }
}

}  // namespace pcr

using namespace pcr;

// the checks both entry points share
static pcr_status icp_check(int p, int n1, int n2, float max_dist, int max_iters,
                            double rel_fitness, double rel_rmse) {
  PCR_REQUIRE(p >= 0 && n1 >= 1 && n2 >= 1, "icp_point_to_point: invalid sizes");
  PCR_REQUIRE(max_dist > 0.0f, "icp_point_to_point: max_dist must be positive");
  PCR_REQUIRE(max_iters >= 0 && max_iters <= kIcpMaxIters,
              "icp_point_to_point: max_iters (%d) outside [0, %d]", max_iters, kIcpMaxIters);
  PCR_REQUIRE(rel_fitness >= 0.0 && rel_rmse >= 0.0,
              "icp_point_to_point: negative or NaN tolerance");
  return PCR_OK;
}

extern "C" pcr_status pcr_icp_point_to_point(const float* xyz1, const float* xyz2, int p, int n1,
                                             int n2, const double* init, float max_dist,
                                             int max_iters, double rel_fitness, double rel_rmse,
                                             double* transform, int* corr, int* num_corr,
                                             double* fitness, double* rmse, int* iterations,
                                             int* status, void* stream) {
  if (icp_check(p, n1, n2, max_dist, max_iters, rel_fitness, rel_rmse) != PCR_OK)
    return PCR_ERR_INVALID;
  if (p == 0) return PCR_OK;
  PCR_REQUIRE(xyz1 && xyz2 && transform && corr && num_corr && fitness && rmse && iterations &&
                  status,
              "icp_point_to_point: null pointer");
  hipStream_t st = as_stream(stream);
  const int cap = icp_cap(n2);
  const size_t lds = icp_lds_bytes(cap);
  const float tau2 = max_dist * max_dist;
  if (n1 <= kITile) {
    allow_big_lds(icp_kernel<true>, lds);
    hipLaunchKernelGGL(icp_kernel<true>, dim3(p), dim3(kIT), lds, st, xyz1, xyz2, n1, n2, init,
                       tau2, max_iters, rel_fitness, rel_rmse, cap, transform, corr, num_corr,
                       fitness, rmse, iterations, status);
  } else {
    allow_big_lds(icp_kernel<false>, lds);
    hipLaunchKernelGGL(icp_kernel<false>, dim3(p), dim3(kIT), lds, st, xyz1, xyz2, n1, n2, init,
                       tau2, max_iters, rel_fitness, rel_rmse, cap, transform, corr, num_corr,
                       fitness, rmse, iterations, status);
  }
  return launch_status("icp_point_to_point");
}

extern "C" pcr_status pcr_icp_point_to_point_ragged(
    const float* xyz1, const float* xyz2, int p, int n1, int n2, const int* counts1,
    const int* counts2, const double* init, float max_dist, int max_iters, double rel_fitness,
    double rel_rmse, double* transform, int* corr, int* num_corr, double* fitness, double* rmse,
    int* iterations, int* status, void* stream) {
  if (icp_check(p, n1, n2, max_dist, max_iters, rel_fitness, rel_rmse) != PCR_OK)
    return PCR_ERR_INVALID;
  if (p == 0) return PCR_OK;
  PCR_REQUIRE(xyz1 && xyz2 && transform && corr && num_corr && fitness && rmse && iterations &&
                  status,
              "icp_point_to_point_ragged: null pointer");
  hipStream_t st = as_stream(stream);
  // the paths follow the strides; the result does not depend on them
  const int cap = icp_cap(n2);
  const size_t lds = icp_lds_bytes(cap);
  const float tau2 = max_dist * max_dist;
  const RaggedCounts rc = {counts1, counts2};
  if (n1 <= kITile) {
    allow_big_lds(icp_kernel<true, RaggedCounts>, lds);
    hipLaunchKernelGGL((icp_kernel<true, RaggedCounts>), dim3(p), dim3(kIT), lds, st, xyz1, xyz2,
                       n1, n2, init, tau2, max_iters, rel_fitness, rel_rmse, cap, transform, corr,
                       num_corr, fitness, rmse, iterations, status, rc);
  } else {
    allow_big_lds(icp_kernel<false, RaggedCounts>, lds);
    hipLaunchKernelGGL((icp_kernel<false, RaggedCounts>), dim3(p), dim3(kIT), lds, st, xyz1, xyz2,
                       n1, n2, init, tau2, max_iters, rel_fitness, rel_rmse, cap, transform, corr,
                       num_corr, fitness, rmse, iterations, status, rc);
  }
  return launch_status("icp_point_to_point_ragged");
}
