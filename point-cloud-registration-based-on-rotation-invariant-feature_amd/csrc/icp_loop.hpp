// icp_loop.hpp -- the iteration loop the ICP kernels (icp.hip point to point,
// icp_plane.hip point to plane) share, and its host plumbing.  A kernel keeps
// its own estimation step; everything around it stands here once.
//
// The shared contract:
//   One workgroup per pair runs the whole loop (bounded by the uniform
//   max_iters, no host round trip).  The target cloud lies in LDS as three
//   planes x / y / z padded with NaN to a multiple of kIPad; it is staged once
//   when it fits one chunk of kIChunk points and re-staged chunk by chunk
//   otherwise.  A thread owns kIP source points per tile of kIT * kIP (point
//   i = tile + k * kIT + tid): it moves them by the current transform and
//   scans the chunk kIPad targets at a time -- their ds_read_b128 (four
//   targets of one plane, the same address in every lane: a broadcast) all
//   issued before the first is scored, then independent distance chains,
//   strict `<` in ascending j, so the lowest index wins a tie and a NaN never
//   wins.  The sums are per-thread fp64 sums in ascending point order, a
//   fixed shuffle butterfly, the waves in order (block_sum_d): no float
//   atomics, the same bits every run and in every thread, so every exit is
//   uniform.  Wave 0 solves and hands R, t to the others through LDS.
//   Ragged pairs: the valid lengths v1 / v2 bound the points
//   and the targets, the strides n1 / n2 choose the paths.  The thread that
//   owns point i, the order of its sums and the ascending strict-`<` target
//   scan depend on i and j alone, so a pair gives the bits of the dense call
//   on the pair trimmed to v1 / v2 whichever path either takes.
#pragma once

#include "common.hpp"
#include "pcr_rigid.h"
#include "rigid_pair.hpp"

// launch shape; other shapes for A/B builds (make ab DEFS=-DPCR_ICP_THREADS=256
// -DPCR_ICP_PPT=4)
#ifndef PCR_ICP_THREADS
#define PCR_ICP_THREADS 512
#endif
#ifndef PCR_ICP_PPT
#define PCR_ICP_PPT 2
#endif

namespace pcr {

constexpr int kIT = PCR_ICP_THREADS;  // threads per workgroup
constexpr int kIP = PCR_ICP_PPT;      // source points per thread and tile
constexpr int kIW = kIT / kWave;
constexpr int kITile = kIT * kIP;
constexpr int kIChunk = 8192;         // target points per LDS chunk (12 bytes each: 96 KB)
constexpr int kIPad = 16;             // targets per scan step; the planes are NaN-padded to it
constexpr int kISol = 16;             // doubles of the hand-off: R[9], t[3], the solver's flag
constexpr int kIcpMaxIters = 100000;  // the cap on max_iters
static_assert(kIT % kWave == 0 && kIT <= 1024 && kIChunk % kIPad == 0, "icp launch shape");

// The dynamic LDS of an ICP kernel: the target planes, block_sum_d's rows and
// wave 0's hand-off, in that order.
struct IcpLds {
  float* tg;           // [3][cap]
  double (*red_s)[16];  // [kIW]
  double* sol_s;        // [kISol]
};
inline int icp_cap(int n2) { return min((n2 + kIPad - 1) / kIPad * kIPad, kIChunk); }
inline size_t icp_lds_bytes(int cap) {
  return (size_t)cap * 12 + (size_t)kIW * 16 * sizeof(double) + kISol * sizeof(double);
}
__device__ inline IcpLds icp_lds(int cap) {
  extern __shared__ __attribute__((aligned(16))) char icp_smem[];
  IcpLds l;
  l.tg = (float*)icp_smem;
  l.red_s = (double(*)[16])(icp_smem + (size_t)cap * 12);
  l.sol_s = (double*)(l.red_s + kIW);
  return l;
}

// the start transform: pair q's init rows, or the identity
__device__ inline void icp_start(const double* __restrict__ init, int q, double (&R)[9],
                                 double (&t)[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++)
      R[3 * i + j] = init ? init[(size_t)q * 16 + 4 * i + j] : (i == j ? 1.0 : 0.0);
    t[i] = init ? init[(size_t)q * 16 + 4 * i + 3] : 0.0;
  }
}

// targets [c0, c0 + len) of the pair -> the three LDS planes, NaN up to the
// next multiple of kIPad (len <= cap, cap % kIPad == 0)
__device__ inline void icp_stage(float* tg, int cap, const float* __restrict__ B, int n2, int c0,
                                 int len) {
  const int lenp = (len + kIPad - 1) & ~(kIPad - 1);
  for (int j = threadIdx.x; j < lenp; j += kIT) {
#pragma unroll
    for (int d = 0; d < 3; d++)
      tg[d * cap + j] = j < len ? B[(size_t)d * n2 + c0 + j] : __builtin_nanf("");
  }
}

// nearest of the staged targets to each of the thread's moved points
__device__ inline void icp_scan(const float* tg, int cap, int c0, int len,
                                const float (&m)[kIP][3], float (&bd)[kIP], int (&bj)[kIP]) {
  const int lenp = (len + kIPad - 1) & ~(kIPad - 1);
  for (int j0 = 0; j0 < lenp; j0 += kIPad) {
    // kIPad / 4 groups of three reads in flight before the first is scored
#pragma unroll
    for (int g = 0; g < kIPad / 4; g++) {
      const int j = j0 + 4 * g;
      const float4 x = *(const float4*)(tg + j);
      const float4 y = *(const float4*)(tg + cap + j);
      const float4 z = *(const float4*)(tg + 2 * cap + j);
      const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w},
                  zs[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
      for (int u = 0; u < 4; u++) {
#pragma unroll
        for (int k = 0; k < kIP; k++) {
          const float d = pcr_sumsq3f(m[k][0] - xs[u], m[k][1] - ys[u], m[k][2] - zs[u]);
          if (d < bd[k]) {
            bd[k] = d;
            bj[k] = c0 + j + u;
          }
        }
      }
    }
  }
}

// Nearest of the pair's v2 targets to each of the thread's moved points: the
// staged cloud when `whole`, otherwise staged and scanned chunk by chunk (the
// barriers are the workgroup's: every thread calls, `any` says whether this
// one has a point in the tile).
__device__ inline void icp_nearest(float* tg, int cap, bool whole, const float* __restrict__ B,
                                   int n2, int v2, bool any, const float (&m)[kIP][3],
                                   float (&bd)[kIP], int (&bj)[kIP]) {
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
}

// The verdict on evaluation `it` from its block sums M (correspondences) and E
// (their squared distances): fitness and RMSE into pfit / prmse, then the
// status the loop ends with -- 0 converged, 2 the iteration limit, 1 fewer
// than kMinCorr correspondences, in that order -- or -1 to take a step.
template <int kMinCorr>
__device__ inline int icp_verdict(double M, double E, int v1, int it, int max_iters,
                                  double rel_fitness, double rel_rmse, double& pfit,
                                  double& prmse) {
  const double fit = M / (double)v1;
  const double rm = M > 0.0 ? __builtin_sqrt(E / M) : 0.0;
  const bool conv = it > 0 && __builtin_fabs(pfit - fit) < rel_fitness &&
                    __builtin_fabs(prmse - rm) < rel_rmse;
  pfit = fit;
  prmse = rm;
  if (conv) return 0;
  if (it >= max_iters) return 2;
  if (M < (double)kMinCorr) return 1;
  return -1;
}

// Wave 0's hand-off: after its solve, thread 0 publishes R, t (with kFlag also
// the solver's flag); past an lds_barrier every thread fetches them (and gets
// the flag).  The solve and the publish stay inside the kernel's wave-0
// branch, so that R, t of the other waves are dead until the fetch.
template <bool kFlag = false>
__device__ inline void icp_publish(double* sol_s, const double (&R)[9], const double (&t)[3],
                                   int flag = 0) {
#pragma unroll
  for (int i = 0; i < 9; i++) sol_s[i] = R[i];
#pragma unroll
  for (int i = 0; i < 3; i++) sol_s[9 + i] = t[i];
  if (kFlag) sol_s[12] = flag ? 1.0 : 0.0;
}
template <bool kFlag = false>
__device__ inline bool icp_fetch(const double* sol_s, double (&R)[9], double (&t)[3]) {
  const bool flag = kFlag && sol_s[12] != 0.0;
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = sol_s[i];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = sol_s[9 + i];
  return flag;
}

// pair q's transform and its five results (one thread)
__device__ inline void icp_store(int q, const double (&R)[9], const double (&t)[3], double M,
                                 double pfit, double prmse, int it, int st, double* transform,
                                 int* num_corr, double* fitness, double* rmse, int* iterations,
                                 int* status) {
  rigid_store_transform(transform + (size_t)q * 16, R, t);
  num_corr[q] = (int)M;
  fitness[q] = pfit;
  rmse[q] = prmse;
  iterations[q] = it;
  status[q] = st;
}

// ---- host side

// the range checks of every ICP entry point, under its name
inline pcr_status icp_check(const char* name, int p, int n1, int n2, float max_dist, int max_iters,
                            double rel_fitness, double rel_rmse) {
  PCR_REQUIRE(p >= 0 && n1 >= 1 && n2 >= 1, "%s: invalid sizes", name);
  PCR_REQUIRE(max_dist > 0.0f, "%s: max_dist must be positive", name);
  PCR_REQUIRE(max_iters >= 0 && max_iters <= kIcpMaxIters, "%s: max_iters (%d) outside [0, %d]",
              name, max_iters, kIcpMaxIters);
  PCR_REQUIRE(rel_fitness >= 0.0 && rel_rmse >= 0.0, "%s: negative or NaN tolerance", name);
  return PCR_OK;
}

// one workgroup per pair of `kernel(xyz1, xyz2, args...)`, with the LDS its
// target chunk needs
template <typename K, typename... Args>
inline void icp_launch(K kernel, int p, int n2, void* stream, Args... args) {
  const size_t lds = icp_lds_bytes(icp_cap(n2));
  allow_big_lds(kernel, lds);
  hipLaunchKernelGGL(kernel, dim3(p), dim3(kIT), lds, as_stream(stream), args...);
}

}  // namespace pcr
