// icp_scan.hpp -- what the ICP kernels (icp.hip point to point, icp_plane.hip
// point to plane) share: the launch shape, the target cloud's LDS planes
// (icp_stage) and the nearest-target scan over them (icp_scan).
#pragma once

#include "common.hpp"
#include "pcr_rigid.h"

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
constexpr int kIcpMaxIters = 100000;  // the cap on max_iters
static_assert(kIT % kWave == 0 && kIT <= 1024 && kIChunk % kIPad == 0, "icp launch shape");

inline int icp_cap(int n2) { return min((n2 + kIPad - 1) / kIPad * kIPad, kIChunk); }
inline size_t icp_lds_bytes(int cap) {
  return (size_t)cap * 12 + (size_t)kIW * 16 * sizeof(double) + 16 * sizeof(double);
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

}  // namespace pcr
