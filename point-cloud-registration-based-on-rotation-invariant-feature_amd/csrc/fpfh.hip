// fpfh.hip -- batched FPFH descriptors (33 channels from points, normals and
// the neighbour lists of pcr_knn_forward) for gfx950: Open3D's
// ComputeFPFHFeature for b clouds at once.  The contract and its scalar math
// are include/pcr_fpfh.h.
//
// Per call, all on the caller's stream, every launch over (tiles of 64
// points, clouds):
//   pack   positions and normals, [3][n] twice -> rows [n][8] (x y z nx ny nz
//          0 0), so that a neighbour is two 16-byte reads
//   spfh   a workgroup takes 64 points; wave w takes the slots w, w + 4, ...
//          of all 64 (the lists are read contiguously in n), a lane computes
//          the pair feature of (point, slot) and counts its three bins in the
//          point's LDS histogram with integer increments, whose order is free.
//          The histograms leave point-major into the workspace, rows of 33
//          floats, so that a neighbour's SPFH is one contiguous read; the
//          optional channel-major copy and nbr_count leave contiguous in n
//   fpfh   a lane per (point, channel), 64 x 33 of them over 256 threads: the
//          neighbour lists of the 64 points are staged in LDS, 32 slots at a
//          time with the slots outside N(i) marked, and every lane adds its
//          channel of the neighbours' rows serially in ascending slot.  The
//          group sums are serial sums over 11 LDS values.  The result leaves
//          through an LDS tile, contiguous in n per channel
// No float atomics, no cross-lane float reduction, no loop that depends on
// the data beyond k, nothing spins, and every output element is written.
#include "common.hpp"
#include "pcr_fpfh.h"

namespace pcr {

constexpr int kFpTile = 64;                  // points per workgroup
constexpr int kFpThreads = 256;
constexpr int kFpCh = PCR_FPFH_CHANNELS;     // 33
constexpr int kFpRow = 8;                    // floats per packed point
constexpr int kFpChunk = 32;                 // slots staged at a time in the fpfh stage
constexpr int kFpTasks = (kFpTile * kFpCh + kFpThreads - 1) / kFpThreads;  // 9 per thread

struct FpWs {
  float* pn;    // [b][n][kFpRow]
  float* rows;  // [b][n][kFpCh] SPFH, point-major
};

static size_t fp_ws_layout(int b, int n, FpWs* ws, void* base) {
  const size_t nk = (size_t)b * n;
  size_t off = 0;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* q = p ? p + off : nullptr;
    off = align_up(off + bytes, 256);
    return q;
  };
  float* pn = (float*)take(nk * kFpRow * 4);
  float* rows = (float*)take(nk * kFpCh * 4);
  if (ws) {
    ws->pn = pn;
    ws->rows = rows;
  }
  return off;
}

__global__ __launch_bounds__(256) void fpfh_pack_kernel(const float* __restrict__ xyz,
                                                        const float* __restrict__ normals, int n,
                                                        float4* __restrict__ pn) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
  if (i >= n) return;
  const float* X = xyz + (size_t)q * 3 * n + i;
  const float* N = normals + (size_t)q * 3 * n + i;
  float4* row = pn + ((size_t)q * n + i) * 2;
  row[0] = make_float4(X[0], X[(size_t)n], X[2 * (size_t)n], N[0]);
  row[1] = make_float4(N[(size_t)n], N[2 * (size_t)n], 0.0f, 0.0f);
}

// the three bins of the pair (point i, neighbour row j) counted in h
__device__ inline void fp_count_pair(const float pi[3], const float ni[3], float4 r0, float4 r1,
                                     int* h) {
  const float pj[3] = {r0.x, r0.y, r0.z}, nj[3] = {r0.w, r1.x, r1.y};
  float f[3];
  int ch[3];
  pcr_fpfh_pair(pi, ni, pj, nj, f);
  pcr_fpfh_bins(f, ch);
  atomicAdd(&h[ch[0]], 1);
  atomicAdd(&h[ch[1]], 1);
  atomicAdd(&h[ch[2]], 1);
}

__global__ __launch_bounds__(kFpThreads) void fpfh_spfh_kernel(
    const float4* __restrict__ pn, const int* __restrict__ nbr_idx,
    const float* __restrict__ nbr_dist, int n, int k, float r2, float* __restrict__ rows,
    float* __restrict__ spfh, int* __restrict__ nbr_count) {
  constexpr int U = 4;  // slots in flight per lane
  __shared__ int hist[kFpTile][kFpCh];
  __shared__ int cnt_s[kFpTile];
  const int q = blockIdx.y, i0 = blockIdx.x * kFpTile, tid = threadIdx.x;
  const int pt = tid & 63, w = tid >> 6, i = i0 + pt;
  const int kk = min(k, n);
  for (int e = tid; e < kFpTile * kFpCh; e += kFpThreads) (&hist[0][0])[e] = 0;
  if (tid < kFpTile) cnt_s[tid] = 0;
  __syncthreads();
  if (i < n) {
    const float4* P = pn + (size_t)q * n * 2;
    const float4 a0 = P[(size_t)i * 2], a1 = P[(size_t)i * 2 + 1];
    const float pi[3] = {a0.x, a0.y, a0.z}, ni[3] = {a0.w, a1.x, a1.y};
    const int* I = nbr_idx + (size_t)q * k * n + i;
    const float* D = nbr_dist + (size_t)q * k * n + i;
    int mine = 0;
    for (int s0 = w; s0 < kk; s0 += 4 * U) {
      int j[U];
      float4 r0[U], r1[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int s = s0 + 4 * u;
        j[u] = -1;
        if (s < kk) {
          const int jj = I[(size_t)s * n];
          if (pcr_fpfh_in_set(jj, D[(size_t)s * n], i, n, r2)) j[u] = jj;
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int src = j[u] >= 0 ? j[u] : i;  // a slot outside N(i) is never an address
        r0[u] = P[(size_t)src * 2];
        r1[u] = P[(size_t)src * 2 + 1];
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (j[u] >= 0) {
          fp_count_pair(pi, ni, r0[u], r1[u], hist[pt]);
          mine++;
        }
      }
    }
    if (mine) atomicAdd(&cnt_s[pt], mine);
  }
  __syncthreads();
  // point-major rows: the tile's 64 x 33 values are consecutive in the workspace
  const int npt = min(kFpTile, n - i0);
  float* R = rows + ((size_t)q * n + i0) * kFpCh;
  for (int e = tid; e < npt * kFpCh; e += kFpThreads) {
    const int p = e / kFpCh, c = e - p * kFpCh;
    R[e] = pcr_fpfh_spfh(hist[p][c], cnt_s[p]);
  }
  if (i < n) {
    if (spfh)
      for (int c = w; c < kFpCh; c += 4)
        spfh[((size_t)q * kFpCh + c) * n + i] = pcr_fpfh_spfh(hist[pt][c], cnt_s[pt]);
    if (nbr_count && w == 0) nbr_count[(size_t)q * n + i] = cnt_s[pt];
  }
}

__global__ __launch_bounds__(kFpThreads) void fpfh_fpfh_kernel(
    const float* __restrict__ rows, const int* __restrict__ nbr_idx,
    const float* __restrict__ nbr_dist, int n, int k, float r2, float* __restrict__ fpfh) {
  constexpr int U = 8;  // rows in flight per lane
  __shared__ int j_s[kFpChunk][kFpTile];
  __shared__ float d_s[kFpChunk][kFpTile];
  __shared__ float acc_s[kFpTile][kFpCh];
  __shared__ float out_s[kFpCh][kFpTile + 1];
  const int q = blockIdx.y, i0 = blockIdx.x * kFpTile, tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int kk = min(k, n), npt = min(kFpTile, n - i0);
  const float* R = rows + (size_t)q * n * kFpCh;
  const int* I = nbr_idx + (size_t)q * k * n;
  const float* D = nbr_dist + (size_t)q * k * n;
  float acc[kFpTasks];
#pragma unroll
  for (int t = 0; t < kFpTasks; t++) acc[t] = 0.0f;
  for (int c0 = 0; c0 < kk; c0 += kFpChunk) {
    const int ns = min(kFpChunk, kk - c0);
    __syncthreads();  // the previous chunk has been consumed
    // the chunk's lists, contiguous in n; slots outside N(i) become j = -1
    for (int s = w; s < ns; s += 4) {
      int jj = -1;
      float dd = 1.0f;
      if (lane < npt) {
        const int i = i0 + lane;
        const int jr = I[(size_t)(c0 + s) * n + i];
        const float dr = D[(size_t)(c0 + s) * n + i];
        if (pcr_fpfh_in_set(jr, dr, i, n, r2)) {
          jj = jr;
          dd = dr;
        }
      }
      j_s[s][lane] = jj;
      d_s[s][lane] = dd;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kFpTasks; t++) {
      const int e = t * kFpThreads + tid;
      const int p = e / kFpCh, c = e - p * kFpCh;
      if (p < npt) {
        float a = acc[t];
        for (int s0 = 0; s0 < ns; s0 += U) {
          int j[U];
          float x[U];
#pragma unroll
          for (int u = 0; u < U; u++) j[u] = s0 + u < ns ? j_s[s0 + u][p] : -1;
#pragma unroll
          for (int u = 0; u < U; u++)
            x[u] = R[(size_t)(j[u] >= 0 ? j[u] : i0 + p) * kFpCh + c];
#pragma unroll
          for (int u = 0; u < U; u++)
            if (j[u] >= 0) a = pcr_fpfh_add(a, x[u], d_s[s0 + u][p]);
        }
        acc[t] = a;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kFpTasks; t++) {
    const int e = t * kFpThreads + tid;
    if (e < kFpTile * kFpCh) (&acc_s[0][0])[e] = acc[t];
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kFpTasks; t++) {
    const int e = t * kFpThreads + tid;
    const int p = e / kFpCh, c = e - p * kFpCh;
    if (p < npt) {
      const int g = c / PCR_FPFH_BINS;
      const float sg = pcr_fpfh_group_sum(&acc_s[p][g * PCR_FPFH_BINS]);
      out_s[c][p] = pcr_fpfh_value(acc[t], sg, R[(size_t)(i0 + p) * kFpCh + c]);
    }
  }
  __syncthreads();
  if (lane < npt)
    for (int c = w; c < kFpCh; c += 4)
      fpfh[((size_t)q * kFpCh + c) * n + i0 + lane] = out_s[c][lane];
}

}  // namespace pcr

using namespace pcr;

extern "C" size_t pcr_fpfh_workspace_size(int b, int n) {
  if (b <= 0 || n <= 0) return 256;
  return fp_ws_layout(b, n, nullptr, nullptr);
}

extern "C" pcr_status pcr_fpfh(const float* xyz, const float* normals, const int* nbr_idx,
                               const float* nbr_dist, int b, int n, int k, float radius,
                               float* fpfh, float* spfh, int* nbr_count, void* workspace,
                               size_t workspace_bytes, void* stream) {
  PCR_REQUIRE(b >= 0, "fpfh: negative batch size");
  PCR_REQUIRE(n >= 1, "fpfh: n must be at least 1");
  PCR_REQUIRE(k >= 1 && k <= PCR_FPFH_MAX_K, "fpfh: k must be in [1, %d] (got %d)",
              PCR_FPFH_MAX_K, k);
  PCR_REQUIRE(radius > 0.0f && radius - radius == 0.0f, "fpfh: radius must be finite and > 0");
  if (b == 0) return PCR_OK;
  PCR_REQUIRE((int64_t)b * k * n < (1ll << 31) && b <= 65535, "fpfh: batch too large");
  PCR_REQUIRE(xyz && normals && nbr_idx && nbr_dist && fpfh, "fpfh: null pointer");
  FpWs ws;
  const size_t need = fp_ws_layout(b, n, &ws, workspace);
  PCR_REQUIRE(workspace != nullptr && workspace_bytes >= need,
              "fpfh: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const float r2 = radius * radius;
  const dim3 tiles(ceil_div(n, kFpTile), b);
  hipLaunchKernelGGL(fpfh_pack_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, xyz, normals,
                     n, (float4*)ws.pn);
  hipLaunchKernelGGL(fpfh_spfh_kernel, tiles, dim3(kFpThreads), 0, st, (const float4*)ws.pn,
                     nbr_idx, nbr_dist, n, k, r2, ws.rows, spfh, nbr_count);
  hipLaunchKernelGGL(fpfh_fpfh_kernel, tiles, dim3(kFpThreads), 0, st, ws.rows, nbr_idx, nbr_dist,
                     n, k, r2, fpfh);
  return launch_status("fpfh");
}
