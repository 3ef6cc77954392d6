// normals_nbr.hip -- point normals from ready neighbour lists, for gfx950:
// Open3D's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) with the
// search taken out.  The lists are pcr_hybrid_search's (hybrid_search.hip),
// slot-major [b, k, n] with the point itself in its own row; this op is the
// PCA over each row, the way pcr_fpfh consumes lists without searching
// (DESIGN.md 4.8h).  The per-point arithmetic is pcr_estimate_normal of
// include/pcr_math.h, the one normals.hip ends in.
//
// Layout: one lane per point.  Slot s of 64 consecutive points is 256
// consecutive bytes of nbr_idx, so the index reads are coalesced; the
// neighbour's coordinates are three 4-byte gathers out of L2 (a cloud is
// 12 n bytes).  kNbU slots are in flight at a time: their index loads, then
// their gathers, are all issued before the first cumulant is touched, and the
// cumulants then take them in ascending slot, so the nine fp64 sums are the
// ordered sums the contract names.  A slot outside [0, n) is skipped and is
// never used as an address.
#include "common.hpp"

namespace pcr {
namespace {

constexpr int kNbThreads = 256;
constexpr int kNbU = 4;  // slots in flight

__global__ __launch_bounds__(kNbThreads) void normals_nbr_kernel(
    const float* __restrict__ xyz, const int* __restrict__ nbr_idx, int n, int k, int blocks_n,
    float* __restrict__ normals, int* __restrict__ nbr_count) {
  const int b = blockIdx.x / blocks_n;
  const int i = (blockIdx.x - b * blocks_n) * kNbThreads + threadIdx.x;
  if (i >= n) return;
  const float* P = xyz + (size_t)b * 3 * n;
  const int* I = nbr_idx + (size_t)b * k * n + i;
  double cum[9];
#pragma unroll
  for (int a = 0; a < 9; a++) cum[a] = 0.0;
  int cnt = 0;
  for (int s0 = 0; s0 < k; s0 += kNbU) {
    int j[kNbU];
    float v[kNbU][3];
#pragma unroll
    for (int u = 0; u < kNbU; u++) j[u] = s0 + u < k ? I[(size_t)(s0 + u) * n] : -1;
#pragma unroll
    for (int u = 0; u < kNbU; u++) {
      const bool ok = j[u] >= 0 && j[u] < n;
#pragma unroll
      for (int d = 0; d < 3; d++) v[u][d] = ok ? P[(size_t)d * n + j[u]] : 0.0f;
      if (!ok) j[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < kNbU; u++) {
      if (j[u] >= 0) {
        const double x = v[u][0], y = v[u][1], z = v[u][2];
        cum[0] += x;
        cum[1] += y;
        cum[2] += z;
        cum[3] += x * x;
        cum[4] += x * y;
        cum[5] += x * z;
        cum[6] += y * y;
        cum[7] += y * z;
        cum[8] += z * z;
        cnt++;
      }
    }
  }
  float nv[3];
  pcr_estimate_normal(cum, cnt, P[i], P[(size_t)n + i], P[(size_t)2 * n + i], nv);
  float* N = normals + (size_t)b * 3 * n;
  N[i] = nv[0];
  N[(size_t)n + i] = nv[1];
  N[(size_t)2 * n + i] = nv[2];
  if (nbr_count) nbr_count[(size_t)b * n + i] = cnt;
}

}  // namespace
}  // namespace pcr

using namespace pcr;

extern "C" pcr_status pcr_normals_from_neighbors(const float* xyz, const int* nbr_idx, int b, int n,
                                                 int k, float* normals, int* nbr_count,
                                                 void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 1, "normals_from_neighbors: invalid sizes b=%d n=%d", b, n);
  PCR_REQUIRE(k >= 1 && k <= 128, "normals_from_neighbors: k (%d) outside [1, 128]", k);
  PCR_REQUIRE((long long)b * k * n < (1ll << 31), "normals_from_neighbors: b * k * n passes 2^31");
  if (b == 0) return PCR_OK;
  PCR_REQUIRE(xyz && nbr_idx && normals, "normals_from_neighbors: null pointer");
  const int blocks_n = ceil_div(n, kNbThreads);
  hipLaunchKernelGGL(normals_nbr_kernel, dim3((unsigned)b * blocks_n), dim3(kNbThreads), 0,
                     as_stream(stream), xyz, nbr_idx, n, k, blocks_n, normals, nbr_count);
  return launch_status("normals_from_neighbors");
}
