// voxelize_big.hip -- average voxelization (spherical / cube) of clouds of
// more than 4096 points, and their coordinate normalisation, for gfx950;
// voxelize.hip's entry points call it past kMaxSortN points.
//
// A stable counting sort by voxel, hand-written, at any size: (1) per-point
// voxel index and count atomics, whose return value is the point's arrival
// slot in its voxel; (2) a per-cloud exclusive scan of the counts (tile sums,
// then each tile scans itself after the sum of the tiles before it) locates
// every voxel's segment; (3) each point lands at start + slot (arrival
// order); (4) each point of a segment of 1 < m <= 64 takes its rank by point
// id among the segment (m reads), a larger segment is sorted by a stable
// workgroup radix sort, so every voxel's points end up in ascending point
// order -- the order the oracle sums in; (5) one thread per voxel sums
// its segment in that order and writes all C channels, so the dense grid is
// written once, coalesced, zeros included.  The reference scatters C fp32
// atomics per point (spherical_vox.cu:103-123, one cache line each).
#include "voxelize.hpp"

namespace pcr {

struct BigVoxWs {
  int* slot;      // [b][n] arrival slot of each point in its voxel
  int* perm_u;    // [b][n] points by voxel, arrival order within a voxel
  int* perm;      // [b][n] points by voxel, ascending within a voxel
  int* start;     // [b][r3] segment start of each voxel (relative to its cloud)
  int* tsum;      // [b][ntile] counts per scan tile
  int* big;       // [1 + b n / (kRankScan + 1)]: count, then voxels of > kRankScan points
  float* featT;   // [b][n][c] point-major copy of the features (nullptr: c == 0)
  int ntile;
};

// segments of up to this many points take their rank by a scan of the
// segment (m reads per point); larger ones are sorted by vox_seg_sort_kernel
constexpr int kRankScan = 64;

constexpr int kBigScanThreads = 256;
constexpr int kBigScanPer = 16;
constexpr int kBigScanTile = kBigScanThreads * kBigScanPer;

static size_t big_ws_layout(int b, int n, int r, BigVoxWs* ws, void* base, int c = 0) {
  const int64_t r3 = (int64_t)r * r * r;
  const size_t nk = (size_t)b * n, nr = (size_t)b * r3;
  const int ntile = (int)((r3 + kBigScanTile - 1) / kBigScanTile);
  size_t off = 0;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* q = p ? p + off : nullptr;
    off = align_up(off + bytes, 256);
    return q;
  };
  int* slot = (int*)take(nk * 4);
  int* perm_u = (int*)take(nk * 4);
  int* perm = (int*)take(nk * 4);
  int* start = (int*)take(nr * 4);
  int* tsum = (int*)take((size_t)b * ntile * 4);
  int* big = (int*)take((1 + nk / (kRankScan + 1)) * 4);
  float* ft = c > 0 ? (float*)take(nk * (size_t)c * 4) : nullptr;
  if (ws) {
    ws->slot = slot;
    ws->perm_u = perm_u;
    ws->perm = perm;
    ws->start = start;
    ws->tsum = tsum;
    ws->big = big;
    ws->featT = ft;
    ws->ntile = ntile;
  }
  return off;
}

template <int MODE>
__global__ __launch_bounds__(256) void vox_key_big_kernel(const float* __restrict__ coords_f,
                                                          const int* __restrict__ coords_i, int n,
                                                          int r, int* __restrict__ ind,
                                                          int* __restrict__ cnt,
                                                          int* __restrict__ slot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= n) return;
  const int r3 = r * r * r;
  int v;
  bool valid;
  if (MODE == kCube) {
    const int* x = coords_i + (size_t)b * 3 * n;
    v = x[i] * r * r + x[i + n] * r + x[i + 2 * n];
    valid = v >= 0 && v < r3;
  } else {
    const float* x = coords_f + (size_t)b * 3 * n;
    v = pcr_sph_index(x[i], x[i + n], x[i + 2 * n], r);
    valid = v >= 0;
  }
  ind[(size_t)b * n + i] = v;
  slot[(size_t)b * n + i] = valid ? atomicAdd(&cnt[(size_t)b * r3 + v], 1) : -1;
}

// per-cloud exclusive scan of the voxel counts, pass 1: each tile's total
__global__ __launch_bounds__(kBigScanThreads) void vox_scan_tiles_kernel(
    const int* __restrict__ cnt, int r3, int ntile, int* __restrict__ tsum) {
  __shared__ int red[kBigScanThreads / kWave];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int* C = cnt + (size_t)b * r3 + (size_t)t * kBigScanTile;
  const int lim = min(kBigScanTile, r3 - t * kBigScanTile);
  int s = 0;
#pragma unroll
  for (int e = 0; e < kBigScanPer; e++) {
    const int v = e * kBigScanThreads + tid;
    s += v < lim ? C[v] : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < kBigScanThreads / kWave; w++) tot += red[w];
    tsum[(size_t)b * ntile + t] = tot;
  }
}

// pass 2: each tile adds the totals of the tiles before it (in order) and
// scans its counts; thread t owns kBigScanPer consecutive voxels
__global__ __launch_bounds__(kBigScanThreads) void vox_scan_apply_kernel(
    const int* __restrict__ cnt, int r3, int ntile, const int* __restrict__ tsum,
    int* __restrict__ start) {
  __shared__ int scan_s[kBigScanThreads / kWave + 1];
  __shared__ int base_s;
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (tid < 64) {
    int s = 0;
    for (int q = tid; q < t; q += 64) s += tsum[(size_t)b * ntile + q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
    if (tid == 0) base_s = s;
  }
  const int v0 = t * kBigScanTile + tid * kBigScanPer;
  const int* C = cnt + (size_t)b * r3;
  int c[kBigScanPer], sum = 0;
#pragma unroll
  for (int e = 0; e < kBigScanPer; e++) {
    c[e] = v0 + e < r3 ? C[v0 + e] : 0;
    sum += c[e];
  }
  const int incl = block_inclusive_scan(sum, scan_s);  // its barriers also publish base_s
  int run = base_s + incl - sum;
  int* S = start + (size_t)b * r3;
#pragma unroll
  for (int e = 0; e < kBigScanPer; e++) {
    if (v0 + e < r3) S[v0 + e] = run;
    run += c[e];
  }
}

// every point at its voxel's start + arrival slot
__global__ __launch_bounds__(256) void vox_place_big_kernel(const int* __restrict__ ind,
                                                            const int* __restrict__ slot, int n,
                                                            int r3, const int* __restrict__ start,
                                                            int* __restrict__ perm_u) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= n) return;
  const int sl = slot[(size_t)b * n + i];
  if (sl < 0) return;
  const int v = ind[(size_t)b * n + i];
  perm_u[(size_t)b * n + start[(size_t)b * r3 + v] + sl] = i;
}

// every point's final place: its rank by point id within its voxel's segment
// (m reads for a voxel of m <= kRankScan points; one-point voxels copy).  A
// larger segment (duplicated points, a cloud padded by repeating a point) is
// listed once, by its first arrival, for vox_seg_sort_kernel: the scan would
// cost m^2 reads there.
__global__ __launch_bounds__(256) void vox_rank_big_kernel(const int* __restrict__ ind,
                                                           const int* __restrict__ slot, int n,
                                                           int r3, const int* __restrict__ cnt,
                                                           const int* __restrict__ start,
                                                           const int* __restrict__ perm_u,
                                                           int* __restrict__ perm,
                                                           int* __restrict__ big) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= n) return;
  const int sl = slot[(size_t)b * n + i];
  if (sl < 0) return;
  const int v = ind[(size_t)b * n + i];
  const size_t vi = (size_t)b * r3 + v;
  const int m = cnt[vi];
  if (m > kRankScan) {
    if (sl == 0) big[1 + atomicAdd(&big[0], 1)] = (int)vi;
    return;
  }
  const int* seg = perm_u + (size_t)b * n + start[vi];
  int rank = 0;
  for (int x = 0; x < m; x++) rank += seg[x] < i ? 1 : 0;
  perm[(size_t)b * n + start[vi] + rank] = i;
}

// the listed large segments: one workgroup per segment (grid-stride over the
// list), its point ids sorted ascending by a stable workgroup radix sort
// (O(m) per 8-bit pass) from the arrival order (perm_u) into perm
constexpr int kSegSortThreads = 1024;
__global__ __launch_bounds__(kSegSortThreads) void vox_seg_sort_kernel(
    const int* __restrict__ big, const int* __restrict__ cnt, const int* __restrict__ start,
    int n, int r3, int kbits, int* __restrict__ perm_u, int* __restrict__ perm) {
  __shared__ int rs_lds[(2 + kSegSortThreads / kWave) * 256];
  const int nb = big[0];
  for (int e = blockIdx.x; e < nb; e += gridDim.x) {
    const int vi = big[1 + e];
    const int m = cnt[vi];
    const size_t off = (size_t)(vi / r3) * n + start[vi];
    int* res = wg_radix_sort<kSegSortThreads>(perm_u + off, perm + off, m, kbits,
                                              [](int v) { return v; }, rs_lds);
    if (res != perm + off)
      for (int t = threadIdx.x; t < m; t += kSegSortThreads) perm[off + t] = res[t];
    __syncthreads();
  }
}

// the listed large segments' means: one workgroup per segment (grid-stride
// over the list), a thread per channel summing the segment's points in
// ascending order (the order of the thread-per-voxel kernels, which skip
// these voxels), eight point ids and their values loaded ahead of the sums.
// FT: point-major features [b][n][c] (else channel-major [b][c][n]).
template <bool FT>
__global__ __launch_bounds__(256) void vox_seg_gather_kernel(
    const int* __restrict__ big, const float* __restrict__ feat, const int* __restrict__ cnt,
    const int* __restrict__ start, const int* __restrict__ perm, int c, int n, int r3,
    float* __restrict__ out) {
  constexpr int kB = 8;
  const int nb = big[0];
  for (int e = blockIdx.x; e < nb; e += gridDim.x) {
    const int vi = big[1 + e];
    const int b = vi / r3, v = vi - b * r3;
    const int m = cnt[vi];
    const int* P = perm + (size_t)b * n + start[vi];
    const float inv = pcr_inv_count(m);
    for (int ch = threadIdx.x; ch < c; ch += blockDim.x) {
      auto val = [&](int i) {
        return FT ? feat[((size_t)b * n + i) * c + ch] : feat[((size_t)b * c + ch) * n + i];
      };
      float acc = 0.0f;
      int s = 0;
      for (; s + kB <= m; s += kB) {
        int pi[kB];
        float x[kB];
#pragma unroll
        for (int u = 0; u < kB; u++) pi[u] = P[s + u];
#pragma unroll
        for (int u = 0; u < kB; u++) x[u] = val(pi[u]);
#pragma unroll
        for (int u = 0; u < kB; u++) acc += x[u] * inv;
      }
      for (; s < m; s++) acc += val(P[s]) * inv;
      __builtin_nontemporal_store(acc, &out[((size_t)b * c + ch) * r3 + v]);
    }
  }
}

// one thread per voxel: its segment of the sorted points, summed per channel
// in ascending point order (acc += f * inv, the product rounded first)
__global__ __launch_bounds__(256) void vox_gather_big_kernel(
    const float* __restrict__ feat, const int* __restrict__ cnt, const int* __restrict__ start,
    const int* __restrict__ perm, int c, int n, int r3, float* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (v >= r3) return;
  const size_t vi = (size_t)b * r3 + v;
  const int m = cnt[vi];
  if (m > kRankScan) return;  // vox_seg_gather_kernel
  const int* P = perm + (size_t)b * n + start[vi];
  const float* F = feat + (size_t)b * c * n;
  float* O = out + (size_t)b * c * r3 + v;
  if (m == 0) {
    for (int ch = 0; ch < c; ch++) O[(size_t)ch * r3] = 0.0f;
    return;
  }
  const float inv = pcr_inv_count(m);
  constexpr int kHold = 8;
  int pts[kHold];
#pragma unroll
  for (int s = 0; s < kHold; s++) pts[s] = s < m ? P[s] : 0;
  for (int ch = 0; ch < c; ch++) {
    const float* f = F + (size_t)ch * n;
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < kHold; s++)
      if (s < m) acc += f[pts[s]] * inv;
    for (int s = kHold; s < m; s++) acc += f[P[s]] * inv;
    O[(size_t)ch * r3] = acc;
  }
}

// Fixed-order normalisation for any n (same order as cloud_mean: thread t
// sums points t, t + 1024, ... ascending in double; wave halving trees).
__global__ __launch_bounds__(kPrepThreads) void sph_normalize_big_kernel(
    const float* __restrict__ coords, int n, float* __restrict__ out) {
  __shared__ double red[48];
  __shared__ float s_stat[4];
  __shared__ float wm[kPrepThreads / kWave];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* x = coords + (size_t)b * 3 * n;
  float* o = out + (size_t)b * 3 * n;
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += kPrepThreads) {
    s[0] += (double)x[i];
    s[1] += (double)x[i + n];
    s[2] += (double)x[i + 2 * n];
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double v = __shfl_down(s[a], off, kWave);
      if (lane < off) s[a] += v;
    }
    if (lane == 0) red[a * 16 + w] = s[a];
  }
  __syncthreads();
  if (tid < 3) {
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = red[tid * 16 + i];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
#pragma unroll
      for (int i = 0; i < off; i++) v[i] += v[i + off];
    s_stat[tid] = (float)(v[0] / (double)n);
  }
  __syncthreads();
  const float m0 = s_stat[0], m1 = s_stat[1], m2 = s_stat[2];
  float mx = 0.0f;
  for (int i = tid; i < n; i += kPrepThreads)
    mx = fmaxf(mx, __builtin_sqrtf(pcr_sumsq3f(x[i] - m0, x[i + n] - m1, x[i + 2 * n] - m2)));
  mx = wave_max(mx);
  if (lane == 0) wm[w] = mx;
  __syncthreads();
  if (tid == 0) {
    float m = 0.0f;
    for (int k = 0; k < kPrepThreads / kWave; k++) m = fmaxf(m, wm[k]);
    s_stat[3] = m + 1e-20f;
  }
  __syncthreads();
  const float den = s_stat[3];
  for (int i = tid; i < n; i += kPrepThreads) {
    o[i] = (x[i] - m0) / den;
    o[i + n] = (x[i + n] - m1) / den;
    o[i + 2 * n] = (x[i + 2 * n] - m2) / den;
  }
}

// [c][n] -> [n][c] per cloud through a 64 x 64 LDS tile (coalesced both ways)
__global__ __launch_bounds__(256) void feat_transpose_kernel(const float* __restrict__ feat,
                                                             int c, int n,
                                                             float* __restrict__ featT) {
  __shared__ float t[64][65];
  const int b = blockIdx.z, n0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const float* F = feat + (size_t)b * c * n;
  float* T = featT + (size_t)b * n * c;
  for (int y = ty; y < 64; y += 4)
    if (c0 + y < c && n0 + tx < n) t[y][tx] = F[(size_t)(c0 + y) * n + n0 + tx];
  __syncthreads();
  for (int y = ty; y < 64; y += 4)
    if (n0 + y < n && c0 + tx < c) T[(size_t)(n0 + y) * c + c0 + tx] = t[tx][y];
}

// vox_gather_big_kernel on the point-major copy: a voxel's point reads 16
// consecutive channels (64 B) at a time instead of 16 scattered lines
template <int CH>
__global__ __launch_bounds__(256) void vox_gather_big_t_kernel(
    const float* __restrict__ featT, const int* __restrict__ cnt, const int* __restrict__ start,
    const int* __restrict__ perm, int c, int n, int r3, float* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (v >= r3) return;
  const size_t vi = (size_t)b * r3 + v;
  const int m = cnt[vi];
  if (m > kRankScan) return;  // vox_seg_gather_kernel
  float* O = out + (size_t)b * c * r3 + v;
  const int* P = perm + (size_t)b * n + (m > 0 ? start[vi] : 0);
  const float* FT = featT + (size_t)b * n * c;
  const float inv = m > 0 ? pcr_inv_count(m) : 0.0f;
  constexpr int kHold = 4;  // the first points' rows, read once for every chunk
  const float* rows[kHold];
#pragma unroll
  for (int s = 0; s < kHold; s++) rows[s] = s < m ? FT + (size_t)P[s] * c : FT;
  const bool vec = (c & 3) == 0;
  // every lane runs the same chunk loop and stores (empty voxels add nothing
  // and store zeros), so the stores stay whole-wave and coalesced
  for (int c0 = 0; c0 < c; c0 += CH) {
    float acc[CH];
#pragma unroll
    for (int q = 0; q < CH; q++) acc[q] = 0.0f;
    if (vec && c0 + CH <= c) {
#pragma unroll
      for (int s = 0; s < kHold; s++) {
        if (s < m) {
#pragma unroll
          for (int q = 0; q < CH; q += 4) {
            const float4 x = *reinterpret_cast<const float4*>(rows[s] + c0 + q);
            acc[q] += x.x * inv;
            acc[q + 1] += x.y * inv;
            acc[q + 2] += x.z * inv;
            acc[q + 3] += x.w * inv;
          }
        }
      }
      for (int s = kHold; s < m; s++) {
        const float* row = FT + (size_t)P[s] * c + c0;
#pragma unroll
        for (int q = 0; q < CH; q += 4) {
          const float4 x = *reinterpret_cast<const float4*>(row + q);
          acc[q] += x.x * inv;
          acc[q + 1] += x.y * inv;
          acc[q + 2] += x.z * inv;
          acc[q + 3] += x.w * inv;
        }
      }
    } else {
      for (int s = 0; s < m; s++) {
        const float* row = FT + (size_t)P[s] * c + c0;
#pragma unroll
        for (int q = 0; q < CH; q++)
          if (c0 + q < c) acc[q] += row[q] * inv;
      }
    }
#pragma unroll
    for (int q = 0; q < CH; q++)
      // nontemporal: the 537 MB grid at c5 is written once (c5 step -2%)
      if (c0 + q < c) __builtin_nontemporal_store(acc[q], &O[(size_t)(c0 + q) * r3]);
  }
}

pcr_status run_voxelize_big(PrepMode mode, const float* features, const float* coords_f,
                            const int* coords_i, int b, int c, int n, int r, float* out, int* ind,
                            int* cnt, void* workspace, size_t ws_bytes, hipStream_t stream,
                            const char* name) {
  const int r3 = r * r * r;
  PCR_REQUIRE(cnt != nullptr && ind != nullptr, "%s: ind and cnt required", name);
  PCR_REQUIRE((int64_t)b * n < (1ll << 31) && (int64_t)b * r3 < (1ll << 31),
              "%s: batch too large for the sorted path", name);
  BigVoxWs ws;
  // with room for the point-major feature copy the coalesced gather runs,
  // else the direct one (same results)
  size_t need = big_ws_layout(b, n, r, &ws, workspace, c);
  if (workspace == nullptr || ws_bytes < need) need = big_ws_layout(b, n, r, &ws, workspace, 0);
  PCR_REQUIRE(workspace != nullptr && ws_bytes >= need, "%s: workspace too small (%zu < %zu)",
              name, ws_bytes, need);
  if (hipMemsetAsync(cnt, 0, (size_t)b * r3 * sizeof(int), stream) != hipSuccess ||
      hipMemsetAsync(ws.big, 0, sizeof(int), stream) != hipSuccess) {
    set_error("%s: memset failed", name);
    return PCR_ERR_LAUNCH;
  }
  const dim3 pts(ceil_div(n, 256), b);
  auto key = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, pts, dim3(256), 0, stream, coords_f, coords_i, n, r, ind, cnt,
                       ws.slot);
  };
  switch (mode) {
    case kSphCoords: key(vox_key_big_kernel<kSphCoords>); break;
    case kSphNormalize: key(vox_key_big_kernel<kSphNormalize>); break;
    case kCube: key(vox_key_big_kernel<kCube>); break;
  }
  if (c > 0 && out) {
    const dim3 tiles(ws.ntile, b);
    hipLaunchKernelGGL(vox_scan_tiles_kernel, tiles, dim3(kBigScanThreads), 0, stream, cnt, r3,
                       ws.ntile, ws.tsum);
    hipLaunchKernelGGL(vox_scan_apply_kernel, tiles, dim3(kBigScanThreads), 0, stream, cnt, r3,
                       ws.ntile, ws.tsum, ws.start);
    hipLaunchKernelGGL(vox_place_big_kernel, pts, dim3(256), 0, stream, ind, ws.slot, n, r3,
                       ws.start, ws.perm_u);
    hipLaunchKernelGGL(vox_rank_big_kernel, pts, dim3(256), 0, stream, ind, ws.slot, n, r3, cnt,
                       ws.start, ws.perm_u, ws.perm, ws.big);
    const int kbits = n > 1 ? 32 - __builtin_clz((unsigned)(n - 1)) : 1;
    hipLaunchKernelGGL(vox_seg_sort_kernel, dim3(64), dim3(kSegSortThreads), 0, stream, ws.big,
                       cnt, ws.start, n, r3, kbits, ws.perm_u, ws.perm);
    if (ws.featT) {
      hipLaunchKernelGGL(feat_transpose_kernel, dim3(ceil_div(n, 64), ceil_div(c, 64), b),
                         dim3(256), 0, stream, features, c, n, ws.featT);
      hipLaunchKernelGGL(vox_gather_big_t_kernel<32>, dim3(ceil_div(r3, 256), b), dim3(256), 0,
                         stream, ws.featT, cnt, ws.start, ws.perm, c, n, r3, out);
      hipLaunchKernelGGL(vox_seg_gather_kernel<true>, dim3(64), dim3(256), 0, stream, ws.big,
                         ws.featT, cnt, ws.start, ws.perm, c, n, r3, out);
    } else {
      hipLaunchKernelGGL(vox_gather_big_kernel, dim3(ceil_div(r3, 256), b), dim3(256), 0, stream,
                         features, cnt, ws.start, ws.perm, c, n, r3, out);
      hipLaunchKernelGGL(vox_seg_gather_kernel<false>, dim3(64), dim3(256), 0, stream, ws.big,
                         features, cnt, ws.start, ws.perm, c, n, r3, out);
    }
  }
  return launch_status(name);
}

size_t vox_big_ws_size(int b, int n, int r, int c) {
  return big_ws_layout(b, n, r, nullptr, nullptr, c);
}

void launch_sph_normalize_big(const float* coords, int b, int n, float* norm_coords,
                              hipStream_t stream) {
  hipLaunchKernelGGL(sph_normalize_big_kernel, dim3(b), dim3(kPrepThreads), 0, stream, coords, n,
                     norm_coords);
}

}  // namespace pcr
