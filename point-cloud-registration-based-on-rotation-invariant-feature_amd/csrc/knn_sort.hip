// knn_sort.hip -- the Morton sort of the spatial KNN (knn_spatial.hip): one
// workgroup per (cloud, point set) computes the 30-bit Morton code of every
// point in the cloud's bounding box, sorts (code, index) in LDS and writes
// the sorted SoA coordinates + original indices and the axis-aligned box of
// every 64-point block (KnnSet); clouds of more than kKnnMaxSortN points take
// a global counting sort with the same outputs.
#include "knn_spatial.hpp"

namespace pcr {

constexpr int kSmallSortThreads = 256;
constexpr int kSmallSortN = kSmallSortThreads * kMaxE;

__device__ inline unsigned spread10(unsigned v) {
  v &= 0x3FFu;
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

__device__ inline unsigned quant10(float v, float lo, float scale) {
  float t = (v - lo) * scale;
  if (!(t > 0.0f)) return 0u;  // also NaN
  if (t >= 1023.0f) return 1023u;
  return (unsigned)t;
}

template <int NT>
__global__ __launch_bounds__(NT) void knn_sort_kernel(const float* __restrict__ pts, int n,
                                                      int npad_sort, KnnSet s) {
  extern __shared__ __align__(16) unsigned long long keys[];  // [npad_sort]
  __shared__ float red[6][NT / kWave];
  __shared__ float frame[6];
  if (!PCR_PRIO(0)) latency_kernel_priority();
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int E = npad_sort / NT;
  const float* P = pts + (size_t)b * 3 * n;
  float px[kMaxE], py[kMaxE], pz[kMaxE];
  float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
  for (int e = 0; e < kMaxE; e++) {
    const int i = e * NT + tid;
    const bool ok = e < E && i < n;
    px[e] = ok ? P[i] : __builtin_nanf("");
    py[e] = ok ? P[n + i] : __builtin_nanf("");
    pz[e] = ok ? P[2 * n + i] : __builtin_nanf("");
    mn[0] = fminf(mn[0], px[e]);  // fminf/fmaxf ignore NaN
    mn[1] = fminf(mn[1], py[e]);
    mn[2] = fminf(mn[2], pz[e]);
    mx[0] = fmaxf(mx[0], px[e]);
    mx[1] = fmaxf(mx[1], py[e]);
    mx[2] = fmaxf(mx[2], pz[e]);
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], off, kWave));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off, kWave));
    }
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      red[a][tid >> 6] = mn[a];
      red[3 + a][tid >> 6] = mx[a];
    }
  }
  __syncthreads();
  if (tid < 6) {
    float v = red[tid][0];
    for (int w = 1; w < NT / kWave; w++)
      v = tid < 3 ? fminf(v, red[tid][w]) : fmaxf(v, red[tid][w]);
    frame[tid] = v;
  }
  __syncthreads();
  float lo[3], sc[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = frame[a];
    const float ext = frame[3 + a] - frame[a];
    sc[a] = (ext > 0.0f && ext < __builtin_inff()) ? 1023.0f / ext : 0.0f;
  }
  // coarse counting sort on the top 12 Morton bits (16^3 cells).  The order
  // inside a cell is arbitrary: KNN results never depend on the visiting
  // order (keys are compared lexicographically), only its speed does.
  int* hist = (int*)keys;     // [4096]
  int* order = hist + 4096;   // [n]
  // the coordinates in sorted order, written by the scatter from the
  // registers that already hold them: the block pass reads them from LDS
  // instead of gathering P[order[p]] from global memory (a dependent round
  // trip, microseconds under the grid stream's writes)
  float* sxyz = (float*)(order + n);  // [3][n]
  __shared__ int scan_b[NT / kWave + 1];
  for (int c = tid; c < 4096; c += NT) hist[c] = 0;
  __syncthreads();
  int cell[kMaxE], slot[kMaxE];
#pragma unroll
  for (int e = 0; e < kMaxE; e++) {
    const int i = e * NT + tid;
    cell[e] = -1;
    if (e < E && i < n) {
      const unsigned code = spread10(quant10(px[e], lo[0], sc[0])) |
                            (spread10(quant10(py[e], lo[1], sc[1])) << 1) |
                            (spread10(quant10(pz[e], lo[2], sc[2])) << 2);
      cell[e] = (int)(code >> 18);
      slot[e] = atomicAdd(&hist[cell[e]], 1);
    }
  }
  __syncthreads();
  {
    constexpr int CPT = 4096 / NT;  // bins per thread
    const int c0 = tid * CPT;
    int h[CPT];
    int sum = 0;
#pragma unroll
    for (int q = 0; q < CPT; q++) {
      h[q] = hist[c0 + q];
      sum += h[q];
    }
    const int incl = block_inclusive_scan(sum, scan_b);
    int run = incl - sum;
#pragma unroll
    for (int q = 0; q < CPT; q++) {
      hist[c0 + q] = run;
      run += h[q];
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kMaxE; e++)
    if (cell[e] >= 0) {
      const int pos = hist[cell[e]] + slot[e];
      order[pos] = e * NT + tid;
      sxyz[pos] = px[e];
      sxyz[n + pos] = py[e];
      sxyz[2 * n + pos] = pz[e];
    }
  __syncthreads();
  // sorted SoA + per-block boxes (one wave per block)
  const size_t base = (size_t)b * s.npad;
  const int lane = tid & 63;
  for (int blk = tid >> 6; blk < s.nblk; blk += NT / kWave) {
    const int p = blk * kBlk + lane;
    float x = __builtin_nanf(""), y = x, z = x;
    int j = -1;
    if (p < n) {
      j = order[p];
      x = sxyz[p];
      y = sxyz[n + p];
      z = sxyz[2 * n + p];
      if (s.inv) s.inv[(size_t)b * n + j] = p;
    }
    s.x[base + p] = x;
    s.y[base + p] = y;
    s.z[base + p] = z;
    s.j[base + p] = j;
    float bmn[3] = {x, y, z}, bmx[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (p >= n || bmn[a] != bmn[a]) {
        bmn[a] = __builtin_inff();
        bmx[a] = -__builtin_inff();
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        bmn[a] = fminf(bmn[a], __shfl_xor(bmn[a], off, kWave));
        bmx[a] = fmaxf(bmx[a], __shfl_xor(bmx[a], off, kWave));
      }
    }
    if (lane < 8) {
      float v = 0.0f;
      if (lane < 3) v = bmn[lane == 0 ? 0 : (lane == 1 ? 1 : 2)];
      else if (lane < 6) v = bmx[lane == 3 ? 0 : (lane == 4 ? 1 : 2)];
      s.box[((size_t)b * s.nblk + blk) * 8 + lane] = v;
    }
  }
}

// ---- clouds of more than kKnnMaxSortN points: the same coarse Morton
// order through a global counting sort (frame, cell counts, scan, scatter,
// block boxes); order inside a cell arbitrary, as above.
__global__ __launch_bounds__(kSortBlock) void knn_big_frame_kernel(const float* __restrict__ pts,
                                                                   int n, KnnSet s) {
  __shared__ float red[6][kSortBlock / kWave];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* P = pts + (size_t)b * 3 * n;
  float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int i = tid; i < n; i += kSortBlock) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float v = P[i + (size_t)a * n];
      mn[a] = fminf(mn[a], v);
      mx[a] = fmaxf(mx[a], v);
    }
  }
  int* cnt = s.cell + (size_t)b * kBigCells;
  for (int c = tid; c < kBigCells; c += kSortBlock) cnt[c] = 0;
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], off, kWave));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], off, kWave));
    }
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      red[a][tid >> 6] = mn[a];
      red[3 + a][tid >> 6] = mx[a];
    }
  }
  __syncthreads();
  if (tid < 3) {
    float lo = red[tid][0], hi = red[3 + tid][0];
    for (int w = 1; w < kSortBlock / kWave; w++) {
      lo = fminf(lo, red[tid][w]);
      hi = fmaxf(hi, red[3 + tid][w]);
    }
    const float ext = hi - lo;
    s.frame[(size_t)b * 8 + tid] = lo;
    s.frame[(size_t)b * 8 + 3 + tid] = (ext > 0.0f && ext < __builtin_inff()) ? 1023.0f / ext : 0.0f;
  }
}

__global__ __launch_bounds__(256) void knn_big_count_kernel(const float* __restrict__ pts, int n,
                                                            KnnSet s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= n) return;
  const float* P = pts + (size_t)b * 3 * n;
  const float* f = s.frame + (size_t)b * 8;
  const unsigned code = spread10(quant10(P[i], f[0], f[3])) |
                        (spread10(quant10(P[i + n], f[1], f[4])) << 1) |
                        (spread10(quant10(P[i + 2 * (size_t)n], f[2], f[5])) << 2);
  const int c = (int)(code >> (30 - kBigCellBits));
  s.pcell[(size_t)b * n + i] = c;
  s.pslot[(size_t)b * n + i] = atomicAdd(&s.cell[(size_t)b * kBigCells + c], 1);
}

__global__ __launch_bounds__(kSortBlock) void knn_big_scan_kernel(KnnSet s) {
  __shared__ int scan_b[kSortBlock / kWave + 1];
  constexpr int CPT = kBigCells / kSortBlock;
  int* cnt = s.cell + (size_t)blockIdx.x * kBigCells;
  const int c0 = threadIdx.x * CPT;
  int sum = 0;
  for (int q = 0; q < CPT; q++) sum += cnt[c0 + q];
  const int incl = block_inclusive_scan(sum, scan_b);
  int run = incl - sum;
  for (int q = 0; q < CPT; q++) {
    const int v = cnt[c0 + q];
    cnt[c0 + q] = run;
    run += v;
  }
}

__global__ __launch_bounds__(256) void knn_big_scatter_kernel(const float* __restrict__ pts, int n,
                                                              KnnSet s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const size_t base = (size_t)b * s.npad;
  if (i < n) {
    const float* P = pts + (size_t)b * 3 * n;
    const size_t o = base + s.cell[(size_t)b * kBigCells + s.pcell[(size_t)b * n + i]] +
                     s.pslot[(size_t)b * n + i];
    s.x[o] = P[i];
    s.y[o] = P[i + n];
    s.z[o] = P[i + 2 * (size_t)n];
    s.j[o] = i;
    s.inv[(size_t)b * n + i] = (int)(o - base);
  } else if (i < s.npad) {
    s.x[base + i] = s.y[base + i] = s.z[base + i] = __builtin_nanf("");
    s.j[base + i] = -1;
  }
}

// one wave per 64-point block
__global__ __launch_bounds__(256) void knn_big_boxes_kernel(KnnSet s) {
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  if (blk >= s.nblk) return;
  const size_t p = (size_t)b * s.npad + (size_t)blk * kBlk + lane;
  const float v[3] = {s.x[p], s.y[p], s.z[p]};
  float bmn[3], bmx[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const bool real = s.j[p] >= 0 && v[a] == v[a];
    bmn[a] = real ? v[a] : __builtin_inff();
    bmx[a] = real ? v[a] : -__builtin_inff();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      bmn[a] = fminf(bmn[a], __shfl_xor(bmn[a], off, kWave));
      bmx[a] = fmaxf(bmx[a], __shfl_xor(bmx[a], off, kWave));
    }
  }
  const float bv = lane == 0 ? bmn[0] : lane == 1 ? bmn[1] : lane == 2 ? bmn[2]
                 : lane == 3 ? bmx[0] : lane == 4 ? bmx[1] : lane == 5 ? bmx[2] : 0.0f;
  if (lane < 8) s.box[((size_t)b * s.nblk + blk) * 8 + lane] = bv;
}

void launch_sort(const float* pts, int b, int n, const KnnSet& s, hipStream_t st) {
  PCR_PRIO_INIT();
  if (n > kKnnMaxSortN) {
    hipLaunchKernelGGL(knn_big_frame_kernel, dim3(b), dim3(kSortBlock), 0, st, pts, n, s);
    hipLaunchKernelGGL(knn_big_count_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, pts, n,
                       s);
    hipLaunchKernelGGL(knn_big_scan_kernel, dim3(b), dim3(kSortBlock), 0, st, s);
    hipLaunchKernelGGL(knn_big_scatter_kernel, dim3(ceil_div(s.npad, 256), b), dim3(256), 0, st,
                       pts, n, s);
    hipLaunchKernelGGL(knn_big_boxes_kernel, dim3(ceil_div(s.nblk, 4), b), dim3(256), 0, st, s);
    return;
  }
  // clouds of <= 1024 points: 256 threads (four points each), so the sort
  // fits on a CU beside the other stream's grid kernel
  const size_t smem = 4096 * 4 + (size_t)n * 16;  // hist | order | sorted x y z
  if (n <= kSmallSortN) {
    const int npad_sort = next_pow2(n < kSmallSortThreads ? kSmallSortThreads : n);
    allow_big_lds(knn_sort_kernel<kSmallSortThreads>, smem);
    hipLaunchKernelGGL((knn_sort_kernel<kSmallSortThreads>), dim3(b), dim3(kSmallSortThreads),
                       smem, st, pts, n, npad_sort, s);
  } else {
    const int npad_sort = next_pow2(n < kSortBlock ? kSortBlock : n);
    allow_big_lds(knn_sort_kernel<kSortBlock>, smem);
    hipLaunchKernelGGL((knn_sort_kernel<kSortBlock>), dim3(b), dim3(kSortBlock), smem, st, pts,
                       n, npad_sort, s);
  }
}

}  // namespace pcr
