// gridsub.hip -- batched grid subsampling (voxel-grid barycentres) of raw
// scans for gfx950: KPConv's grid_subsampling
// (cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp) for b
// ragged clouds at once.  The contract and its scalar math are
// include/pcr_gridsub.h.
//
// Every cell is summed in ascending point index, in fp32, without float
// atomics: a stable sort of (key, point) gives that order.  Per call, all on
// the caller's stream, every launch over (tiles, clouds):
//   bounds   min / max of the valid points as order-preserving unsigned
//            integers (exact and order-free), a non-finite flag: one partial
//            per workgroup; then a wave per cloud folds them and makes
//            origin, dims, status and the number of sort passes
//   keys     the 64-bit cell key of every valid point
//   sort     stable LSD radix sort of (key, point), 8 bits per pass, over the
//            key bits in use only.  The host cannot know that number without
//            a sync, so it queues all kGsPasses passes and the passes past
//            the last used bit return at once; the result's buffer follows
//            from the number of passes that ran.  A pass: per-tile digit
//            histograms, then each tile places its elements after the
//            smaller digits and the earlier tiles (ranks inside a tile by
//            ballots, as common.hpp's wg_radix_sort)
//   heads    key[i] != key[i - 1] starts a cell: per-tile head counts, then a
//            scan gives every sorted point its output slot (cell_of) and
//            every slot its segment start
//   rows     coordinates and features, [3 + c][n], transposed to point-major
//            rows [n][3 + c] through LDS tiles, so that a point's channels
//            are one contiguous read
//   sums     one thread per (slot, channel), channels across lanes: the
//            segment summed serially, 32 or 8 rows in flight; a workgroup's 64
//            slots go out through an LDS tile so the stores are contiguous;
//            slots past out_count get zeros
// No loop depends on the data beyond a segment's length (<= n), nothing
// spins, and every output element is written whatever the status.
#include "common.hpp"
#include "pcr_gridsub.h"

namespace pcr {

constexpr int kGsTile = 1024;        // elements per sort / scan tile = threads per workgroup
constexpr int kGsPasses = 8;         // 8 x 8 bits >= the 60 key bits a status-0 cloud can use
constexpr int kGsBoundsBlocks = 64;  // bounds workgroups per cloud: one lane each in the setup
constexpr int kGsMeta = 8;           // ints per cloud: valid points, NX, NY, passes

static_assert(kGsBoundsBlocks <= kWave, "the setup wave folds one partial per lane");

struct GsWs {
  unsigned* acc;               // [b][kGsBoundsBlocks][8] per workgroup: ~min xyz, max xyz
                               // (pcr_gridsub_ord), non-finite flag
  int* meta;                   // [b][kGsMeta]
  unsigned long long* key[2];  // [b][n] ping-pong
  int* idx[2];                 // [b][n] ping-pong
  int* hist;                   // [b][ntile][256]
  int* tsum;                   // [b][ntile] heads per tile
  int* start;                  // [b][n] first sorted position of each output slot
  float* rows;                 // [b][n][3 + c] point-major coordinates and features
  int ntile;
};

static size_t gs_ws_layout(int b, int n, int c, GsWs* ws, void* base) {
  const size_t nk = (size_t)b * n;
  const int ntile = ceil_div(n > 0 ? n : 1, kGsTile);
  size_t off = 0;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* q = p ? p + off : nullptr;
    off = align_up(off + bytes, 256);
    return q;
  };
  unsigned* acc = (unsigned*)take((size_t)b * kGsBoundsBlocks * 8 * 4);
  int* meta = (int*)take((size_t)b * kGsMeta * 4);
  unsigned long long* k0 = (unsigned long long*)take(nk * 8);
  unsigned long long* k1 = (unsigned long long*)take(nk * 8);
  int* i0 = (int*)take(nk * 4);
  int* i1 = (int*)take(nk * 4);
  int* hist = (int*)take((size_t)b * ntile * 256 * 4);
  int* tsum = (int*)take((size_t)b * ntile * 4);
  int* start = (int*)take(nk * 4);
  float* rows = (float*)take(nk * (size_t)(3 + c) * 4);
  if (ws) {
    ws->acc = acc;
    ws->meta = meta;
    ws->key[0] = k0;
    ws->key[1] = k1;
    ws->idx[0] = i0;
    ws->idx[1] = i1;
    ws->hist = hist;
    ws->tsum = tsum;
    ws->start = start;
    ws->rows = rows;
    ws->ntile = ntile;
  }
  return off;
}

__device__ inline int gs_valid(const int* counts_in, int q, int n) {
  const int m = counts_in ? counts_in[q] : n;
  return (m >= 1 && m <= n) ? m : 0;
}

// bounds of the valid points: workgroup g of cloud q writes its maxima of ~ord
// (the minimum) and ord (the maximum) per axis and its non-finite flag to
// acc[q][g]; a workgroup without points writes zeros, which change nothing
__global__ __launch_bounds__(256) void gridsub_bounds_kernel(const float* __restrict__ xyz,
                                                             const int* __restrict__ counts_in,
                                                             int n, unsigned* __restrict__ acc) {
  __shared__ unsigned red[4][8];
  const int q = blockIdx.y;
  const int m = gs_valid(counts_in, q, n);
  const float* X = xyz + (size_t)q * 3 * n;
  unsigned v[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};  // lo xyz, hi xyz, bad
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const float x = X[(size_t)d * n + i];
      const unsigned u = pcr_gridsub_ord(x);
      v[6] |= pcr_gridsub_finite(x) ? 0u : 1u;
      v[d] = max(v[d], ~u);
      v[3 + d] = max(v[3 + d], u);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 7; k++) v[k] = max(v[k], (unsigned)__shfl_xor((int)v[k], off, kWave));
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 7; k++) red[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    acc[((size_t)q * kGsBoundsBlocks + blockIdx.x) * 8 + k] =
        max(max(red[0][k], red[1][k]), max(red[2][k], red[3][k]));
  }
}

// a wave per cloud: folds the workgroups' bounds (lane g takes acc[q][g]);
// lane 0 makes the status, origin, dims and the sort's parameters
__global__ __launch_bounds__(64) void gridsub_setup_kernel(
    const unsigned* __restrict__ acc, const int* __restrict__ counts_in, int nblocks, int n,
    float cell, float* __restrict__ origin, int* __restrict__ dims, int* __restrict__ status,
    int* __restrict__ meta) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int m = gs_valid(counts_in, q, n);
  unsigned A[7];
#pragma unroll
  for (int k = 0; k < 7; k++)
    A[k] = lane < nblocks ? acc[((size_t)q * kGsBoundsBlocks + lane) * 8 + k] : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 7; k++) A[k] = max(A[k], (unsigned)__shfl_xor((int)A[k], off, kWave));
  if (lane != 0) return;
  float org[3] = {0.0f, 0.0f, 0.0f};
  int dm[3] = {0, 0, 0}, st;
  if (m == 0) {
    st = PCR_GRIDSUB_COUNT;
  } else if (A[6]) {
    st = PCR_GRIDSUB_NONFINITE;
  } else {
    float mn[3], mx[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      mn[d] = pcr_gridsub_unord(~A[d]);
      mx[d] = pcr_gridsub_unord(A[3 + d]);
    }
    st = pcr_gridsub_grid(mn, mx, cell, org, dm);
  }
  int* M = meta + (size_t)q * kGsMeta;
  const bool ok = st == PCR_GRIDSUB_OK;
  M[0] = ok ? m : 0;
  M[1] = ok ? dm[0] : 1;
  M[2] = ok ? dm[1] : 1;
  M[3] = ok ? (pcr_gridsub_key_bits(dm[0], dm[1], dm[2]) + 7) / 8 : 0;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    origin[(size_t)q * 3 + d] = org[d];
    dims[(size_t)q * 3 + d] = dm[d];
  }
  status[q] = st;
}

// the key of every valid point, and the identity permutation
__global__ __launch_bounds__(256) void gridsub_key_kernel(
    const float* __restrict__ xyz, int n, float cell, const float* __restrict__ origin,
    const int* __restrict__ meta, unsigned long long* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  const int* M = meta + (size_t)q * kGsMeta;
  if (i >= M[0]) return;
  const float* X = xyz + (size_t)q * 3 * n;
  const float* O = origin + (size_t)q * 3;
  const int ix = pcr_gridsub_index(X[i], O[0], cell);
  const int iy = pcr_gridsub_index(X[(size_t)n + i], O[1], cell);
  const int iz = pcr_gridsub_index(X[2 * (size_t)n + i], O[2], cell);
  key[(size_t)q * n + i] = pcr_gridsub_key(ix, iy, iz, M[1], M[2]);
  idx[(size_t)q * n + i] = i;
}

// sort pass, part 1: the digit histogram of every tile
__global__ __launch_bounds__(kGsTile) void gridsub_hist_kernel(
    const unsigned long long* __restrict__ k0, const unsigned long long* __restrict__ k1, int n,
    int ntile, int pass, const int* __restrict__ meta, int* __restrict__ hist) {
  __shared__ int h[256];
  const int t = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int* M = meta + (size_t)q * kGsMeta;
  if (pass >= M[3]) return;
  const int m = M[0];
  const unsigned long long* K = ((pass & 1) ? k1 : k0) + (size_t)q * n;
  if (tid < 256) h[tid] = 0;
  __syncthreads();
  const int e = t * kGsTile + tid;
  if (e < m) atomicAdd(&h[(int)(K[e] >> (8 * pass)) & 255], 1);
  __syncthreads();
  if (tid < 256) hist[((size_t)q * ntile + t) * 256 + tid] = h[tid];
}

// sort pass, part 2: each tile's elements to their places.  Digit d of tile t
// starts after every smaller digit (all tiles) and digit d of the tiles
// before t; inside the tile a wave ranks its 64 elements among the same digit
// with 8 ballots and the waves' digit counts are scanned in wave order, so
// equal digits keep their order.
__global__ __launch_bounds__(kGsTile) void gridsub_scatter_kernel(
    unsigned long long* __restrict__ k0, unsigned long long* __restrict__ k1,
    int* __restrict__ i0, int* __restrict__ i1, int n, int ntile, int pass,
    const int* __restrict__ meta, const int* __restrict__ hist) {
  constexpr int NW = kGsTile / kWave;
  __shared__ int base[256];
  __shared__ int tot[4];
  __shared__ int wtab[NW * 256];
  const int t = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int* M = meta + (size_t)q * kGsMeta;
  if (pass >= M[3]) return;
  const int m = M[0];
  if (t * kGsTile >= m) return;
  const bool odd = pass & 1;
  const unsigned long long* Ks = (odd ? k1 : k0) + (size_t)q * n;
  unsigned long long* Kd = (odd ? k0 : k1) + (size_t)q * n;
  const int* Is = (odd ? i1 : i0) + (size_t)q * n;
  int* Id = (odd ? i0 : i1) + (size_t)q * n;
  for (int i = tid; i < NW * 256; i += kGsTile) wtab[i] = 0;
  // the tile's bucket starts
  int before = 0, total = 0;
  if (tid < 256) {
    const int* H = hist + (size_t)q * ntile * 256 + tid;
    const int used = (m + kGsTile - 1) / kGsTile;
    for (int s = 0; s < used; s++) {
      const int c = H[(size_t)s * 256];
      before += s < t ? c : 0;
      total += c;
    }
  }
  int c = total;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int v = __shfl_up(c, off, kWave);
    if (lane >= off) c += v;
  }
  if (tid < 256 && lane == 63) tot[wv] = c;
  __syncthreads();
  if (tid < 256) {
    int add = 0;
    for (int w = 0; w < wv; w++) add += tot[w];
    base[tid] = add + c - total + before;
  }
  // ranks inside the tile
  const int e = t * kGsTile + tid;
  const bool ok = e < m;
  const unsigned long long kv = ok ? Ks[e] : 0ull;
  const int iv = ok ? Is[e] : 0;
  const int dg = (int)(kv >> (8 * pass)) & 255;
  unsigned long long peers = __ballot(ok);
#pragma unroll
  for (int bit = 0; bit < 8; bit++) {
    const bool one = (dg >> bit) & 1;
    const unsigned long long bb = __ballot(ok && one);
    peers &= one ? bb : ~bb;
  }
  const int rank = __popcll(peers & ((1ull << lane) - 1ull));
  if (ok && rank == 0) wtab[wv * 256 + dg] = __popcll(peers);
  __syncthreads();
  if (tid < 256) {
    int run = 0;
    for (int w = 0; w < NW; w++) {
      const int cw = wtab[w * 256 + tid];
      wtab[w * 256 + tid] = run;
      run += cw;
    }
  }
  __syncthreads();
  if (ok) {
    const int dst = base[dg] + wtab[wv * 256 + dg] + rank;
    if (dst < m) {  // always: the histograms count these very elements
      Kd[dst] = kv;
      Id[dst] = iv;
    }
  }
}

// a point index read back from the workspace, kept inside the cloud: what the
// workspace holds is never trusted as an address
__device__ inline int gs_point(int i, int m) { return min(max(i, 0), m - 1); }

__device__ inline bool gs_is_head(const unsigned long long* K, int e) {
  return e == 0 || K[e] != K[e - 1];
}

// cells starting in every tile of the sorted keys
__global__ __launch_bounds__(kGsTile) void gridsub_heads_kernel(
    const unsigned long long* __restrict__ k0, const unsigned long long* __restrict__ k1, int n,
    int ntile, const int* __restrict__ meta, int* __restrict__ tsum) {
  __shared__ int red[kGsTile / kWave];
  const int t = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int* M = meta + (size_t)q * kGsMeta;
  const int m = M[0];
  const unsigned long long* K = ((M[3] & 1) ? k1 : k0) + (size_t)q * n;
  const int e = t * kGsTile + tid;
  const unsigned long long bal = __ballot(e < m && gs_is_head(K, e));
  if ((tid & 63) == 0) red[tid >> 6] = __popcll(bal);
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < kGsTile / kWave; w++) s += red[w];
    tsum[(size_t)q * ntile + t] = s;
  }
}

// every sorted point's output slot: cell_of of its point, the slot's segment
// start; cell_of = -1 for the points past the valid count; out_count
__global__ __launch_bounds__(kGsTile) void gridsub_slots_kernel(
    const unsigned long long* __restrict__ k0, const unsigned long long* __restrict__ k1,
    const int* __restrict__ i0, const int* __restrict__ i1, int n, int ntile,
    const int* __restrict__ meta, const int* __restrict__ tsum, int* __restrict__ start,
    int* __restrict__ cell_of, int* __restrict__ out_count) {
  __shared__ int scan_s[kGsTile / kWave + 1];
  __shared__ int base_s[2];
  const int t = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
  const int* M = meta + (size_t)q * kGsMeta;
  const int m = M[0];
  const bool odd = M[3] & 1;
  const unsigned long long* K = (odd ? k1 : k0) + (size_t)q * n;
  const int* I = (odd ? i1 : i0) + (size_t)q * n;
  if (tid < 64) {
    int s = 0, all = 0;
    for (int r = tid; r < ntile; r += 64) {
      const int v = tsum[(size_t)q * ntile + r];
      s += r < t ? v : 0;
      all += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_xor(s, off, kWave);
      all += __shfl_xor(all, off, kWave);
    }
    if (tid == 0) {
      base_s[0] = s;
      base_s[1] = all;
    }
  }
  const int e = t * kGsTile + tid;
  const int head = (e < m && gs_is_head(K, e)) ? 1 : 0;
  const int incl = block_inclusive_scan(head, scan_s);  // its barriers also publish base_s
  const int slot = base_s[0] + incl - 1;
  if (e < m) {
    if (head) start[(size_t)q * n + slot] = e;
    cell_of[(size_t)q * n + gs_point(I[e], m)] = slot;
  } else if (e < n) {
    cell_of[(size_t)q * n + e] = -1;
  }
  if (t == 0 && tid == 0) out_count[q] = base_s[1];
}

// coordinates (channels 0..2) and features (3..) of every point, [C][n] ->
// rows [n][C], through a 64 x 64 LDS tile (coalesced both ways)
__global__ __launch_bounds__(256) void gridsub_rows_kernel(const float* __restrict__ xyz,
                                                           const float* __restrict__ features,
                                                           int n, int c,
                                                           float* __restrict__ rows) {
  __shared__ float t[64][65];
  const int q = blockIdx.z, n0 = blockIdx.x * 64, c0 = blockIdx.y * 64, C = 3 + c;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int y = ty; y < 64; y += 4) {
    const int ch = c0 + y;
    if (ch < C && n0 + tx < n)
      t[y][tx] = ch < 3 ? xyz[((size_t)q * 3 + ch) * n + n0 + tx]
                        : features[((size_t)q * c + (ch - 3)) * n + n0 + tx];
  }
  __syncthreads();
  for (int y = ty; y < 64; y += 4)
    if (n0 + y < n && c0 + tx < C) rows[((size_t)q * n + n0 + y) * C + c0 + tx] = t[tx][y];
}

// acc + the channel of the rows of N consecutive sorted points, added in that
// order, all N reads in flight first
template <int N>
__device__ inline float gs_add_rows(float acc, const int* __restrict__ I,
                                    const float* __restrict__ R, int C, int m) {
  int pi[N];
  float x[N];
#pragma unroll
  for (int u = 0; u < N; u++) pi[u] = gs_point(I[u], m);
#pragma unroll
  for (int u = 0; u < N; u++) x[u] = R[(size_t)pi[u] * C];
#pragma unroll
  for (int u = 0; u < N; u++) acc += x[u];
  return acc;
}

// A workgroup sums 64 output slots x CW = 2^cw_log2 channels (4 .. 64, the
// smallest that holds all 3 + c, else chunks of 64 over blockIdx.y).  A lane
// is a (slot, channel) with the channel fastest, so a point's row is one
// contiguous read by the lanes of its slot; the wave takes 64 / CW slots per
// step.  The segment's points are added in sorted order (ascending point
// index), 32 rows in flight while that many are left, then eight.  The means go through an LDS tile and leave as
// contiguous slots per channel; slots past out_count get zeros.
__global__ __launch_bounds__(256) void gridsub_sum_kernel(
    const float* __restrict__ rows, int n, int c, int cw_log2, const int* __restrict__ i0,
    const int* __restrict__ i1, const int* __restrict__ meta, const int* __restrict__ start,
    const int* __restrict__ out_count, float* __restrict__ out_xyz,
    float* __restrict__ out_features, int* __restrict__ cell_count) {
  constexpr int kB = 8, kLong = 32;
  __shared__ float t[64][65];
  __shared__ int cnt_s[64];
  const int C = 3 + c, CW = 1 << cw_log2, spw = 64 >> cw_log2;
  const int s0 = blockIdx.x * 64, c0 = blockIdx.y << cw_log2, q = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int chl = lane & (CW - 1), sub = lane >> cw_log2, ch = c0 + chl;
  const int* M = meta + (size_t)q * kGsMeta;
  const int m = M[0], cells = min(out_count[q], m);
  const int* I = ((M[3] & 1) ? i1 : i0) + (size_t)q * n;
  const float* R = rows + (size_t)q * n * C + ch;
  for (int r = 0; r < (CW >> 2); r++) {
    const int sl = (r * 4 + w) * spw + sub;  // 0 .. 63, each once
    const int s = s0 + sl;
    float res = 0.0f;
    int cnt = 0;
    if (s < cells && ch < C) {
      const int lo = min(max(start[(size_t)q * n + s], 0), m);
      const int hi = s + 1 < cells ? min(max(start[(size_t)q * n + s + 1], lo), m) : m;
      cnt = hi - lo;
      float acc = 0.0f;
      int j = lo;
      for (; j + kLong <= hi; j += kLong) acc = gs_add_rows<kLong>(acc, I + j, R, C, m);
      for (; j + kB <= hi; j += kB) acc = gs_add_rows<kB>(acc, I + j, R, C, m);
      for (; j < hi; j++) acc += R[(size_t)gs_point(I[j], m) * C];
      res = ch < 3 ? pcr_gridsub_xyz_mean(acc, cnt) : pcr_gridsub_feat_mean(acc, cnt);
    }
    t[chl][sl] = res;
    if (chl == 0) cnt_s[sl] = cnt;
  }
  __syncthreads();
  const int so = s0 + lane;
  if (so < n) {
    for (int y = w; y < CW; y += 4) {
      const int cho = c0 + y;
      if (cho < C) {
        float* dst = cho < 3 ? out_xyz + ((size_t)q * 3 + cho) * n
                             : out_features + ((size_t)q * c + (cho - 3)) * n;
        dst[so] = t[y][lane];
      }
    }
    if (blockIdx.y == 0 && w == 0) cell_count[(size_t)q * n + so] = cnt_s[lane];
  }
}

}  // namespace pcr

using namespace pcr;

extern "C" size_t pcr_grid_subsample_workspace_size(int b, int n, int c) {
  if (b <= 0 || n <= 0 || c < 0) return 256;
  return gs_ws_layout(b, n, c, nullptr, nullptr);
}

extern "C" pcr_status pcr_grid_subsample(const float* xyz, const float* features,
                                         const int* counts_in, int b, int n, int c, float cell,
                                         float* out_xyz, float* out_features, int* out_count,
                                         int* cell_of, int* cell_count, float* origin, int* dims,
                                         int* status, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 0 && c >= 0, "grid_subsample: negative size");
  PCR_REQUIRE(b == 0 || n >= 1, "grid_subsample: n must be at least 1");
  PCR_REQUIRE(cell > 0.0f && cell - cell == 0.0f, "grid_subsample: cell must be finite and > 0");
  if (b == 0) return PCR_OK;
  PCR_REQUIRE((int64_t)b * n < (1ll << 31) && b <= 65535 && c <= 65532,
              "grid_subsample: batch too large");
  PCR_REQUIRE(xyz && out_xyz && out_count && cell_of && cell_count && origin && dims && status,
              "grid_subsample: null pointer");
  PCR_REQUIRE(c == 0 || (features && out_features),
              "grid_subsample: features and out_features required with c > 0");
  GsWs ws;
  const size_t need = gs_ws_layout(b, n, c, &ws, workspace);
  PCR_REQUIRE(workspace != nullptr && workspace_bytes >= need,
              "grid_subsample: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const int ntile = ws.ntile;
  const dim3 tiles(ntile, b);
  const int nblocks = min(ceil_div(n, 256), kGsBoundsBlocks);
  hipLaunchKernelGGL(gridsub_bounds_kernel, dim3(nblocks, b), dim3(256), 0, st, xyz, counts_in, n,
                     ws.acc);
  hipLaunchKernelGGL(gridsub_setup_kernel, dim3(b), dim3(64), 0, st, ws.acc, counts_in, nblocks,
                     n, cell, origin, dims, status, ws.meta);
  hipLaunchKernelGGL(gridsub_key_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, xyz, n, cell,
                     origin, ws.meta, ws.key[0], ws.idx[0]);
  for (int pass = 0; pass < kGsPasses; pass++) {
    hipLaunchKernelGGL(gridsub_hist_kernel, tiles, dim3(kGsTile), 0, st, ws.key[0], ws.key[1], n,
                       ntile, pass, ws.meta, ws.hist);
    hipLaunchKernelGGL(gridsub_scatter_kernel, tiles, dim3(kGsTile), 0, st, ws.key[0], ws.key[1],
                       ws.idx[0], ws.idx[1], n, ntile, pass, ws.meta, ws.hist);
  }
  hipLaunchKernelGGL(gridsub_heads_kernel, tiles, dim3(kGsTile), 0, st, ws.key[0], ws.key[1], n,
                     ntile, ws.meta, ws.tsum);
  hipLaunchKernelGGL(gridsub_slots_kernel, tiles, dim3(kGsTile), 0, st, ws.key[0], ws.key[1],
                     ws.idx[0], ws.idx[1], n, ntile, ws.meta, ws.tsum, ws.start, cell_of,
                     out_count);
  const int C = 3 + c;
  int cw_log2 = 2;
  while (cw_log2 < 6 && (1 << cw_log2) < C) cw_log2++;
  hipLaunchKernelGGL(gridsub_rows_kernel, dim3(ceil_div(n, 64), ceil_div(C, 64), b), dim3(256), 0,
                     st, xyz, features, n, c, ws.rows);
  hipLaunchKernelGGL(gridsub_sum_kernel, dim3(ceil_div(n, 64), ceil_div(C, 1 << cw_log2), b),
                     dim3(256), 0, st, ws.rows, n, c, cw_log2, ws.idx[0], ws.idx[1], ws.meta,
                     ws.start, out_count, out_xyz, out_features, cell_count);
  return launch_status("grid_subsample");
}
