// hybrid_search.hip -- batched hybrid (radius + max_nn) neighbour search of
// ragged clouds against themselves for gfx950: Open3D's
// KDTreeSearchParamHybrid(radius, max_nn), the search FPFH is defined on.  The
// contract and its scalar math are include/pcr_hybrid.h: the
// result is the brute-force rule there for every input; the cell grid only
// bounds the work.
//
// Per call, all on the caller's stream:
//   bounds   min / max of the valid points with three finite coordinates as
//            order-preserving unsigned integers (exact and order-free): one
//            partial per workgroup
//   setup    a workgroup per cloud: wave 0 folds the partials and makes
//            origin, 1 / side and dims (pcr_hybrid_grid); all threads zero the
//            cloud's cell counters
//   count    the cell of every valid finite point (-1 for the others), and the
//            points per cell (integer atomics)
//   scan     a workgroup per cloud: the cells' first positions
//   scatter  every point to a position of its cell (x, y, z, index as one
//            float4).  The order inside a cell varies from run to run; the
//            result does not: selection is on the 64-bit key (bits of d, j)
//   query    a workgroup per 32 consecutive queries, a wave per query in
//            turn.  The wave strides the 27 cells around the query's (nine
//            contiguous ranges, x fastest), and compacts the keys within the
//            radius into its LDS buffer by ballot.  With more than k of them
//            it finds the k-th smallest key by a radix selection over the 64
//            key bits, 8 bits a pass (a 256-bin LDS histogram per wave; it
//            stops once a digit's keys are exactly the ones still needed), from
//            the buffer -- or, when more keys are within the radius than the
//            buffer holds, from the cells again: 8 more sweeps, no larger
//            allocation.  The keys up to the threshold (at most 128) are
//            sorted in registers by a bitonic network and go to the
//            workgroup's LDS tile [query][slot], which leaves as rows that are
//            contiguous along n.
// No trip count depends on the data beyond n, k and the 8 passes over the key
// bits; nothing spins; no float atomics; every index read back from the
// workspace is clamped before it is an address; every output element is
// written.
#include "common.hpp"
#include "pcr_gridsub.h"  // pcr_gridsub_ord / _unord: the bounds' integer order
#include "pcr_hybrid.h"

namespace pcr {

constexpr int kHyBoundsBlocks = 64;  // bounds workgroups per cloud: one lane each in the setup
constexpr int kHyMeta = 16;          // ints per cloud: m, dims, origin bits, 1 / side bits
constexpr int kHyWaves = 4;          // waves per query workgroup
constexpr int kHyTile = 32;          // queries per query workgroup
constexpr int kHyCap = PCR_HYBRID_WAVE_CAP;
constexpr int kHyScan = 1024;        // threads of the scan workgroup

static_assert(kHyBoundsBlocks <= kWave, "the setup wave folds one partial per lane");
static_assert(PCR_HYBRID_MAX_K <= 2 * kWave, "the sort holds two keys per lane");
static_assert(kHyCap >= PCR_HYBRID_MAX_K, "a row that is not cut fits the buffer");

struct HyWs {
  unsigned* acc;  // [b][kHyBoundsBlocks][8] ~min xyz, max xyz, any finite point
  int* meta;      // [b][kHyMeta]
  int* hist;      // [b][ncell] points per cell; the scatter counts them down
  int* start;     // [b][ncell + 1] first position of each cell
  int* cellof;    // [b][n] cell of each point, -1: in no cell
  float4* pts;    // [b][n] points in cell order: x, y, z, index bits
  int ncell;      // gmax^3
  int gmax;
};

static size_t hy_ws_layout(int b, int n, HyWs* ws, void* base) {
  const int g = pcr_hybrid_gmax(n);
  const int ncell = g * g * g;
  const size_t nk = (size_t)b * n;
  size_t off = 0;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* q = p ? p + off : nullptr;
    off = align_up(off + bytes, 256);
    return q;
  };
  unsigned* acc = (unsigned*)take((size_t)b * kHyBoundsBlocks * 8 * 4);
  int* meta = (int*)take((size_t)b * kHyMeta * 4);
  int* hist = (int*)take((size_t)b * ncell * 4);
  int* start = (int*)take((size_t)b * (ncell + 1) * 4);
  int* cellof = (int*)take(nk * 4);
  float4* pts = (float4*)take(nk * 16);
  if (ws) {
    ws->acc = acc;
    ws->meta = meta;
    ws->hist = hist;
    ws->start = start;
    ws->cellof = cellof;
    ws->pts = pts;
    ws->ncell = ncell;
    ws->gmax = g;
  }
  return off;
}

__device__ inline int hy_valid(const int* counts, int q, int n) {
  return counts ? min(max(counts[q], 0), n) : n;
}

// what the setup left in the workspace, kept inside the layout
struct HyGrid {
  int m, dx, dy, dz;
  float ox, oy, oz, inv;
};

__device__ inline HyGrid hy_grid(const int* meta, int q, int n, int gmax) {
  const int* M = meta + (size_t)q * kHyMeta;
  HyGrid g;
  g.m = min(max(M[0], 0), n);
  g.dx = min(max(M[1], 1), gmax);
  g.dy = min(max(M[2], 1), gmax);
  g.dz = min(max(M[3], 1), gmax);
  g.ox = __int_as_float(M[4]);
  g.oy = __int_as_float(M[5]);
  g.oz = __int_as_float(M[6]);
  g.inv = __int_as_float(M[7]);
  return g;
}

// bounds of the valid points whose coordinates are all finite: workgroup g of
// cloud q writes its maxima of ~ord (the minimum) and ord (the maximum) per
// axis and whether it saw such a point; zeros change nothing in the fold
__global__ __launch_bounds__(256) void hybrid_bounds_kernel(const float* __restrict__ xyz,
                                                            const int* __restrict__ counts, int n,
                                                            unsigned* __restrict__ acc) {
  __shared__ unsigned red[4][8];
  const int q = blockIdx.y;
  const int m = hy_valid(counts, q, n);
  const float* X = xyz + (size_t)q * 3 * n;
  unsigned v[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};  // lo xyz, hi xyz, any
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const float p[3] = {X[i], X[(size_t)n + i], X[2 * (size_t)n + i]};
    if (!pcr_hybrid_finite3(p[0], p[1], p[2])) continue;
    v[6] = 1u;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const unsigned u = pcr_gridsub_ord(p[d]);
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
    acc[((size_t)q * kHyBoundsBlocks + blockIdx.x) * 8 + k] =
        max(max(red[0][k], red[1][k]), max(red[2][k], red[3][k]));
  }
}

// a workgroup per cloud: wave 0 folds the bounds (lane g takes acc[q][g]) and
// its lane 0 makes the grid; every thread zeroes cell counters
__global__ __launch_bounds__(256) void hybrid_setup_kernel(const unsigned* __restrict__ acc,
                                                           const int* __restrict__ counts,
                                                           int nblocks, int n, float radius,
                                                           int gmax, int ncell,
                                                           int* __restrict__ meta,
                                                           int* __restrict__ hist) {
  const int q = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < ncell; c += blockDim.x) hist[(size_t)q * ncell + c] = 0;
  if (tid >= kWave) return;
  unsigned A[7];
#pragma unroll
  for (int k = 0; k < 7; k++)
    A[k] = tid < nblocks ? acc[((size_t)q * kHyBoundsBlocks + tid) * 8 + k] : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 7; k++) A[k] = max(A[k], (unsigned)__shfl_xor((int)A[k], off, kWave));
  if (tid != 0) return;
  float mn[3], mx[3], org[3], inv;
  int dm[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    mn[d] = pcr_gridsub_unord(~A[d]);
    mx[d] = pcr_gridsub_unord(A[3 + d]);
  }
  pcr_hybrid_grid(mn, mx, A[6] != 0u, radius, gmax, org, &inv, dm);
  int* M = meta + (size_t)q * kHyMeta;
  M[0] = hy_valid(counts, q, n);
#pragma unroll
  for (int d = 0; d < 3; d++) {
    M[1 + d] = dm[d];
    M[4 + d] = __float_as_int(org[d]);
  }
  M[7] = __float_as_int(inv);
}

// the cell of every point (-1: past the count or not finite) and the cells'
// populations
__global__ __launch_bounds__(256) void hybrid_count_kernel(const float* __restrict__ xyz, int n,
                                                           int gmax, int ncell,
                                                           const int* __restrict__ meta,
                                                           int* __restrict__ cellof,
                                                           int* __restrict__ hist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  if (i >= n) return;
  const HyGrid g = hy_grid(meta, q, n, gmax);
  const float* X = xyz + (size_t)q * 3 * n;
  int c = -1;
  if (i < g.m) {
    const float x = X[i], y = X[(size_t)n + i], z = X[2 * (size_t)n + i];
    if (pcr_hybrid_finite3(x, y, z)) {
      const int cx = pcr_hybrid_cell(x, g.ox, g.inv, g.dx);
      const int cy = pcr_hybrid_cell(y, g.oy, g.inv, g.dy);
      const int cz = pcr_hybrid_cell(z, g.oz, g.inv, g.dz);
      c = cx + g.dx * (cy + g.dy * cz);  // < dx dy dz <= ncell
      atomicAdd(&hist[(size_t)q * ncell + c], 1);
    }
  }
  cellof[(size_t)q * n + i] = c;
}

// a workgroup per cloud: start[c] = the points in the cells before c, for c =
// 0 .. dx dy dz (the last entry is the number of points in cells)
__global__ __launch_bounds__(kHyScan) void hybrid_scan_kernel(int n, int gmax, int ncell,
                                                              const int* __restrict__ meta,
                                                              const int* __restrict__ hist,
                                                              int* __restrict__ start) {
  __shared__ int scan_s[kHyScan / kWave + 1];
  const int q = blockIdx.x, tid = threadIdx.x;
  const HyGrid g = hy_grid(meta, q, n, gmax);
  const int nc = g.dx * g.dy * g.dz;
  const int per = (nc + kHyScan - 1) / kHyScan;
  const int c0 = min(tid * per, nc), c1 = min(c0 + per, nc);
  const int* H = hist + (size_t)q * ncell;
  int* S = start + (size_t)q * (ncell + 1);
  int s = 0;
  for (int c = c0; c < c1; c++) s += H[c];
  const int incl = block_inclusive_scan(s, scan_s);
  int run = incl - s;
  for (int c = c0; c < c1; c++) {
    S[c] = run;
    run += H[c];
  }
  if (tid == kHyScan - 1) S[nc] = incl;
}

// every point in a cell to one of its cell's positions
__global__ __launch_bounds__(256) void hybrid_scatter_kernel(const float* __restrict__ xyz, int n,
                                                             int gmax, int ncell,
                                                             const int* __restrict__ meta,
                                                             const int* __restrict__ cellof,
                                                             const int* __restrict__ start,
                                                             int* __restrict__ hist,
                                                             float4* __restrict__ pts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  if (i >= n) return;
  const int c = cellof[(size_t)q * n + i];
  if (c < 0) return;
  const HyGrid g = hy_grid(meta, q, n, gmax);
  const int cc = min(c, g.dx * g.dy * g.dz - 1);
  const int left = atomicSub(&hist[(size_t)q * ncell + cc], 1);  // count .. 1
  const int pos = min(max(start[(size_t)q * (ncell + 1) + cc] + left - 1, 0), n - 1);
  const float* X = xyz + (size_t)q * 3 * n;
  pts[(size_t)q * n + pos] =
      make_float4(X[i], X[(size_t)n + i], X[2 * (size_t)n + i], __int_as_float(i));
}

// orders the wave's LDS accesses (its LDS operations complete in order; this
// keeps the compiler's order too)
__device__ inline void hy_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline unsigned long long hy_min(unsigned long long a, unsigned long long b) {
  return a < b ? a : b;
}
__device__ inline unsigned long long hy_max(unsigned long long a, unsigned long long b) {
  return a < b ? b : a;
}

// one compare-exchange step of the bitonic network between lanes (J < 64) for
// the element at index idx
template <int J, int KK>
__device__ inline void hy_cmpx(unsigned long long& v, int idx) {
  const unsigned long long o = shfl_xor_u64(v, J);
  const bool take_min = ((idx & J) == 0) == ((idx & KK) == 0);
  v = take_min ? hy_min(v, o) : hy_max(v, o);
}

template <int KK, int J = KK / 2>
__device__ inline void hy_merge(unsigned long long& v, int idx) {
  if constexpr (J >= 1) {
    if constexpr (J < kWave) hy_cmpx<J, KK>(v, idx);
    hy_merge<KK, J / 2>(v, idx);
  }
}

// ascending sort of the 64 keys of a wave (element lane)
__device__ inline void hy_sort64(unsigned long long& v, int lane) {
  hy_merge<2>(v, lane);
  hy_merge<4>(v, lane);
  hy_merge<8>(v, lane);
  hy_merge<16>(v, lane);
  hy_merge<32>(v, lane);
  hy_merge<64>(v, lane);
}

// ascending sort of 128 keys: element lane in v0, element 64 + lane in v1
__device__ inline void hy_sort128(unsigned long long& v0, unsigned long long& v1, int lane) {
  const int hi = kWave + lane;
  hy_merge<2>(v0, lane);
  hy_merge<2>(v1, hi);
  hy_merge<4>(v0, lane);
  hy_merge<4>(v1, hi);
  hy_merge<8>(v0, lane);
  hy_merge<8>(v1, hi);
  hy_merge<16>(v0, lane);
  hy_merge<16>(v1, hi);
  hy_merge<32>(v0, lane);
  hy_merge<32>(v1, hi);
  hy_merge<64>(v0, lane);  // ascending
  hy_merge<64>(v1, hi);    // descending: bit 64 of its index is set
  const unsigned long long a = hy_min(v0, v1), b = hy_max(v0, v1);  // J = 64 of KK = 128
  v0 = a;
  v1 = b;
  hy_merge<128>(v0, lane);  // J = 32 .. 1
  hy_merge<128>(v1, hi);
}

// The candidates of a query: the points of its (up to) nine cell ranges, 64 a
// step; lane r < 9 holds range r in lo_v / hi_v.  f(key, inr) is called by the
// whole wave for every step; inr: the lane holds a point within the radius.
template <typename F>
__device__ inline void hy_sweep(const float4* __restrict__ P, int lo_v, int hi_v, float qx,
                                float qy, float qz, float r2, int n, int lane, F f) {
#pragma unroll 1
  for (int r = 0; r < 9; r++) {
    const int lo = __builtin_amdgcn_readlane(lo_v, r), hi = __builtin_amdgcn_readlane(hi_v, r);
#pragma unroll 1
    for (int p0 = lo; p0 < hi; p0 += kWave) {
      const int p = p0 + lane;
      const bool ok = p < hi;
      const float4 c = P[ok ? p : lo];  // lo < hi <= n
      const float d = pcr_hybrid_dist(qx, qy, qz, c.x, c.y, c.z);
      const int j = min(max(__float_as_int(c.w), 0), n - 1);
      f(pcr_hybrid_key(d, j), ok && pcr_hybrid_in_radius(d, r2));
    }
  }
}

// the same over the wave's buffer of `count` keys, all within the radius
template <typename F>
__device__ inline void hy_sweep_buf(const unsigned long long* buf, int count, int lane, F f) {
#pragma unroll 1
  for (int e0 = 0; e0 < count; e0 += kWave) {
    const int e = e0 + lane;
    const bool ok = e < count;
    f(buf[ok ? e : 0], ok);
  }
}

__global__ __launch_bounds__(kHyWaves* kWave) void hybrid_query_kernel(
    const float* __restrict__ xyz, int n, int k, float r2, int gmax, int ncell,
    const int* __restrict__ meta, const int* __restrict__ cellof, const int* __restrict__ start,
    const float4* __restrict__ pts, float* __restrict__ nbr_dist, int* __restrict__ nbr_idx,
    int* __restrict__ nbr_count, int* __restrict__ within_out) {
  extern __shared__ unsigned long long tile_s[];  // [kHyTile][k | 1] sorted keys per query
  __shared__ unsigned long long buf_s[kHyWaves][kHyCap];
  __shared__ unsigned long long sel_s[kHyWaves][PCR_HYBRID_MAX_K];
  __shared__ int hist_s[kHyWaves][256];
  __shared__ int cnt_s[kHyTile], win_s[kHyTile];
  const int q = blockIdx.y, i0 = blockIdx.x * kHyTile;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int stride = k | 1;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const HyGrid g = hy_grid(meta, q, n, gmax);
  const int nc = g.dx * g.dy * g.dz;
  const float* X = xyz + (size_t)q * 3 * n;
  const int* S = start + (size_t)q * (ncell + 1);
  const float4* P = pts + (size_t)q * n;
  unsigned long long* buf = buf_s[wv];
  unsigned long long* sel = sel_s[wv];
  int* hist = hist_s[wv];
#pragma unroll 1
  for (int ql = wv; ql < kHyTile; ql += kHyWaves) {
    const int i = i0 + ql;
    if (i >= n) break;
    unsigned long long* row = tile_s + ql * stride;
    const int c = cellof[(size_t)q * n + i];
    int within = 0, cnt = 0;
    unsigned long long v0 = PCR_HYBRID_EMPTY, v1 = PCR_HYBRID_EMPTY;
    if (c >= 0) {  // a valid point with finite coordinates
      const float qx = X[i], qy = X[(size_t)n + i], qz = X[2 * (size_t)n + i];
      // lane r < 9: the x-run of cells of row (dy, dz) = (r % 3 - 1, r / 3 - 1)
      int lo_v = 0, hi_v = 0;
      if (lane < 9) {
        const int cc = min(c, nc - 1);
        const int cx = cc % g.dx, cy = (cc / g.dx) % g.dy, cz = cc / (g.dx * g.dy);
        const int yy = cy + lane % 3 - 1, zz = cz + lane / 3 - 1;
        if (yy >= 0 && yy < g.dy && zz >= 0 && zz < g.dz) {
          const int base = g.dx * (yy + g.dy * zz);
          lo_v = min(max(S[base + max(cx - 1, 0)], 0), n);
          hi_v = min(max(S[base + min(cx + 1, g.dx - 1) + 1], lo_v), n);
        }
      }
      // 1. the keys within the radius, compacted; those past the buffer are
      // counted only
      hy_sweep(P, lo_v, hi_v, qx, qy, qz, r2, n, lane, [&](unsigned long long key, bool inr) {
        const unsigned long long bal = __ballot(inr);
        const int pos = within + __popcll(bal & lt);
        if (inr && pos < kHyCap) buf[pos] = key;
        within += __popcll(bal);
      });
      hy_wave_sync();
      const bool fits = within <= kHyCap;
      // 2. with more than k: the k-th smallest key, 8 bits a pass from the top
      unsigned long long thr = ~0ull;
      if (within > k) {
        unsigned long long prefix = 0ull, mask = 0ull;
        int need = k;
#pragma unroll 1
        for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
          for (int u = 0; u < 4; u++) hist[u * kWave + lane] = 0;
          hy_wave_sync();
          auto tally = [&](unsigned long long key, bool inr) {
            if (inr && (key & mask) == prefix) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
          };
          if (fits)
            hy_sweep_buf(buf, within, lane, tally);
          else
            hy_sweep(P, lo_v, hi_v, qx, qy, qz, r2, n, lane, tally);
          hy_wave_sync();
          // lane l holds digits 4 l .. 4 l + 3; the digit where the running
          // count reaches `need`
          int cd[4], sum = 0;
#pragma unroll
          for (int u = 0; u < 4; u++) {
            cd[u] = hist[4 * lane + u];
            sum += cd[u];
          }
          int incl = sum;
#pragma unroll
          for (int off = 1; off < kWave; off <<= 1) {
            const int t = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += t;
          }
          int below = incl - sum, dg = 4 * lane, here = cd[0];
          const bool hit = below < need && need <= incl;
#pragma unroll
          for (int u = 0; u < 3; u++)
            if (dg == 4 * lane + u && below + cd[u] < need) {
              below += cd[u];
              dg++;
              here = cd[u + 1];
            }
          const unsigned long long hb = __ballot(hit);  // one lane: the counts sum to >= need
          const int src = hb ? __ffsll((long long)hb) - 1 : 0;
          dg = __shfl(dg, src, kWave);
          below = __shfl(below, src, kWave);
          here = __shfl(here, src, kWave);
          need -= below;
          prefix |= (unsigned long long)dg << shift;
          mask |= 255ull << shift;
          hy_wave_sync();
          // every key of this digit is among the `need` smallest left: the
          // threshold is the digit's last key, whatever the lower bits hold
          if (here == need) {
            prefix |= (1ull << shift) - 1ull;
            break;
          }
        }
        thr = prefix;
      }
      // 3. the keys up to the threshold: min(within, k) of them
      auto pick = [&](unsigned long long key, bool inr) {
        const bool t = inr && key <= thr;
        const unsigned long long bal = __ballot(t);
        const int pos = cnt + __popcll(bal & lt);
        if (t && pos < PCR_HYBRID_MAX_K) sel[pos] = key;
        cnt += __popcll(bal);
      };
      if (fits)
        hy_sweep_buf(buf, within, lane, pick);
      else
        hy_sweep(P, lo_v, hi_v, qx, qy, qz, r2, n, lane, pick);
      hy_wave_sync();
      cnt = min(cnt, k);
      // 4. sorted in registers
      if (lane < cnt) v0 = sel[lane];
      if (kWave + lane < cnt) v1 = sel[kWave + lane];
      if (cnt > kWave)
        hy_sort128(v0, v1, lane);
      else
        hy_sort64(v0, lane);
    }
    if (lane < k) row[lane] = v0;
    if (kWave + lane < k) row[kWave + lane] = v1;
    if (lane == 0) {
      cnt_s[ql] = cnt;
      win_s[ql] = within;
    }
    hy_wave_sync();  // sel and buf are read before the next query rewrites them
  }
  __syncthreads();
  // the tile leaves slot-major: 32 consecutive points per row segment
  const int ql = tid & (kHyTile - 1), i = i0 + ql;
  if (i < n) {
    for (int s = tid / kHyTile; s < k; s += kHyWaves * kWave / kHyTile) {
      const unsigned long long key = tile_s[ql * stride + s];
      nbr_dist[((size_t)q * k + s) * n + i] = pcr_hybrid_key_dist(key);
      nbr_idx[((size_t)q * k + s) * n + i] = pcr_hybrid_key_index(key);
    }
    if (tid < kHyTile) {
      nbr_count[(size_t)q * n + i] = cnt_s[ql];
      if (within_out) within_out[(size_t)q * n + i] = win_s[ql];
    }
  }
}

}  // namespace pcr

using namespace pcr;

extern "C" size_t pcr_hybrid_search_workspace_size(int b, int n) {
  if (b <= 0 || n <= 0) return 256;
  return hy_ws_layout(b, n, nullptr, nullptr);
}

extern "C" pcr_status pcr_hybrid_search(const float* xyz, const int* counts, int b, int n, int k,
                                        float radius, float* nbr_dist, int* nbr_idx,
                                        int* nbr_count, int* within, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  PCR_REQUIRE(b >= 0, "hybrid_search: negative batch size");
  PCR_REQUIRE(n >= 1, "hybrid_search: n must be at least 1");
  PCR_REQUIRE(k >= 1 && k <= PCR_HYBRID_MAX_K, "hybrid_search: k must be in [1, %d] (got %d)",
              PCR_HYBRID_MAX_K, k);
  PCR_REQUIRE(radius > 0.0f && radius - radius == 0.0f,
              "hybrid_search: radius must be finite and > 0");
  const float r2 = radius * radius;
  PCR_REQUIRE(r2 - r2 == 0.0f, "hybrid_search: radius * radius must be finite");
  if (b == 0) return PCR_OK;
  PCR_REQUIRE((int64_t)b * k * n < (1ll << 31) && b <= 65535, "hybrid_search: batch too large");
  PCR_REQUIRE(xyz && nbr_dist && nbr_idx && nbr_count, "hybrid_search: null pointer");
  HyWs ws;
  const size_t need = hy_ws_layout(b, n, &ws, workspace);
  PCR_REQUIRE(workspace != nullptr && workspace_bytes >= need,
              "hybrid_search: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const int nblocks = min(ceil_div(n, 256), kHyBoundsBlocks);
  const dim3 points(ceil_div(n, 256), b);
  hipLaunchKernelGGL(hybrid_bounds_kernel, dim3(nblocks, b), dim3(256), 0, st, xyz, counts, n,
                     ws.acc);
  hipLaunchKernelGGL(hybrid_setup_kernel, dim3(b), dim3(256), 0, st, ws.acc, counts, nblocks, n,
                     radius, ws.gmax, ws.ncell, ws.meta, ws.hist);
  hipLaunchKernelGGL(hybrid_count_kernel, points, dim3(256), 0, st, xyz, n, ws.gmax, ws.ncell,
                     ws.meta, ws.cellof, ws.hist);
  hipLaunchKernelGGL(hybrid_scan_kernel, dim3(b), dim3(kHyScan), 0, st, n, ws.gmax, ws.ncell,
                     ws.meta, ws.hist, ws.start);
  hipLaunchKernelGGL(hybrid_scatter_kernel, points, dim3(256), 0, st, xyz, n, ws.gmax, ws.ncell,
                     ws.meta, ws.cellof, ws.start, ws.hist, ws.pts);
  const size_t tile_bytes = (size_t)kHyTile * (k | 1) * sizeof(unsigned long long);
  hipLaunchKernelGGL(hybrid_query_kernel, dim3(ceil_div(n, kHyTile), b), dim3(kHyWaves * kWave),
                     tile_bytes, st, xyz, n, k, r2, ws.gmax, ws.ncell, ws.meta, ws.cellof,
                     ws.start, ws.pts, nbr_dist, nbr_idx, nbr_count, within);
  return launch_status("hybrid_search");
}
