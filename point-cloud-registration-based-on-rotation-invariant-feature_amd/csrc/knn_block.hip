// knn_block.hip -- the spatial KNN for 32 < k <= 128 (knn_spatial.hip):
// knn_block_kernel, one wave per 64 consecutive (Morton-sorted) queries,
// top-k per lane in registers as a lexicographically sorted array.
// Candidate blocks are visited outward from the wave's own block; a block
// is skipped when, for every lane, the squared distance to its box
// (computed with the same rounding chain, hence a true lower bound of
// every candidate distance inside) exceeds the lane's current k-th
// distance.  Candidates of a processed block are loaded once (coalesced,
// one per lane) and broadcast with v_readlane.  Because the array is kept
// in (d, index) order, the visiting order cannot change the result.
#include "knn_spatial.hpp"

namespace pcr {

template <int KMAX>
struct TopKKey {
  kkey key[KMAX];
  __device__ void init(int k) {
    const kkey undef = make_key(PCR_KNN_UNDEF, 0);
#pragma unroll
    for (int q = 0; q < KMAX; q++) key[q] = (q < KMAX - k) ? 0.0 : undef;
  }
  __device__ bool qualifies(kkey x) const { return x < key[KMAX - 1]; }
  __device__ float kth() const { return key_dist(key[KMAX - 1]); }
};

__device__ inline void cex_up(kkey& a, kkey& b) {
  const kkey lo = __builtin_fmin(a, b);
  const kkey hi = __builtin_fmax(a, b);
  a = lo;
  b = hi;
}

// Merge a batch of kQ (unsorted) keys into the sorted top-k array: bitonic
// sort of the batch, C[i] = min(A[i], Q[K-1-i]) (the K smallest of A u Q as
// a bitonic sequence), then a bitonic merge.
constexpr int kQ = 8;
template <int KMAX>
__device__ inline void merge_batch(kkey (&key)[KMAX], kkey (&q)[kQ]) {
#pragma unroll
  for (int kk = 2; kk <= kQ; kk <<= 1) {
#pragma unroll
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
#pragma unroll
      for (int i = 0; i < kQ; i++) {
        const int l = i ^ jj;
        if (l > i) {
          if ((i & kk) == 0)
            cex_up(q[i], q[l]);
          else
            cex_up(q[l], q[i]);
        }
      }
    }
  }
#pragma unroll
  for (int i = KMAX - kQ; i < KMAX; i++) key[i] = __builtin_fmin(key[i], q[KMAX - 1 - i]);
#pragma unroll
  for (int jj = KMAX >> 1; jj > 0; jj >>= 1) {
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
      const int l = i ^ jj;
      if (l > i) cex_up(key[i], key[l]);
    }
  }
}

// Waves per query block: the candidate blocks of one 64-query block are
// dealt round-robin to NW waves (more parallelism than one wave per query
// block: B=32 x N=1024 gives only 512 query blocks for 1024 SIMDs), each wave
// keeps its own top-k, and the lists are merged through LDS at the end.
template <int KMAX>
struct KnnNW {
  // waves per query block / waves per workgroup
  static constexpr int value = KMAX <= 32 ? 8 : (KMAX <= 64 ? 2 : 1);
  static constexpr int wg = KMAX <= 32 ? 8 : 4;
};

// r-th block of the visiting order home, home-1, home+1, home-2, ...
__device__ inline int visit_block(int r, int home, int nblk) {
  const int lo = home, hi = nblk - 1 - home;
  const int m2 = lo < hi ? lo : hi;
  if (r == 0) return home;
  if (r <= 2 * m2) {
    const int o = (r + 1) >> 1;
    return (r & 1) ? home - o : home + o;
  }
  const int extra = r - 2 * m2;
  return lo > hi ? home - (m2 + extra) : home + (m2 + extra);
}

template <int KMAX, bool PPF>
__global__ __launch_bounds__(KnnNW<KMAX>::wg * 64) void knn_block_kernel(
    KnnSet qs, KnnSet cs, int k, float* __restrict__ dist, int* __restrict__ idx,
    // fused local PPF: original candidate coords/normals and query normals
    const float* __restrict__ qxyz, const float* __restrict__ qnrm,
    const float* __restrict__ cxyz, const float* __restrict__ cnrm, int relative,
    float* __restrict__ ppf) {
  constexpr int NW = KnnNW<KMAX>::value;
  constexpr int WGW = KnnNW<KMAX>::wg;  // waves per workgroup
  constexpr int QPW = WGW / NW;          // query blocks per workgroup
  // LDS: the per-lane batches (scan phase) and the merge lists (merge / PPF
  // phase) are never live together -> one union
  constexpr int kQBytes = WGW * kQ * kBlk * 8;
  constexpr int kLBytes = NW > 1 ? QPW * (NW / 2) * KMAX * kBlk * 8 : 8;
  __shared__ __align__(16) unsigned char lds_u[kQBytes > kLBytes ? kQBytes : kLBytes];
  kkey* qbuf = (kkey*)lds_u;
  kkey* lst = (kkey*)lds_u;
  __shared__ float thr_s[WGW][kBlk];
  const int b = blockIdx.y;
  const int wv = threadIdx.x >> 6;
  const int w = wv % NW;                       // wave within its query block
  const int qblk = blockIdx.x * QPW + wv / NW;
  const int lane = threadIdx.x & 63;
  const bool live = qblk < qs.nblk;            // wave-uniform
  const size_t qb = (size_t)b * qs.npad + (size_t)(live ? qblk : 0) * kBlk + lane;
  const float qx = qs.x[qb], qy = qs.y[qb], qz = qs.z[qb];
  const int qj = live ? qs.j[qb] : -1;
  TopKKey<KMAX> top;
  top.init(k);
  kkey* myq = qbuf + wv * kQ * kBlk + lane;
  int qn = 0;
  thr_s[wv][lane] = PCR_KNN_UNDEF;
  __syncthreads();
  int nflush = 0, nproc = 0;
  kkey thr_key = top.key[KMAX - 1];
  auto flush = [&]() {
    kkey qv[kQ];
#pragma unroll
    for (int s = 0; s < kQ; s++) qv[s] = myq[s * kBlk];
#pragma unroll
    for (int s = 0; s < kQ; s++) qv[s] = s < qn ? qv[s] : PCR_KEY_PAD;
    merge_batch<KMAX>(top.key, qv);
    qn = 0;
    nflush++;
    thr_s[wv][lane] = top.kth();  // publish: an upper bound of the final k-th
    thr_key = __builtin_fmin(thr_key, top.key[KMAX - 1]);
  };
  const int gbase = wv - w;  // first wave of this query block
  const float* boxes = cs.box + (size_t)b * cs.nblk * 8;
  const size_t cbase = (size_t)b * cs.npad;
  int home = (int)(((long long)(live ? qblk : 0) * cs.nblk) / qs.nblk);
  if (home >= cs.nblk) home = cs.nblk - 1;
  auto scan_block = [&](int blk) {
    // best bound known to any wave of this query block
    float thr = top.kth();
#pragma unroll
    for (int o = 0; o < NW; o++) thr = fminf(thr, thr_s[gbase + o][lane]);
    // one key bound: below this wave's k-th key and at most the best k-th
    // distance any wave of the query block has published
    thr_key = __builtin_fmin(top.key[KMAX - 1],
                             __longlong_as_double((long long)(((unsigned long long)
                                 __float_as_uint(thr) << 32) | 0xFFFFFFFFull)));
    const float lb = box_lb(qx, qy, qz, boxes + (size_t)blk * 8);
    if (!__any(lb <= thr)) return;  // no lane can gain from this block
    const size_t cp = cbase + (size_t)blk * kBlk + lane;
    const float cx = cs.x[cp], cy = cs.y[cp], cz = cs.z[cp];
    const int cj = cs.j[cp];
    nproc++;
    for (int t = 0; t < kBlk; t += 2) {
      if (__any(qn > kQ - 2)) flush();
      const float sx0 = readlane_f(cx, t), sy0 = readlane_f(cy, t), sz0 = readlane_f(cz, t);
      const float sx1 = readlane_f(cx, t + 1), sy1 = readlane_f(cy, t + 1),
                  sz1 = readlane_f(cz, t + 1);
      const int sj0 = __builtin_amdgcn_readlane(cj, t);
      const int sj1 = __builtin_amdgcn_readlane(cj, t + 1);
      const float a0 = qx - sx0, b0 = qy - sy0, c0 = qz - sz0;
      const float a1 = qx - sx1, b1 = qy - sy1, c1 = qz - sz1;
      float d0 = a0 * a0, d1 = a1 * a1;
      d0 = __builtin_fmaf(b0, b0, d0);
      d1 = __builtin_fmaf(b1, b1, d1);
      d0 = __builtin_fmaf(c0, c0, d0);
      d1 = __builtin_fmaf(c1, c1, d1);
      const kkey k0 = make_key(d0, sj0), k1 = make_key(d1, sj1);
      // keys above this wave's (stale) k-th, or farther than another wave's
      // k-th distance, can never reach the final list.  Branch-free append:
      // slot qn is free (flushed above when fewer than 2 are left).
      myq[qn * kBlk] = k0;
      qn += k0 < thr_key ? 1 : 0;
      myq[qn * kBlk] = k1;
      qn += k1 < thr_key ? 1 : 0;
    }
  };
  // warm-up: wave 0 alone scans the home block and publishes its k-th
  // distance, so the other waves start with a tight bound instead of each
  // filling a list of its own from scratch
  if (live && w == 0) {
    scan_block(home);
    if (__any(qn > 0)) flush();
  }
  if (NW > 1) __syncthreads();
  if (live) {
    for (int rr = (w == 0 ? NW : w); rr < cs.nblk; rr += NW) scan_block(visit_block(rr, home, cs.nblk));
    if (__any(qn > 0)) flush();
  }
  (void)nflush;
  (void)nproc;
  // merge the NW lists of a query block: tree of bitonic merges through LDS.
  // The partner's k-k front sentinels (key 0) must not enter the result:
  // they read as +inf.
  const int base = KMAX - k;
#pragma unroll
  for (int half = NW / 2; half >= 1; half >>= 1) {
    __syncthreads();
    if (live && w >= half && w < 2 * half) {
      kkey* dst = lst + (size_t)((wv / NW) * (NW / 2) + (w - half)) * KMAX * kBlk;
#pragma unroll
      for (int s = 0; s < KMAX; s++) dst[s * kBlk + lane] = top.key[s];
    }
    __syncthreads();
    if (live && w < half) {
      const kkey* src = lst + (size_t)((wv / NW) * (NW / 2) + w) * KMAX * kBlk;
      // C[i] = min(A[i], B[K-1-i]) then bitonic merge
#pragma unroll
      for (int i = 0; i < KMAX; i++) {
        // partner's reals ascending then padding: B''[t] = B[base + t] (t < k)
        const kkey o = i >= base ? src[(base + KMAX - 1 - i) * kBlk + lane] : PCR_KEY_PAD;
        top.key[i] = __builtin_fmin(top.key[i], o);
      }
#pragma unroll
      for (int jj = KMAX >> 1; jj > 0; jj >>= 1) {
#pragma unroll
        for (int i = 0; i < KMAX; i++) {
          const int l = i ^ jj;
          if (l > i) cex_up(top.key[i], top.key[l]);
        }
      }
    }
  }
  const int n = qs.n;
  if (live && w == 0 && qj >= 0) {
#pragma unroll
    for (int s = 0; s < KMAX; s++) {
      if (s >= base) {
        const size_t o = ((size_t)b * k + (s - base)) * n + qj;
        if (dist) dist[o] = key_dist(top.key[s]);
        idx[o] = key_idx(top.key[s]);
      }
    }
  }
  if (PPF) {
    // every wave of the query block takes a share of the slots
    kkey* fin = lst + (size_t)(wv / NW) * KMAX * kBlk;
    if (NW > 1) {
      __syncthreads();  // merge reads of lst are complete
      if (live && w == 0) {
#pragma unroll
        for (int s = 0; s < KMAX; s++) fin[s * kBlk + lane] = top.key[s];
      }
      __syncthreads();
    }
    if (!live || qj < 0) return;
    const int m = cs.n;
    const float* cb = cxyz + (size_t)b * 3 * m;
    const float* nb = cnrm + (size_t)b * 3 * m;
    const float* qnr = qnrm + (size_t)b * 3 * n;
    const float* qo = qxyz + (size_t)b * 3 * n;
    const float ox = qo[qj], oy = qo[qj + n], oz = qo[qj + 2 * n];
    const float cnx = qnr[qj], cny = qnr[qj + n], cnz = qnr[qj + 2 * n];
#pragma unroll 1
    for (int slot = w; slot < k; slot += NW) {
      const int jn = NW > 1 ? key_idx(fin[(base + slot) * kBlk + lane])
                            : idx[((size_t)b * k + slot) * n + qj];
      float o[4];
      pcr_local_ppf(ox, oy, oz, cnx, cny, cnz, cb[jn], cb[jn + m], cb[jn + 2 * m], nb[jn],
                    nb[jn + m], nb[jn + 2 * m], relative, o);
#pragma unroll
      for (int ch = 0; ch < 4; ch++) ppf[(((size_t)b * 4 + ch) * k + slot) * n + qj] = o[ch];
    }
  }
}

template <int KM, bool PPF>
static void launch_block_km(const KnnSet& qs, const KnnSet& cs, int b, int k, const KnnDir& d,
                            hipStream_t st) {
  const dim3 grid(ceil_div(qs.nblk, KnnNW<KM>::wg / KnnNW<KM>::value), b);
  hipLaunchKernelGGL((knn_block_kernel<KM, PPF>), grid, dim3(KnnNW<KM>::wg * 64), 0, st, qs, cs, k,
                     d.dist, d.idx, d.qxyz, d.qnrm, d.cxyz, d.cnrm, d.relative, d.ppf);
}

// Smaller k never gets here (the selection takes every k <= 32), so the
// kernel exists for lists of 64 and 128 keys only.
void launch_block_kernel(const KnnSet& qs, const KnnSet& cs, int b, int k, const KnnDir& d,
                         hipStream_t st, bool ppf) {
  if (k <= 64) {
    if (ppf) launch_block_km<64, true>(qs, cs, b, k, d, st);
    else launch_block_km<64, false>(qs, cs, b, k, d, st);
  } else {
    if (ppf) launch_block_km<128, true>(qs, cs, b, k, d, st);
    else launch_block_km<128, false>(qs, cs, b, k, d, st);
  }
}

}  // namespace pcr
