// knn_spatial.hip -- exact k-nearest-neighbour search with spatial pruning,
// for gfx950.  Same results as knn/knn.cu:5-49 of the reference (k
// lexicographically smallest (squared distance, index) pairs with distance
// < 10000, squared distance with the reference's FMA contraction, unfilled
// slots (10000, 0)), but sub-quadratic in practice:
//
//  1. knn_sort_kernel -- one workgroup per (cloud, point set): 30-bit Morton
//     code of every point in the cloud's bounding box, LDS bitonic sort of
//     (code, index), then the sorted SoA coordinates + original indices and
//     the axis-aligned box of every 64-point block.
//  2. the neighbours of every query from the sorted sets, by one of three
//     kernel families (launch_block below): the threshold selection
//     (knn_select_kernel, this file) for k <= 32 and, on clouds of more than
//     1024 points, k <= 64; the per-lane top-k lists (knn_block.hip) for every
//     other k <= 128; and, for the runner's sorted-rows stage on clouds of
//     <= 1024 points, the transposed selection (knn_wsel.hip).
#include "knn_spatial.hpp"

namespace pcr {

constexpr int kKnnMaxN = 1 << 22;         // global counting sort beyond

// ---------------------------------------------------------------------------
// knn_select_kernel (k <= 32): threshold selection instead of per-wave top-k
// lists.  One workgroup of NW waves serves 64 Morton-consecutive queries (one
// per lane); the candidate blocks are dealt round-robin to the waves.  At
// N = 1024 no block can be skipped for a whole 64-query block (the 64 k-NN
// balls cover most of the cloud), so every pass is a brute-force sweep over
// the candidates, two per packed-fp32 instruction.  Clouds of <= kSelCache
// points are staged in LDS once per workgroup and read as broadcast
// ds_read_b128 (in-order LDS returns: no scalar-load round trip in the
// loop); larger ones are read through scalar loads.
//
//  1. bound   D_q = min over candidate blocks holding >= k points of the
//             largest distance from q to the block's box (the same rounding
//             chain, so >= every candidate distance in it): at least k
//             candidates lie within D_q, hence kth(q) <= D_q.
//  2. count   histogram of every candidate distance in quarter-octave bins
//             of d (float bits >> 21) over the kNB bins ending at D_q's bin
//             (bin 0 takes everything below).  One LDS counter per (bin,
//             lane) holds CB-bit fields, one per wave, so the same no-return
//             atomics also give every wave its own counts.
//  3. cut     first bin where the running count reaches k: every candidate
//             with bits >> 21 <= that bin is collected (~1.2-1.9 k for
//             smooth clouds, kCap slots per query).  A wave's slot base is
//             the count of the waves before it, read from the fields.
//  4. collect one sweep writes the (d, index) keys of the collected
//             candidates into the wave's slots.
//  5. rank    the keys are unique; each wave ranks its share of them against
//             all; a key of rank r < k is output slot r.  Every wave then
//             writes k / NW slots and their local PPF (neighbour loads issued
//             for all its slots before any arithmetic).
// A query block where some query has no finite bound below 10000 (fewer than
// k points, NaN / huge coordinates) or more than kCap collected keys
// (duplicates, extreme clustering) takes the exact fallback: wave 0 runs the
// reference's insertion scan with the list in LDS.  Both paths give the
// reference's result: the k lexicographically smallest (d, index) with
// d < 10000, unfilled slots (10000, 0).
constexpr int kNB = 24;
constexpr int kCap = 88;
constexpr int kSelCache = 1024;  // candidates staged in LDS per workgroup
constexpr int kSelMaxK = 32;
constexpr int kCap64 = 112;  // the same selection for 32 < k <= 64 (large clouds): two workgroups per CU
constexpr int kSelMaxK64 = 64;

typedef float pf2 __attribute__((ext_vector_type(2)));

// clamp to [lo, hi] in one instruction (the compiler emits min + max)
__device__ inline int med3_i32(int x, int lo, int hi) {
  int r;
  asm volatile("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(lo), "v"(hi));
  return r;
}

__device__ inline float cand_dist(float qx, float qy, float qz, float sx, float sy, float sz) {
  const float a = qx - sx, bq = qy - sy, c = qz - sz;
  float d = a * a;
  d = __builtin_fmaf(bq, bq, d);
  d = __builtin_fmaf(c, c, d);
  return d;
}

// two candidates at once (v_pk_add / v_pk_mul / v_pk_fma_f32); per element
// the same operations and roundings as cand_dist
__device__ inline pf2 cand_dist2(pf2 qx, pf2 qy, pf2 qz, pf2 sx, pf2 sy, pf2 sz) {
  const pf2 a = qx - sx, bq = qy - sy, c = qz - sz;
  pf2 d = a * a;
  d = __builtin_elementwise_fma(bq, bq, d);
  d = __builtin_elementwise_fma(c, c, d);
  return d;
}

template <int CB>
__device__ inline unsigned field_sum(unsigned v) {
  if (CB == 8) {
    v = (v & 0x00FF00FFu) + ((v >> 8) & 0x00FF00FFu);
    return (v & 0xFFFFu) + (v >> 16);
  }
  return (v & 0xFFFFu) + (v >> 16);
}

template <int NW, int CB, bool CL, bool PPF, int CAP = kCap, int KSEL = kSelMaxK,
          int CACHE = kSelCache>
__global__ __launch_bounds__(NW * 64) void knn_select_kernel(
    KnnSet qs, KnnSet cs, int k, float* __restrict__ dist, int* __restrict__ idx,
    const float* __restrict__ qxyz, const float* __restrict__ qnrm,
    const float* __restrict__ cxyz, const float* __restrict__ cnrm, int relative,
    float* __restrict__ ppf, int sorted_emit) {
  constexpr int FPD = 32 / CB;              // wave fields per counter dword
  constexpr int NG = (NW + FPD - 1) / FPD;  // counter dwords per (bin, lane)
  // the histogram is dead once the cut is chosen: the collected keys reuse it
  constexpr int kHistBytes = NG * (kNB + 1) * kBlk * 4;
  constexpr int kBufBytes = (CAP + 1) * kBlk * 8;  // row CAP: sink of masked writes
  __shared__ __align__(16) unsigned char sel_u[kHistBytes > kBufBytes ? kHistBytes : kBufBytes];
  unsigned* hist_s = (unsigned*)sel_u;
  kkey* buf_s = (kkey*)sel_u;
  __shared__ unsigned dest_s[kBlk];
  __shared__ unsigned cut_s[2 + 2 * NG][kBlk];  // wave 0's cut: bin, count, wave fields (cut, below)
  // cached clouds: the Morton-sorted candidates (the near ones of a query
  // block cluster in a few groups, so few groups are collected) and their
  // point ids as u16, read with the coordinates: the collect pass never
  // waits on an LDS read inside its sweep
  __shared__ __align__(16) float cand_s[CL ? 3 * CACHE : 4];  // x | y | z
  __shared__ __align__(16) unsigned short cand_j[CL ? CACHE : 8];
  __shared__ __align__(16) float cand_w[CL ? 1 : NW][CL ? 4 : 3 * kBlk];  // a block per wave
  (void)PCR_PRIO(1);
  const int b = blockIdx.y;
  const int qblk = blockIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const size_t qb = (size_t)b * qs.npad + (size_t)qblk * kBlk + lane;
  const float qx = qs.x[qb], qy = qs.y[qb], qz = qs.z[qb];
  const int qj = qs.j[qb];
  const bool qlive = qj >= 0;
  const int m = cs.n;
  const int nblk = cs.nblk;
  const float* boxes = cs.box + (size_t)b * nblk * 8;
  const size_t cbase = (size_t)b * cs.npad;
  const pf2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};

  for (int i = threadIdx.x; i < NG * (kNB + 1) * kBlk; i += NW * kBlk) hist_s[i] = 0u;
  if (wv == 0) dest_s[lane] = 0x7F800000u;  // +inf
  if (CL) {
    const int np = cs.npad;
    for (int i = threadIdx.x; i < np; i += NW * kBlk) {
      cand_s[i] = cs.x[cbase + i];
      cand_j[i] = (unsigned short)cs.j[cbase + i];
      cand_s[CACHE + i] = cs.y[cbase + i];
      cand_s[2 * CACHE + i] = cs.z[cbase + i];
    }
  }
  // Visit every group of four candidates this wave owns: f(pos, d[4]), pos =
  // sorted position of the group's first candidate.  Cached clouds: wave w
  // owns candidates [64 b + w S, 64 b + w S + S) of every block b (S = 64 /
  // NW), so the candidates near the queries -- the ones the collect pass
  // keeps -- are spread over all waves; no pruning (at <= CACHE points a
  // 64-query block reaches nearly every candidate block).  The next group's
  // LDS reads are issued before f runs, so their wait never covers the LDS
  // atomics / stores f issues.  Larger clouds: whole blocks round-robin over
  // the waves, skipped when no lane's box distance is below `lim`.
  int nvisit = 0;  // candidate blocks this wave processed (diagnostics)
  // Large clouds: the boxes of this wave's blocks (wv + NW (64 j + lane)) sit
  // in registers and reach the whole wave by v_readlane, so the per-block
  // tests never wait on memory; a processed block is loaded one candidate
  // per lane (coalesced) into the wave's LDS slot and read back as
  // broadcast ds_read_b128, as the cached path does.
  constexpr int kBoxJ = 2;
  const bool breg = !CL && nblk <= NW * kBlk * kBoxJ;
  float bl[kBoxJ][6];
#pragma unroll
  for (int j = 0; j < kBoxJ; j++) {
    const int blk = wv + NW * (j * kBlk + lane);
    const bool ok = breg && blk < nblk;
#pragma unroll
    for (int a = 0; a < 6; a++) bl[j][a] = ok ? boxes[(size_t)blk * 8 + a] : 0.0f;
  }
  // the query block's box (scalar loads; the register-box sweep's prefilter)
  float qbx[6];
#pragma unroll
  for (int a = 0; a < 6; a++)
    qbx[a] = breg ? qs.box[((size_t)b * qs.nblk + qblk) * 8 + a] : 0.0f;
  // visits this wave's blocks in order: g(blk, box[6]) (register boxes only)
  auto for_blocks = [&](auto&& g) {
#pragma unroll
    for (int j = 0; j < kBoxJ; j++) {
      for (int l = 0; l < kBlk; l++) {
        const int blk = wv + NW * (j * kBlk + l);
        if (blk >= nblk) return;
        float b6[6];
#pragma unroll
        for (int a = 0; a < 6; a++) b6[a] = readlane_f(bl[j][a], l);
        g(blk, b6);
      }
    }
  };
  int cj_cur = 0;  // original index of candidate `lane` of the block in process
  // register-box path: blocks a count round already visited (excluded from
  // the next round) and whether this visit records its blocks there
  unsigned long long vskip[kBoxJ];
#pragma unroll
  for (int j = 0; j < kBoxJ; j++) vskip[j] = 0ull;
  bool vrecord = false;
  auto visit = [&](float lim, auto want_j, auto&& f) {
    constexpr bool WANT_J = decltype(want_j)::value;
    if (CL) {
      constexpr int S = kBlk / NW;
      constexpr int GPB = S / 4;
      static_assert(S % 4 == 0, "a wave owns whole groups of four");
      static_assert(GPB == 2, "two groups of four per wave and block");
      // one block (two groups) per half iteration; positions advance by a
      // constant, so every read is one base register plus an immediate.
      // Reads past the last block land in the next LDS array (never used).
      // the ids of the wave's 8 candidates (u16) are read with them only
      // when the callback uses them (the collect pass)
      auto rd = [&](int o, float4 (&X)[2], float4 (&Y)[2], float4 (&Z)[2], uint4& J) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
          X[h] = *(const float4*)(cand_s + o + 4 * h);
          Y[h] = *(const float4*)(cand_s + CACHE + o + 4 * h);
          Z[h] = *(const float4*)(cand_s + 2 * CACHE + o + 4 * h);
        }
        if (WANT_J) J = *(const uint4*)(cand_j + o);
      };
      auto eval = [&](int o, const float4 (&X)[2], const float4 (&Y)[2], const float4 (&Z)[2],
                      const uint4& J) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const pf2 d0 = cand_dist2(qx2, qy2, qz2, pf2{X[h].x, X[h].y}, pf2{Y[h].x, Y[h].y},
                                    pf2{Z[h].x, Z[h].y});
          const pf2 d1 = cand_dist2(qx2, qy2, qz2, pf2{X[h].z, X[h].w}, pf2{Y[h].z, Y[h].w},
                                    pf2{Z[h].z, Z[h].w});
          const float d[4] = {d0[0], d0[1], d1[0], d1[1]};
          f(o + 4 * h, d, h == 0 ? uint2{J.x, J.y} : uint2{J.z, J.w});
        }
      };
      // ping-pong register sets A / B, no copies: B's reads are issued
      // before A's evaluation (and its LDS atomics / stores) and vice versa
      float4 AX[2], AY[2], AZ[2], BX[2], BY[2], BZ[2];
      uint4 AJ = {0u, 0u, 0u, 0u}, BJ = {0u, 0u, 0u, 0u};
      int o = wv * S;
      rd(o, AX, AY, AZ, AJ);
      for (int blk = 0; blk < nblk; blk += 2, o += 2 * kBlk) {
        rd(o + kBlk, BX, BY, BZ, BJ);
        __builtin_amdgcn_sched_barrier(0);  // reads first, then A's (older) data is waited on
        eval(o, AX, AY, AZ, AJ);
        rd(o + 2 * kBlk, AX, AY, AZ, AJ);
        __builtin_amdgcn_sched_barrier(0);
        if (blk + 1 < nblk) eval(o + kBlk, BX, BY, BZ, BJ);
      }
    } else if (breg) {
      // which of this wave's blocks does any query lane need?  Lane l tests
      // block wv + NW (64 j + l) against the 64 queries (read by v_readlane):
      // one ballot per 64 blocks instead of one box test + ballot per block
      // (up to 64 blocks per wave, i.e. clouds of <= 32k points: one box
      // test + ballot per block is cheaper than the 64-query sweep)
      unsigned long long vm[kBoxJ];
      if (nblk <= NW * kBlk) {
        vm[0] = 0ull;
#pragma unroll
        for (int j = 1; j < kBoxJ; j++) vm[j] = 0ull;
        for (int l = 0; wv + NW * l < nblk; l++) {
          float b6[6];
#pragma unroll
          for (int a = 0; a < 6; a++) b6[a] = readlane_f(bl[0][a], l);
          if (__any(box_lb(qx, qy, qz, b6) < lim)) vm[0] |= 1ull << l;
        }
      } else {
        // lane l tests block wv + NW (64 j + l) against the box of the
        // query block with the largest limit of its queries (the same
        // rounding chain, so it is a lower bound of every query's box
        // distance: a block failing it is needed by no query); only the
        // blocks passing it get the per-query test (one box test + ballot
        // each), instead of a sweep of all 64 queries for every block
        float mlim = lim;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mlim = fmaxf(mlim, __shfl_xor(mlim, off, kWave));
#pragma unroll
        for (int j = 0; j < kBoxJ; j++) {
          const float gx = fmaxf(fmaxf(bl[j][0] - qbx[3], qbx[0] - bl[j][3]), 0.0f);
          const float gy = fmaxf(fmaxf(bl[j][1] - qbx[4], qbx[1] - bl[j][4]), 0.0f);
          const float gz = fmaxf(fmaxf(bl[j][2] - qbx[5], qbx[2] - bl[j][5]), 0.0f);
          float bb = gx * gx;
          bb = __builtin_fmaf(gy, gy, bb);
          bb = __builtin_fmaf(gz, gz, bb);
          unsigned long long cand =
              __ballot(bb < mlim && wv + NW * (j * kBlk + lane) < nblk);
          vm[j] = 0ull;
          while (cand) {
            const int l = __builtin_ctzll(cand);
            cand &= cand - 1ull;
            float b6[6];
#pragma unroll
            for (int a = 0; a < 6; a++) b6[a] = readlane_f(bl[j][a], l);
            if (__any(box_lb(qx, qy, qz, b6) < lim)) vm[j] |= 1ull << l;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kBoxJ; j++) {
        vm[j] &= ~vskip[j];
        if (vrecord) vskip[j] |= vm[j];
      }
      // the visited blocks in order, the next one's candidates loaded (one
      // per lane) while the current one is evaluated from the wave's LDS slot
      int jc = 0;
      auto next = [&]() {
        while (jc < kBoxJ && vm[jc] == 0ull) jc++;
        if (jc >= kBoxJ) return -1;
        const int l = __builtin_ctzll(vm[jc]);
        vm[jc] &= vm[jc] - 1ull;
        return wv + NW * (jc * kBlk + l);
      };
      float* cw = cand_w[CL ? 0 : wv];
      int cur = next();
      float px = 0.0f, py = 0.0f, pz = 0.0f;
      int pj = 0;
      if (cur >= 0) {
        const size_t cp = cbase + (size_t)cur * kBlk + lane;
        px = cs.x[cp];
        py = cs.y[cp];
        pz = cs.z[cp];
        pj = cs.j[cp];
      }
      while (cur >= 0) {
        nvisit++;
        const int nxt = next();
        // the wave's previous block is fully read (LDS is in order per wave)
        cw[lane] = px;
        cw[kBlk + lane] = py;
        cw[2 * kBlk + lane] = pz;
        cj_cur = pj;
        if (nxt >= 0) {
          const size_t cp = cbase + (size_t)nxt * kBlk + lane;
          px = cs.x[cp];
          py = cs.y[cp];
          pz = cs.z[cp];
          pj = cs.j[cp];
        }
        // ping-pong register sets: the next group's LDS reads are issued
        // before this group's callback (its LDS atomics / stores), so its
        // wait never covers them (LDS operations complete in order)
        auto rd4 = [&](int t, float4& X, float4& Y, float4& Z) __attribute__((always_inline)) {
          X = *(const float4*)(cw + t);
          Y = *(const float4*)(cw + kBlk + t);
          Z = *(const float4*)(cw + 2 * kBlk + t);
        };
        auto ev4 = [&](int t, const float4& X, const float4& Y, const float4& Z)
                       __attribute__((always_inline)) {
          const pf2 d0 = cand_dist2(qx2, qy2, qz2, pf2{X.x, X.y}, pf2{Y.x, Y.y}, pf2{Z.x, Z.y});
          const pf2 d1 = cand_dist2(qx2, qy2, qz2, pf2{X.z, X.w}, pf2{Y.z, Y.w}, pf2{Z.z, Z.w});
          const float d[4] = {d0[0], d0[1], d1[0], d1[1]};
          f(cur * kBlk + t, d, uint2{0u, 0u});
        };
        float4 AX, AY, AZ, BX, BY, BZ;
        rd4(0, AX, AY, AZ);
#pragma unroll 2
        for (int t = 0; t < kBlk; t += 8) {
          rd4(t + 4, BX, BY, BZ);
          __builtin_amdgcn_sched_barrier(0);
          ev4(t, AX, AY, AZ);
          if (t + 8 < kBlk) rd4(t + 8, AX, AY, AZ);
          __builtin_amdgcn_sched_barrier(0);
          ev4(t + 4, BX, BY, BZ);
        }
        cur = nxt;
      }
    } else {
      for (int blk = wv; blk < nblk; blk += NW) {
        if (!__any(box_lb(qx, qy, qz, boxes + (size_t)blk * 8) < lim)) continue;
        nvisit++;
        const float* bx = cs.x + cbase + (size_t)blk * kBlk;
        const float* by = cs.y + cbase + (size_t)blk * kBlk;
        const float* bz = cs.z + cbase + (size_t)blk * kBlk;
#pragma unroll 4
        for (int t = 0; t < kBlk; t += 4) {
          const float4 X = *(const float4*)(bx + t);
          const float4 Y = *(const float4*)(by + t);
          const float4 Z = *(const float4*)(bz + t);
          const pf2 d0 = cand_dist2(qx2, qy2, qz2, pf2{X.x, X.y}, pf2{Y.x, Y.y}, pf2{Z.x, Z.y});
          const pf2 d1 = cand_dist2(qx2, qy2, qz2, pf2{X.z, X.w}, pf2{Y.z, Y.w}, pf2{Z.z, Z.w});
          const float d[4] = {d0[0], d0[1], d1[0], d1[1]};
          f(blk * kBlk + t, d, uint2{0u, 0u});
        }
      }
    }
  };
  // original indices of the four candidates at sorted position pos
  auto cand_idx4 = [&](int pos) {
    if (CL) return int4{0, 0, 0, 0};  // unused: the cached path passes its ids to the callback
    if (breg) {
      const int t = pos & (kBlk - 1);
      return int4{__builtin_amdgcn_readlane(cj_cur, t), __builtin_amdgcn_readlane(cj_cur, t + 1),
                  __builtin_amdgcn_readlane(cj_cur, t + 2),
                  __builtin_amdgcn_readlane(cj_cur, t + 3)};
    }
    const int* bj = cs.j + cbase + pos;
    return int4{bj[0], bj[1], bj[2], bj[3]};
  };
  __syncthreads();

  // 1. bound
  {
    float dq = __builtin_inff();
    // a self KNN over many blocks takes its bound from the blocks within
    // kBoundWin of the query block in Morton order (any block of >= k points
    // bounds kth, so fewer blocks only loosen the bound; the box nearest a
    // query is almost always there): the boxes are read by scalar loads, not
    // one readlane sweep over all of this wave's blocks
    constexpr int kBoundWin = 64;
    if (!CL && qs.x == cs.x && nblk > 2 * kBoundWin + NW && breg) {
      // the window's boxes of this wave are lanes [l0, l1] of its register
      // boxes (block wv + NW (64 j + l)): v_readlane, no scalar-load chain
      const int lo = max(0, qblk - kBoundWin), hi = min(nblk - 1, qblk + kBoundWin);
#pragma unroll
      for (int j = 0; j < kBoxJ; j++) {
        const int f0 = lo - wv - NW * j * kBlk, f1 = hi - wv - NW * j * kBlk;
        const int l0 = max(0, (f0 + NW - 1 + NW * kBlk) / NW - kBlk), l1 = min(kBlk - 1, f1 >= 0 ? f1 / NW : -1);
        for (int l = l0; l <= l1; l++) {
          const int blk = wv + NW * (j * kBlk + l);
          float b6[6];
#pragma unroll
          for (int a = 0; a < 6; a++) b6[a] = readlane_f(bl[j][a], l);
          if (min(kBlk, m - blk * kBlk) >= k) dq = fminf(dq, box_ub(qx, qy, qz, b6));
        }
      }
    } else if (!CL && qs.x == cs.x && nblk > 2 * kBoundWin + NW) {
      const int lo = max(0, qblk - kBoundWin), hi = min(nblk - 1, qblk + kBoundWin);
      for (int blk = lo + wv; blk <= hi; blk += NW) {
        const int real = min(kBlk, m - blk * kBlk);
        if (real >= k) dq = fminf(dq, box_ub(qx, qy, qz, boxes + (size_t)blk * 8));
      }
    } else if (breg) {
      for_blocks([&](int blk, const float (&b6)[6]) {
        const int real = min(kBlk, m - blk * kBlk);
        if (real >= k) dq = fminf(dq, box_ub(qx, qy, qz, b6));
      });
    } else {
      for (int blk = wv; blk < nblk; blk += NW) {
        const int real = min(kBlk, m - blk * kBlk);
        if (real >= k) dq = fminf(dq, box_ub(qx, qy, qz, boxes + (size_t)blk * 8));
      }
    }
    atomicMin(&dest_s[lane], __float_as_uint(dq));  // NaN never wins: fminf drops it
  }
  __syncthreads();
  const unsigned dbits = dest_s[lane];
  bool fallback = __any(qlive && !(dbits < __float_as_uint(PCR_KNN_UNDEF)));
  const int etop = (int)(dbits >> 21);
  const int ebase = etop - (kNB - 1);
  // smallest distance that is not counted (0 for padding lanes: they never
  // keep a block alive)
  const float ftop = (qlive && !fallback) ? __uint_as_float((unsigned)(etop + 1) << 21) : 0.0f;

  // 2. count + 3. cut.  Pass 1 counts quarter-octave bins (float bits >> 21)
  // of the kNB below D_q's bin.  A block where some query has more than CAP
  // keys at its cut (a bin of many near-equal distances: an outlier facing
  // the bulk of the cloud) recounts inside each query's cut bin with
  // 1/64-octave bins (bits >> 17) before it gives up to the insertion
  // fallback.  Every wave computes the same cut for its 64 queries.
  // total: keys at or below the cut bin; lo_total (S): keys below it (all of
  // them are among the k nearest); slot / slot_lo: this wave's first slot
  // among all / the below-cut keys of the lane
  int total = 0, slot = 0, bstar = -1, lo_total = 0, slot_lo = 0;
  int shift = 21, base = ebase;
  unsigned ucut = 0u, ulo = 0u;
  auto count_visit = [&](float lim) {
    unsigned* hw = hist_s + (size_t)(wv / FPD) * (kNB + 1) * kBlk + lane;
    const unsigned inc = 1u << ((wv % FPD) * CB);
    // counter of bin e (clamped to [base, base + kNB]; the last = not
    // counted, also NaN) at hwb + e * kBlk
    unsigned* hwb = hw - base * kBlk;
    const int top = base + kNB;
    const int sh = shift;
    visit(lim, std::false_type(), [&](int, const float (&d)[4], uint2) {
#pragma unroll
      for (int h = 0; h < 4; h++) {
        const int e = med3_i32((int)(__float_as_uint(d[h]) >> sh), base, top);
        __hip_atomic_fetch_add(hwb + e * kBlk, inc, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    });
  };
  // upper edge of the first bin where the lane's count so far reaches k
  // (every count is a real candidate, so kth(q) lies below it), else `lim`
  auto running_cut = [&](float lim) {
    int cum = 0;
    float t = lim;
    bool found = false;
    for (int bin = 0; bin < kNB; bin++) {
#pragma unroll
      for (int g = 0; g < NG; g++) cum += (int)field_sum<CB>(hist_s[(g * (kNB + 1) + bin) * kBlk + lane]);
      if (!found && cum >= k) {
        found = true;
        t = __uint_as_float((unsigned)(base + bin + 1) << shift);
      }
      if (__all(found)) break;
    }
    return fminf(t, lim);
  };
  auto count_cut = [&](float lim) {
    if (!CL && breg) {
      // large clouds: two rounds.  D_q is several times kth (its bin top
      // reaches past most of the cloud's near blocks), so the blocks near
      // the queries (lower bound below D_q / 8) are counted first; their
      // counts give each query an upper bound of kth (the first bin where
      // the count reaches k), and the second round adds only the blocks
      // below that tighter bound.  Every block a query may need is still
      // counted for it: an unvisited block has every lane's lower bound at
      // or above that lane's limit, and the final cut never exceeds it.
      vrecord = true;
      count_visit(lim * 0.125f);
      vrecord = false;
      __syncthreads();
      count_visit(qlive ? running_cut(lim) : 0.0f);
#pragma unroll
      for (int j = 0; j < kBoxJ; j++) vskip[j] = 0ull;
    } else {
      count_visit(lim);
    }
    __syncthreads();
    // wave 0 finds the cut of the 64 queries (the other waves would repeat
    // the same sweep) and hands it over through LDS
    unsigned cum[NG], cut[NG], cutb[NG];
#pragma unroll
    for (int g = 0; g < NG; g++) cum[g] = cut[g] = cutb[g] = 0u;
    if (wv == 0) {
      bstar = -1;
      total = 0;
      for (int b0 = 0; b0 < kNB; b0 += 4) {
#pragma unroll
        for (int bin = b0; bin < b0 + 4; bin++) {
          unsigned prev[NG];
          int tb = 0;
#pragma unroll
          for (int g = 0; g < NG; g++) {
            prev[g] = cum[g];
            cum[g] += hist_s[(g * (kNB + 1) + bin) * kBlk + lane];
            tb += (int)field_sum<CB>(cum[g]);
          }
          if (bstar < 0 && tb >= k) {
            bstar = bin;
            total = tb;
#pragma unroll
            for (int g = 0; g < NG; g++) {
              cut[g] = cum[g];
              cutb[g] = prev[g];
            }
          }
        }
        if (__all(bstar >= 0)) break;
      }
      cut_s[0][lane] = (unsigned)bstar;
      cut_s[1][lane] = (unsigned)total;
#pragma unroll
      for (int g = 0; g < NG; g++) {
        cut_s[2 + g][lane] = cut[g];
        cut_s[2 + NG + g][lane] = cutb[g];
      }
    }
    __syncthreads();
    bstar = (int)cut_s[0][lane];
    total = (int)cut_s[1][lane];
#pragma unroll
    for (int g = 0; g < NG; g++) {
      cut[g] = cut_s[2 + g][lane];
      cutb[g] = cut_s[2 + NG + g][lane];
    }
    // slots of the waves before this one, among all and among the below-cut
    // keys; the lane's below-cut total
    const int mg = wv / FPD;
    const unsigned below = (1u << ((wv % FPD) * CB)) - 1u;
    slot = slot_lo = lo_total = 0;
#pragma unroll
    for (int g = 0; g < NG; g++) {
      slot += (int)field_sum<CB>(g < mg ? cut[g] : (g == mg ? (cut[g] & below) : 0u));
      slot_lo += (int)field_sum<CB>(g < mg ? cutb[g] : (g == mg ? (cutb[g] & below) : 0u));
      lo_total += (int)field_sum<CB>(cutb[g]);
    }
  };
  // the collected keys sit in two regions of the key buffer: rows [0, S) the
  // keys below the cut bin (all among the k nearest, S < k), rows [cut0,
  // cut0 + total - S) the cut bin's keys, so each is ranked within its own
  // region (S^2 + C^2 compares instead of (S + C)^2).  A lane whose cut bin
  // holds more than CAP - cut0 keys overflows.
  const int cut0 = (k + 7) & ~7;
  auto overflow = [&]() { return qlive && total - lo_total > CAP - cut0; };
  if (!fallback) {
    count_cut(ftop);
    const bool no_cut = __any(qlive && bstar < 0);
    if (!no_cut && __any(overflow())) {
      // refine: bin 0 = below the cut bin, bins 1..16 = its 16 sub-bins
      const float lim = qlive ? __uint_as_float((unsigned)(base + bstar + 1) << 21) : 0.0f;
      base = qlive ? ((base + bstar) << 4) - 1 : 0;
      shift = 17;
      __syncthreads();  // pass-1 histogram reads done
      for (int i = threadIdx.x; i < NG * (kNB + 1) * kBlk; i += NW * kBlk) hist_s[i] = 0u;
      __syncthreads();
      count_cut(lim);
    }
    fallback = __any(qlive && bstar < 0) || __any(overflow());
    if (qlive && !fallback) {
      ucut = (unsigned)(base + bstar + 1) << shift;
      ulo = bstar > 0 ? (unsigned)(base + bstar) << shift : 0u;
    }
  }
  __syncthreads();  // histogram reads done: buf_s overwrites it
  (void)nvisit;

  if (!fallback) {
    // 4. collect
    const float fcut = __uint_as_float(ucut);
    int slot_cut = cut0 + (slot - slot_lo);
    visit(fcut, std::true_type(), [&](int pos, const float (&d)[4], uint2 jp) {
      bool take[4];
#pragma unroll
      for (int h = 0; h < 4; h++) take[h] = __float_as_uint(d[h]) < ucut;
      // most groups of four are taken by no lane: skip them uniformly
      if (__any(take[0] | take[1] | take[2] | take[3])) {
        const int4 jj = CL ? int4{(int)(jp.x & 0xFFFFu), (int)(jp.x >> 16), (int)(jp.y & 0xFFFFu),
                                  (int)(jp.y >> 16)}
                           : cand_idx4(pos);
        const int j4[4] = {jj.x, jj.y, jj.z, jj.w};
#pragma unroll
        for (int h = 0; h < 4; h++) {
          // exec-masked: only the taking lanes store (few lanes of a wave)
          if (take[h]) {
            const bool lo = __float_as_uint(d[h]) < ulo;
            buf_s[(lo ? slot_lo : slot_cut) * kBlk + lane] = make_key_finite(d[h], j4[h]);
            slot_lo += lo ? 1 : 0;
            slot_cut += lo ? 0 : 1;
          }
        }
      }
    });
    // region sizes: S = lo_total below the cut bin, C = total - S in it;
    // rows past a lane's own count, up to the wave-wide maximum rounded to
    // four (the sweep reads four rows per wait: eight made this phase the
    // kernel's VGPR peak, 94 instead of 72), read as padding
    const int cnt_c = total - lo_total;
    auto wave_max_i = [&](int v) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
      return __builtin_amdgcn_readfirstlane(v);
    };
    const int smax = wave_max_i(lo_total), cmax = wave_max_i(cnt_c);
    const int spad = (smax + 3) & ~3, cpad = (cmax + 3) & ~3;
    for (int i = lo_total + wv; i < spad; i += NW) buf_s[i * kBlk + lane] = PCR_KEY_PAD;
    for (int i = cnt_c + wv; i < cpad; i += NW) buf_s[(cut0 + i) * kBlk + lane] = PCR_KEY_PAD;
    __syncthreads();

    // 5. rank: wave wv holds the keys wv, wv + NW, ... of each region and
    //    counts, for each, the keys below it in one sweep of that region's
    //    rows; the sweep is compiled for a few key counts so that no compare
    //    is wasted on empty key slots and none needs a guard.  A below-cut
    //    key's rank is its rank in its region; a cut-bin key's is S + its
    //    rank in its region.
    constexpr int kEL = (KSEL + NW - 1) / NW;  // below-cut keys per wave (S < k <= KSEL)
    constexpr int kEC = CAP / NW;              // cut-bin keys per wave (C <= CAP - cut0)
    constexpr int kE = kEC > kEL ? kEC : kEL;
    // one register set for both regions (the below-cut keys are placed before
    // the cut bin's are loaded): the selection's VGPRs bound how many other
    // waves share its CUs
    kkey key[kE];
    int rank[kE];
    const int nel = (smax - wv + NW - 1) / NW;
    const int nec = (cmax - wv + NW - 1) / NW;
    // rows [r0, r0 + rpad) against the first NE keys, four rows per wait
    auto sweep = [&](auto ne_c, int r0, int rpad) __attribute__((always_inline)) {
      constexpr int NE = decltype(ne_c)::value;
      for (int j2 = r0; j2 < r0 + rpad; j2 += 4) {
        kkey o[4];
#pragma unroll
        for (int u = 0; u < 4; u++) o[u] = buf_s[(j2 + u) * kBlk + lane];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
          for (int e = 0; e < NE; e++) rank[e] += o[u] < key[e] ? 1 : 0;
      }
    };
    auto sweep_n = [&](int ne, int r0, int rpad, auto km_c) __attribute__((always_inline)) {
      constexpr int KM = decltype(km_c)::value;
      if (ne <= 0) return;
      if (ne <= 1)
        sweep(std::integral_constant<int, 1>(), r0, rpad);
      else if (ne <= 2)
        sweep(std::integral_constant<int, 2>(), r0, rpad);
      else if (ne <= 3 || KM <= 3)
        sweep(std::integral_constant<int, (KM < 3 ? KM : 3)>(), r0, rpad);
      else if (ne <= 4 || KM <= 4)
        sweep(std::integral_constant<int, (KM < 4 ? KM : 4)>(), r0, rpad);
      else if (ne <= 6 || KM <= 6)
        sweep(std::integral_constant<int, (KM < 6 ? KM : 6)>(), r0, rpad);
      else if (ne <= 8 || KM <= 8)
        sweep(std::integral_constant<int, (KM < 8 ? KM : 8)>(), r0, rpad);
      else
        sweep(std::integral_constant<int, KM>(), r0, rpad);
    };
    // below-cut region: ranks within it are final
#pragma unroll
    for (int e = 0; e < kE; e++) {
      const int i = wv + e * NW;
      key[e] = (e < kEL && i < lo_total) ? buf_s[i * kBlk + lane] : PCR_KEY_PAD;
      rank[e] = 0;
    }
    sweep_n(nel, 0, spad, std::integral_constant<int, kEL>());
    __syncthreads();  // the region's ranking reads are done
    // placed in rows [0, S), which the cut-bin sweep does not read
#pragma unroll
    for (int e = 0; e < kEL; e++)
      if (wv + e * NW < lo_total) buf_s[rank[e] * kBlk + lane] = key[e];
    // cut-bin region: rank S + its rank within the region, kept when < k
    // (rows [S, k) are below cut0, so no sweep reads them)
#pragma unroll
    for (int e = 0; e < kE; e++) {
      const int i = wv + e * NW;
      key[e] = (e < kEC && i < cnt_c) ? buf_s[(cut0 + i) * kBlk + lane] : PCR_KEY_PAD;
      rank[e] = 0;
    }
    sweep_n(nec, cut0, cpad, std::integral_constant<int, kEC>());
#pragma unroll
    for (int e = 0; e < kEC; e++) {
      const int r = lo_total + rank[e];
      if (wv + e * NW < cnt_c && r < k) buf_s[r * kBlk + lane] = key[e];
    }
    __syncthreads();
    if (sorted_emit == 2) {
      // the workgroup's 64 rows of kSkeyK keys are one contiguous range:
      // consecutive threads store consecutive keys (knn_emit_kernel
      // un-permutes them)
      kkey* rows = qs.skey + ((size_t)b * qs.npad + (size_t)qblk * kBlk) * kSkeyK;
      for (int e = threadIdx.x; e < kBlk * k; e += NW * kBlk) {
        const int q = e / k, sl = e - q * k;
        // nontemporal: 268 MB of key rows at c5, read once by the emit
        // (c5 KNN + PPF 2.12 -> 2.09 ms)
        __builtin_nontemporal_store(buf_s[sl * kBlk + q], &rows[(size_t)q * kSkeyK + sl]);
      }
      return;
    }
    if (!qlive) return;

    // output slots wv, wv + NW, ...
    constexpr int SPW = (KSEL + NW - 1) / NW;
    const int n = qs.n;
    int jn[SPW];
#pragma unroll
    for (int u = 0; u < SPW; u++) {
      const int sl = wv + u * NW;
      jn[u] = 0;
      if (sl < k) {
        const kkey x = buf_s[sl * kBlk + lane];
        const size_t o = ((size_t)b * k + sl) * n + qj;
        jn[u] = key_idx(x);
        if (dist) dist[o] = key_dist(x);
        if (sorted_emit)  // sorted query order: whole rows (see kSortedMaxN)
          qs.sidx[((size_t)b * kSortedK + sl) * qs.npad + (size_t)qblk * kBlk + lane] = jn[u];
        else
          idx[o] = jn[u];
      }
    }
    if (PPF) {
      const float* qo = qxyz + (size_t)b * 3 * n;
      const float* qnr = qnrm + (size_t)b * 3 * n;
      const float* cb = cxyz + (size_t)b * 3 * m;
      const float* nb = cnrm + (size_t)b * 3 * m;
      const float ox = qo[qj], oy = qo[qj + n], oz = qo[qj + 2 * n];
      const float cnx = qnr[qj], cny = qnr[qj + n], cnz = qnr[qj + 2 * n];
      float nbr[SPW][6];
#pragma unroll
      for (int u = 0; u < SPW; u++) {
        const int j = jn[u];
        nbr[u][0] = cb[j];
        nbr[u][1] = cb[j + m];
        nbr[u][2] = cb[j + 2 * m];
        nbr[u][3] = nb[j];
        nbr[u][4] = nb[j + m];
        nbr[u][5] = nb[j + 2 * m];
      }
#pragma unroll
      for (int u = 0; u < SPW; u++) {
        const int sl = wv + u * NW;
        if (sl < k) {
          float f[4];
          pcr_local_ppf(ox, oy, oz, cnx, cny, cnz, nbr[u][0], nbr[u][1], nbr[u][2], nbr[u][3],
                        nbr[u][4], nbr[u][5], relative, f);
#pragma unroll
          for (int ch = 0; ch < 4; ch++) ppf[(((size_t)b * 4 + ch) * k + sl) * n + qj] = f[ch];
        }
      }
    }
    return;
  }

  // fallback: wave 0, reference insertion scan, list in LDS (rows 0..k-1)
  if (wv != 0) return;
  const kkey undef = make_key(PCR_KNN_UNDEF, 0);
  for (int s2 = 0; s2 < k; s2++) buf_s[s2 * kBlk + lane] = undef;
  kkey kth = undef;
  for (int blk = 0; blk < nblk; blk++) {
    // cached clouds read the candidates from LDS (broadcast reads)
    const float* bx = CL ? cand_s + blk * kBlk : cs.x + cbase + (size_t)blk * kBlk;
    const float* by = CL ? cand_s + CACHE + blk * kBlk : cs.y + cbase + (size_t)blk * kBlk;
    const float* bz = CL ? cand_s + 2 * CACHE + blk * kBlk : cs.z + cbase + (size_t)blk * kBlk;
    const int* bj = cs.j + cbase + (size_t)blk * kBlk;
    for (int t = 0; t < kBlk; t++) {
      const kkey x = make_key(cand_dist(qx, qy, qz, bx[t], by[t], bz[t]),
                              CL ? (int)cand_j[blk * kBlk + t] : bj[t]);
      if (x < kth) {
        int s2 = k - 1;
        while (s2 > 0) {
          const kkey p = buf_s[(s2 - 1) * kBlk + lane];
          if (p < x) break;
          buf_s[s2 * kBlk + lane] = p;
          s2--;
        }
        buf_s[s2 * kBlk + lane] = x;
        kth = buf_s[(k - 1) * kBlk + lane];
      }
    }
  }
  if (!qlive) return;
  if (sorted_emit == 2) {
    kkey* row = qs.skey + ((size_t)b * qs.npad + (size_t)qblk * kBlk + lane) * kSkeyK;
    for (int s2 = 0; s2 < k; s2++) row[s2] = buf_s[s2 * kBlk + lane];
    return;
  }
  const int n = qs.n;
  for (int s2 = 0; s2 < k; s2++) {
    const kkey x = buf_s[s2 * kBlk + lane];
    const size_t o = ((size_t)b * k + s2) * n + qj;
    if (dist) dist[o] = key_dist(x);
    if (sorted_emit)
      qs.sidx[((size_t)b * kSortedK + s2) * qs.npad + (size_t)qblk * kBlk + lane] = key_idx(x);
    else
      idx[o] = key_idx(x);
  }
  if (PPF) {
    const float* qo = qxyz + (size_t)b * 3 * n;
    const float* qnr = qnrm + (size_t)b * 3 * n;
    const float* cb = cxyz + (size_t)b * 3 * m;
    const float* nb = cnrm + (size_t)b * 3 * m;
    const float ox = qo[qj], oy = qo[qj + n], oz = qo[qj + 2 * n];
    const float cnx = qnr[qj], cny = qnr[qj + n], cnz = qnr[qj + 2 * n];
    for (int s2 = 0; s2 < k; s2++) {
      const int j = key_idx(buf_s[s2 * kBlk + lane]);
      float f[4];
      pcr_local_ppf(ox, oy, oz, cnx, cny, cnz, cb[j], cb[j + m], cb[j + 2 * m], nb[j],
                    nb[j + m], nb[j + 2 * m], relative, f);
#pragma unroll
      for (int ch = 0; ch < 4; ch++) ppf[(((size_t)b * 4 + ch) * k + s2) * n + qj] = f[ch];
    }
  }
}

// Un-permutes the selection's sorted-order keys (qs.skey, sorted_emit 2)
// into the reference's [b][k][n] outputs (knn/knn.cu:40-47 layout) and
// computes the local PPF of every (query, slot) on the way
// (models/pvcnn_classify.py:252-269, the same pcr_local_ppf call as the
// selection's own epilogue).  One wave per 64 consecutive original queries
// and 16 slots (16 contiguous keys of each query's row: one 128-byte line
// per lane); every output store is a whole 256-byte row.
// XCD-aware: the dispatcher deals workgroups round-robin over the 8 XCDs, so
// work unit (blockIdx.x % 8) * (grid / 8) + blockIdx.x / 8 keeps a run of
// consecutive query blocks -- one cloud's neighbour gathers -- in one L2.
template <bool PPF>
__global__ __launch_bounds__(256) void knn_emit_kernel(KnnSet qs, int k, int nqb, float* dist,
                                                       int* idx, const float* __restrict__ qxyz,
                                                       const float* __restrict__ qnrm,
                                                       const float* __restrict__ crec, int m,
                                                       int relative, float* ppf) {
  constexpr int kChunk = kSkeyK / 4;  // slots per wave
  constexpr int kG = 4;               // slots whose neighbours are gathered together
  const int total = gridDim.x;
  int u = blockIdx.x;
  if ((total & 7) == 0) u = (u & 7) * (total >> 3) + (u >> 3);
  const int b = u / nqb, qb = u - b * nqb;
  const int n = qs.n;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int qj = qb * kBlk + lane;
  const int s0 = wv * kChunk;
  if (qj >= n || s0 >= k) return;  // no barrier below
  const int ns = min(k - s0, kChunk);
  const int p = qs.inv[(size_t)b * n + qj];
  // the wave's 16 keys of the query's row at once (one 128-byte line per
  // lane; the row always holds kSkeyK keys, so no guard): each line is
  // fetched once, not once per slot
  const double2* row = (const double2*)(qs.skey + ((size_t)b * qs.npad + p) * kSkeyK + s0);
  kkey key[kChunk];
#pragma unroll
  for (int i = 0; i < kChunk / 2; i++) {
    const double2 v = row[i];
    key[i * 2] = v.x;
    key[i * 2 + 1] = v.y;
  }
  float ox = 0.0f, oy = 0.0f, oz = 0.0f, cnx = 0.0f, cny = 0.0f, cnz = 0.0f;
  // a neighbour's point and normal as one 32-byte record (two dwordx4): one
  // line per gather instead of six
  const float4* rb = (const float4*)(crec + (size_t)b * m * 8);
  if (PPF) {
    const float* qo = qxyz + (size_t)b * 3 * n;
    const float* qnr = qnrm + (size_t)b * 3 * n;
    ox = qo[qj];
    oy = qo[qj + n];
    oz = qo[qj + 2 * n];
    cnx = qnr[qj];
    cny = qnr[qj + n];
    cnz = qnr[qj + 2 * n];
  }
#pragma unroll
  for (int g = 0; g < kChunk; g += kG) {
    if (g >= ns) break;
    float nbr[kG][6];
#pragma unroll
    for (int t = 0; t < kG; t++) {
      const int j = g + t < ns ? key_idx(key[g + t]) : 0;
      if (PPF) {
        const float4 r0 = rb[2 * (size_t)j], r1 = rb[2 * (size_t)j + 1];
        nbr[t][0] = r0.x;
        nbr[t][1] = r0.y;
        nbr[t][2] = r0.z;
        nbr[t][3] = r0.w;
        nbr[t][4] = r1.x;
        nbr[t][5] = r1.y;
      }
    }
#pragma unroll
    for (int t = 0; t < kG; t++) {
      if (g + t >= ns) break;
      const int sl = s0 + g + t;
      const size_t o = ((size_t)b * k + sl) * n + qj;
      // streamed outputs (far larger than the L2 / MALL): nontemporal stores
      // (c5 KNN + PPF 2.20 -> 2.12 ms)
#define PCR_EST(p, v) __builtin_nontemporal_store((v), &(p))
      if (idx) PCR_EST(idx[o], key_idx(key[g + t]));
      if (dist) PCR_EST(dist[o], key_dist(key[g + t]));
      if (PPF) {
        float f[4];
        pcr_local_ppf(ox, oy, oz, cnx, cny, cnz, nbr[t][0], nbr[t][1], nbr[t][2], nbr[t][3],
                      nbr[t][4], nbr[t][5], relative, f);
#pragma unroll
        for (int ch = 0; ch < 4; ch++) PCR_EST(ppf[(((size_t)b * 4 + ch) * k + sl) * n + qj], f[ch]);
      }
    }
  }
}

// [b][3][m] points + normals -> [b][m][8] records (x y z nx ny nz 0 0)
__global__ __launch_bounds__(256) void knn_pack_rec_kernel(const float* __restrict__ xyz,
                                                           const float* __restrict__ nrm, int m,
                                                           float* __restrict__ rec) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= m) return;
  const float* P = xyz + (size_t)b * 3 * m;
  const float* N = nrm + (size_t)b * 3 * m;
  float4* r = (float4*)(rec + ((size_t)b * m + i) * 8);
  r[0] = float4{P[i], P[i + m], P[i + 2 * (size_t)m], N[i]};
  r[1] = float4{N[i + m], N[i + 2 * (size_t)m], 0.0f, 0.0f};
}

// What knn_select_kernel writes (its sorted_emit argument)
enum KnnEmit : int {
  kEmitOriginal = 0,    // dist / idx (+ PPF) in original query order
  kEmitSortedRows = 1,  // neighbour ids in sorted query order (qs.sidx rows)
  kEmitSortedKeys = 2,  // keys in sorted query order (qs.skey), then knn_emit_kernel
};

template <bool PPF>
static void launch_emit(const KnnSet& qs, const KnnSet& cs, int b, int k, const KnnDir& d,
                        hipStream_t st) {
  const int nqb = ceil_div(qs.n, kBlk);
  // the candidates' records, in the candidate set's workspace
  if (PPF)
    hipLaunchKernelGGL(knn_pack_rec_kernel, dim3(ceil_div(cs.n, 256), b), dim3(256), 0, st,
                       d.cxyz, d.cnrm, cs.n, cs.rec);
  hipLaunchKernelGGL((knn_emit_kernel<PPF>), dim3(nqb * b), dim3(256), 0, st, qs, k, nqb, d.dist,
                     d.idx, d.qxyz, d.qnrm, cs.rec, cs.n, d.relative, d.ppf);
}

template <int NW, bool PPF, int CAP = kCap, int KSEL = kSelMaxK>
static void launch_select(const KnnSet& qs, const KnnSet& cs, int b, int k, const KnnDir& d,
                          hipStream_t st, KnnEmit emit = kEmitOriginal) {
  // a wave sees ceil(nblk / NW) * 64 candidates: byte fields when that fits
  PCR_PRIO_INIT();
  const int per_wave = ceil_div(cs.nblk, NW) * kBlk;
  const dim3 grid(qs.nblk, b), blk(NW * 64);
#define PCR_SEL(CBV, CLV, CACHEV)                                                             \
  hipLaunchKernelGGL((knn_select_kernel<NW, CBV, CLV, PPF, CAP, KSEL, CACHEV>), grid, blk, 0, st, \
                     qs, cs, k, d.dist, d.idx, d.qxyz, d.qnrm, d.cxyz, d.cnrm, d.relative,     \
                     d.ppf, (int)emit)
  if constexpr (CAP == kCap) {
    // c3 clouds (2048 points): 32 KB of candidates in LDS, two workgroups per CU
    if (cs.npad > kSelCache && cs.npad <= 2 * kSelCache) {
      PCR_SEL(16, true, 2 * kSelCache);
      return;
    }
  }
  if (per_wave <= 255 && cs.npad <= kSelCache)
    PCR_SEL(8, true, kSelCache);
  else if (per_wave <= 255)
    PCR_SEL(8, false, kSelCache);
  else
    PCR_SEL(16, false, kSelCache);
#undef PCR_SEL
}

size_t knn_ws_size(int b, int n, int m) {
  size_t off = knn_set_layout(b, n, nullptr, nullptr, 0);
  return knn_set_layout(b, m, nullptr, nullptr, off);
}

template <bool PPF>
static pcr_status launch_block(const KnnSet& qs, const KnnSet& cs, int b, int k, const KnnDir& d,
                               hipStream_t st, KnnEmit emit = kEmitOriginal) {
  const bool sel = k <= kSelMaxK || (k <= kSelMaxK64 && cs.npad > kSelCache);
  if (sel && emit == kEmitOriginal && qs.skey != nullptr) {
    // queries past kSortedMaxN: keys in sorted query order, then un-permuted
    if (k <= kSelMaxK)
      launch_select<8, false>(qs, cs, b, k, KnnDir{}, st, kEmitSortedKeys);
    else
      launch_select<8, false, kCap64, kSelMaxK64>(qs, cs, b, k, KnnDir{}, st, kEmitSortedKeys);
    launch_emit<PPF>(qs, cs, b, k, d, st);
    return PCR_OK;
  }
  if (k <= kSelMaxK) {
    launch_select<8, PPF>(qs, cs, b, k, d, st, emit);
  } else if (k <= kSelMaxK64 && cs.npad > kSelCache) {
    // large clouds (BASELINE c5, k = 64): the pruned threshold selection with
    // room for 2.75 k collected keys per query
    launch_select<8, PPF, kCap64, kSelMaxK64>(qs, cs, b, k, d, st);
  } else {
    if (k > 128) return PCR_ERR_UNSUPPORTED;
    launch_block_kernel(qs, cs, b, k, d, st, PPF);
  }
  return PCR_OK;
}

// Returns PCR_ERR_UNSUPPORTED (nothing launched) when the spatial path does
// not apply; the caller then uses the brute-force kernels.
pcr_status knn_spatial(const float* xyz1, const float* xyz2, int b, int n, int m, int k,
                       const KnnIO& io, void* ws, size_t ws_bytes, bool self, hipStream_t st,
                       int stages) {
  if (ws == nullptr || n > kKnnMaxN || m > kKnnMaxN || n < 1 || m < 1 || k > 128)
    return PCR_ERR_UNSUPPORTED;
  if (ws_bytes < knn_ws_size(b, n, m)) return PCR_ERR_UNSUPPORTED;
  KnnSet s1, s2;
  size_t off = knn_set_layout(b, n, &s1, (char*)ws, 0);
  knn_set_layout(b, m, &s2, (char*)ws, off);
  if (stages & kKnnSort) {
    launch_sort(xyz1, b, n, s1, st);
    if (!self) launch_sort(xyz2, b, m, s2, st);
  }
  if (!(stages & kKnnSelect)) return PCR_OK;
  const KnnSet& c1 = self ? s1 : s2;
  if (stages & kKnnSortedRows) {
    // selection only, neighbour ids in sorted query order into s1.sidx (the
    // cached selection, k <= kSortedK); the caller's PPF launch un-permutes
    if (!self || io.ppf1 || io.dist1 || io.idx2 || k > kSortedK || k > kSelMaxK ||
        s1.sidx == nullptr || s1.npad > 2 * kSelCache)
      return PCR_ERR_UNSUPPORTED;
    // clouds of <= 1024 points: the transposed selection (c2: 31.0 us alone
    // against 32.8 for knn_select_kernel).  At 2048 points its R = 32
    // registers per coordinate leave 2 waves per SIMD and it lost (928 us
    // against 600 at c3), so those keep the per-lane kernel.
    if (s1.npad <= 16 * kBlk) {
      launch_wsel(s1, b, k, st);
      return PCR_OK;
    }
    return launch_block<false>(s1, c1, b, k, KnnDir{nullptr, io.idx1}, st, kEmitSortedRows);
  }
  pcr_status rc;
  if (io.ppf1)
    rc = launch_block<true>(s1, c1, b, k,
                            KnnDir{io.dist1, io.idx1, xyz1, io.nrm1, xyz2, io.nrm2, io.relative,
                                   io.ppf1},
                            st);
  else
    rc = launch_block<false>(s1, c1, b, k, KnnDir{io.dist1, io.idx1}, st);
  if (rc != PCR_OK) return rc;
  if (io.idx2) rc = launch_block<false>(c1, s1, b, k, KnnDir{io.dist2, io.idx2}, st);
  return rc;
}

// the sorted-order outputs of a self KNN workspace (kKnnSortedRows)
bool knn_sorted_views(void* ws, int b, int n, const int** sidx, const int** inv, int* npad) {
  KnnSet s;
  knn_set_layout(b, n, &s, (char*)ws, 0);
  *sidx = s.sidx;
  *inv = s.inv;
  *npad = s.npad;
  return s.sidx != nullptr;
}

}  // namespace pcr

extern "C" size_t pcr_knn_workspace_size(int b, int n, int m) {
  if (b <= 0 || n <= 0 || m <= 0) return 256;
  return pcr::knn_ws_size(b, n, m);
}
