// knn_wsel.hip -- the transposed self-KNN selection of small clouds
// (knn_spatial.hip's kKnnSortedRows stage), for gfx950.
//
// knn_wsel_kernel (round 5): the self-KNN selection of clouds of <= 64 R
// points, k <= 32, transposed -- one query per wave instruction, the cloud's
// candidates in the lanes.  The workgroup lands the cloud's sorted x / y / z /
// index rows in LDS once (LDS-DMA, 16 KB at 1024 points; until round 7 each
// of its 8 or 12 waves loaded the whole cloud from global memory: 53 loads per
// wave, 12x the vector-L1 requests).  Lane l then holds the Morton-sorted
// candidates 64 r + l (r < R) in registers for the whole launch, filled from
// LDS two registers per ds_read2st64_b32, so a query costs:
//
//  1. distances  its R distances per lane with the reference's FMA chain
//                (knn.cu:20-23; two candidates per packed instruction);
//  2. threshold  count(d <= t) over the wave is one v_cmp + s_bcnt1 per
//                register (the count is a ballot across the lanes, so no
//                per-pair atomic and no histogram).  t starts from the
//                previous query's threshold (Morton neighbours have similar
//                k-th distances) and moves by count ~ t^1.5 interpolation,
//                bracketed, until k <= count <= 64: 1.78 passes on average
//                with 12 waves taking a block's queries one at a time (a
//                wave's previous query is ~12 Morton positions back; seeding
//                from the nearest finished query of the block instead saves
//                0.03 passes in scripts/wsel_seed_model.py: not built);
//  3. compact    the <= 64 keys with d <= t into one lane each (ballot +
//                mbcnt slots in the wave's LDS rows; per candidate register
//                4 VALU and one ds_write2st64_b32 of distance + position);
//  4. sort       a 64-lane bitonic sort of 32-bit keys (d bits >> 5 << 6 |
//                slot): DPP / swizzle partners, min / max / select per stage.
//                Two keys whose truncated distances tie inside the first k
//                send the query to the exact 64-bit sort, as do
//  5. edge cases no t with k <= count <= 64 (exact duplicates, clusters):
//                the exact k-th distance by bisection of its float bits, the
//                tie at it broken by bisection of the original index, the
//                exactly k members compacted and sorted on 64-bit keys.
//
// Result: the k lexicographically smallest (d, original index) with d <
// 10000, unfilled slots index 0 -- the reference's insertion-sort result
// (knn.cu:24-46).  Written as neighbour ids in sorted query order (KnnSet::
// sidx rows, like knn_select_kernel's sorted_emit 1) through an LDS tile, so
// every store is a whole 256-byte row.
#include "knn_spatial.hpp"

namespace pcr {

// Waves per workgroup (one 64-query block), W, and the queries a wave takes
// from the block's counter at a time, wsel_chunk<W>.  A launch of at most
// 4096 waves at W = 8 (c2: 32 clouds x 16 blocks) leaves 4 waves per SIMD:
// there W = 12 (the compiler then fits the kernel in 81 VGPRs instead of 91)
// taking one query at a time, c2 +1.7% (profiles/r06_ab_wsel_waves.log,
// r06_ab_wsel_chunk.log, r06_ab_wsel_pairs_waves.log; 10 waves -3%, 14 / 16
// spill SGPRs, -12%).  Larger launches (pairs: 256 clouds) keep W = 8 with
// two queries at a time: each wave holds the whole cloud in registers, and
// 12 waves cost pairs 9% (312-315k against 341-343k clouds/s, measured when
// every wave still loaded the cloud from global memory).
template <int W>
constexpr int wsel_chunk() { return W == 8 ? 2 : 1; }
// true: W = 8 (more than 4096 waves at W = 8), false: W = 12
static inline bool wsel_narrow(int nblk, int b) { return (size_t)nblk * b * 8 > 4096; }
constexpr int kWselCap = 64;   // keys collected per query (one per lane)
constexpr int kWselTmax = 0x461C3FFF;  // bits of the largest float below 10000

// One compare-exchange stage of the sort below where the lower lanes of the
// pairs are the even lanes (m = 1) or lanes 0-1 of each quad (m = 2): the
// partner by DPP, folded into the compare and the select (2 VALU + 2 SALU):
// the borrow of partner - x (v_sub_co: VOPC has no DPP form on gfx950) is vcc
// = partner < x, flipped on the lanes that keep the minimum, then x = vcc ? x
// : partner.  s_nop 1: the previous stage's VALU wrote x, which this DPP
// reads (gfx9 needs 2 wait states).
#define PCR_WSEL_VCC_STAGE(NAME, CTRL, LOW)                                        \
  __device__ inline unsigned NAME(unsigned x) {                                    \
    unsigned t;                                                                    \
    asm volatile("s_nop 1\n\t"                                                     \
                 "v_sub_co_u32_dpp %1, vcc, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\t" \
                 "s_xor_b32 vcc_lo, vcc_lo, " LOW "\n\t"                           \
                 "s_xor_b32 vcc_hi, vcc_hi, " LOW "\n\t"                           \
                 "v_cndmask_b32_dpp %0, %0, %0, vcc " CTRL " row_mask:0xf bank_mask:0xf" \
                 : "+v"(x), "=&v"(t)                                               \
                 :                                                                 \
                 : "vcc");                                                         \
    return x;                                                                      \
  }
PCR_WSEL_VCC_STAGE(wsel_x1, "quad_perm:[1,0,3,2]", "0x55555555")
PCR_WSEL_VCC_STAGE(wsel_x2, "quad_perm:[2,3,0,1]", "0x33333333")
PCR_WSEL_VCC_STAGE(wsel_m4, "quad_perm:[3,2,1,0]", "0x33333333")
#undef PCR_WSEL_VCC_STAGE
// Stages whose lower lanes are whole 4-lane banks of a row (m = 4, 8) or whole
// rows (m = 16, 32): the DPP bank / row masks pick the lanes, so the lower
// lanes write min(partner, x) and the upper lanes max(partner, x) into a new
// register with two masked VALU -- no VCC, no SALU.  LO / HI are the
// partner's DPP controls for the lower / upper lanes, MLO / MHI their masks.
#define PCR_WSEL_MINMAX_STAGE(NAME, LO, HI, MLO, MHI)                              \
  __device__ inline unsigned NAME(unsigned x) {                                    \
    unsigned a;                                                                    \
    asm volatile("s_nop 1\n\t"                                                     \
                 "v_min_u32_dpp %0, %1, %1 " LO " " MLO "\n\t"                     \
                 "v_max_u32_dpp %0, %1, %1 " HI " " MHI                            \
                 : "=&v"(a)                                                        \
                 : "v"(x));                                                        \
    return a;                                                                      \
  }
PCR_WSEL_MINMAX_STAGE(wsel_m8, "row_half_mirror", "row_half_mirror",
                      "row_mask:0xf bank_mask:0x5", "row_mask:0xf bank_mask:0xa")
PCR_WSEL_MINMAX_STAGE(wsel_m16, "row_mirror", "row_mirror",
                      "row_mask:0xf bank_mask:0x3", "row_mask:0xf bank_mask:0xc")
PCR_WSEL_MINMAX_STAGE(wsel_x4, "row_shl:4", "row_shr:4",
                      "row_mask:0xf bank_mask:0x5", "row_mask:0xf bank_mask:0xa")
PCR_WSEL_MINMAX_STAGE(wsel_x8, "row_shl:8", "row_shr:8",
                      "row_mask:0xf bank_mask:0x3", "row_mask:0xf bank_mask:0xc")
#undef PCR_WSEL_MINMAX_STAGE
// Cross-row partners (FETCH into %2): lane ^ 16 / lane ^ 32 from gfx950's
// v_permlane16_swap / v_permlane32_swap of a register with itself, the 32- and
// 64-lane mirrors from a row mirror plus those swaps; then the row-masked
// min / max (identity DPP: only its row mask matters).  No LDS round trip.
#define PCR_WSEL_ROW_STAGE(NAME, FETCH, RLO, RHI)                                  \
  __device__ inline unsigned NAME(unsigned x) {                                    \
    unsigned a, p;                                                                 \
    asm volatile("s_nop 1\n\t" FETCH                                               \
                 "s_nop 1\n\t"                                                     \
                 "v_min_u32_dpp %0, %1, %2 quad_perm:[0,1,2,3] row_mask:" RLO " bank_mask:0xf\n\t" \
                 "v_max_u32_dpp %0, %1, %2 quad_perm:[0,1,2,3] row_mask:" RHI " bank_mask:0xf" \
                 : "=&v"(a), "+v"(x), "=&v"(p)                                     \
                 :);                                                               \
    return a;                                                                      \
  }
PCR_WSEL_ROW_STAGE(wsel_x16,
                   "v_mov_b32_e32 %2, %1\n\t"
                   "s_nop 1\n\t"
                   "v_permlane16_swap_b32 %2, %2\n\t",
                   "0x5", "0xa")
PCR_WSEL_ROW_STAGE(wsel_m32,
                   "v_mov_b32_dpp %2, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"
                   "s_nop 1\n\t"
                   "v_permlane16_swap_b32 %2, %2\n\t",
                   "0x5", "0xa")
PCR_WSEL_ROW_STAGE(wsel_m64,
                   "v_mov_b32_dpp %2, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"
                   "s_nop 1\n\t"
                   "v_permlane16_swap_b32 %2, %2\n\t"
                   "s_nop 1\n\t"
                   "v_permlane32_swap_b32 %2, %2\n\t",
                   "0x3", "0xc")
#undef PCR_WSEL_ROW_STAGE

// ascending 64-lane bitonic sort ("mirror" form: the first stage of each
// merge compares i with its mirror i ^ (kk - 1), so every block sorts
// ascending and the lower lane of a pair always keeps the minimum)
__device__ inline unsigned wsel_sort64(unsigned x) {
  x = wsel_x1(x);
  x = wsel_m4(x);
  x = wsel_x1(x);
  x = wsel_m8(x);
  x = wsel_x2(x);
  x = wsel_x1(x);
  x = wsel_m16(x);
  x = wsel_x4(x);
  x = wsel_x2(x);
  x = wsel_x1(x);
  x = wsel_m32(x);
  x = wsel_x8(x);
  x = wsel_x4(x);
  x = wsel_x2(x);
  x = wsel_x1(x);
  x = wsel_m64(x);
  x = wsel_x16(x);
  x = wsel_x8(x);
  x = wsel_x4(x);
  x = wsel_x2(x);
  x = wsel_x1(x);
  // the caller's next DPP read of x follows a VALU write inside the asm above,
  // which the compiler's hazard tracking does not see
  asm volatile("s_nop 1");
  return x;
}

// the same on 64-bit keys (d bits << 32 | original index): exact, rare
__device__ inline unsigned long long wsel_sort64_exact(unsigned long long x, int lane) {
  for (int kk = 2; kk <= 64; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      const int m = jj == (kk >> 1) ? kk - 1 : jj;  // mirror first, then half-cleaners
      const unsigned long long p = shfl_xor_u64(x, m);
      const bool lower = (lane & jj) == 0;
      x = lower ? (x < p ? x : p) : (x < p ? p : x);
    }
  }
  return x;
}

// Appends the keys of candidate register r's lanes in `m` (a ballot mask) to
// the wave's LDS rows at slots base, base + 1, ...: d bits to kd, the sorted
// position 64 r + lane to kd + 256 bytes, both by one ds_write2st64_b32.
// The position is one VALU on the one lane register, 64 r an immediate (r is
// a constant once the caller's loop is unrolled and this is inlined): as a
// C++ expression the compiler hoists the R positions out of the query loop,
// one VGPR each (109 instead of 91 VGPRs; c2 -1.8%,
// profiles/r05_wsel_opaque_ab.log).  Then exec = m for three VALU (the slot:
// mbcnt lo / hi; the address) and the write, restored after: no per-lane
// condition is materialised.
__device__ __attribute__((always_inline)) inline void wsel_append(unsigned long long m,
                                                                  unsigned addr, unsigned d,
                                                                  int lane, int r) {
  unsigned t, p;
  unsigned long long save;
  asm volatile("v_add_u32_e32 %0, %2, %1" : "=v"(p) : "v"(lane), "i"(64 * r));
  asm volatile(
      "s_mov_b64 %1, exec\n\t"
      "s_mov_b64 exec, %2\n\t"
      "v_mbcnt_lo_u32_b32 %0, %3, 0\n\t"
      "v_mbcnt_hi_u32_b32 %0, %4, %0\n\t"
      "v_lshl_add_u32 %0, %0, 2, %5\n\t"
      "ds_write2st64_b32 %0, %6, %7 offset1:1\n\t"
      "s_mov_b64 exec, %1"
      : "=&v"(t), "=&s"(save)
      : "s"(m), "s"((unsigned)m), "s"((unsigned)(m >> 32)), "s"(addr), "v"(d), "v"(p)
      : "memory");
}

template <int R, int W>
__global__ __launch_bounds__(W * 64) void knn_wsel_kernel(KnnSet s, int k) {
  constexpr int kWselWaves = W;
  constexpr int kWselChunk = wsel_chunk<W>();
  // [wave][0][slot] collected d bits, [wave][1][slot] their sorted positions
  // (256 bytes apart: wsel_append's ds_write offset)
  __shared__ unsigned kbuf_s[kWselWaves][2][kWselCap];
  __shared__ int tile_s[kBlk][kSortedK + 1];  // output ids [query][slot] (padded: no bank conflicts)
  __shared__ int qnext_s;                     // the next chunk of the block's queries
  // the cloud's sorted coordinates and original indices (position p = 64 r +
  // lane), staged once per workgroup: NaN / -1 from the cloud's end
  __shared__ __align__(16) float cx_s[R * kBlk], cy_s[R * kBlk], cz_s[R * kBlk];
  __shared__ __align__(16) int cj_s[R * kBlk];
  static_assert(sizeof(kbuf_s[0][0]) == 256, "wsel_append's offset");
  static_assert(sizeof(cx_s) % (64 * 16) == 0, "whole LDS-DMA pieces");
  const int b = blockIdx.y, qblk = blockIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const size_t cb = (size_t)b * s.npad;
  // One copy of the cloud per workgroup, by LDS-DMA (rows of npad elements at
  // 256-byte aligned offsets; the last piece's lanes past the row re-read its
  // last 16 bytes, and the arrays are whole pieces).  Rows shorter than the
  // arrays: once the copy has landed, everything past the row becomes NaN / -1,
  // so no position of the arrays is read unwritten.
  lds_dma_copy<16>(cx_s, s.x + cb, 4 * s.npad);
  lds_dma_copy<16>(cy_s, s.y + cb, 4 * s.npad);
  lds_dma_copy<16>(cz_s, s.z + cb, 4 * s.npad);
  lds_dma_copy<16>(cj_s, s.j + cb, 4 * s.npad);
  if (threadIdx.x == 0) qnext_s = 0;
  wait_vmcnt<0>();
  __syncthreads();
  if (s.npad < R * kBlk) {
    for (int i = s.npad + threadIdx.x; i < R * kBlk; i += kWselWaves * kBlk) {
      cx_s[i] = cy_s[i] = cz_s[i] = __builtin_nanf("");
      cj_s[i] = -1;
    }
    __syncthreads();
  }
  typedef float pf2v __attribute__((ext_vector_type(2)));
  // the whole cloud, one candidate per lane and register: a register pair's
  // positions are 64 dwords apart, one ds_read2st64_b32 (the compaction stores
  // positions, the output looks the original index up in cj_s)
  pf2v cx[R / 2], cy[R / 2], cz[R / 2];
#pragma unroll
  for (int h = 0; h < R / 2; h++) {
    const int p = 2 * h * kBlk + lane;
    cx[h] = pf2v{cx_s[p], cx_s[p + kBlk]};
    cy[h] = pf2v{cy_s[p], cy_s[p + kBlk]};
    cz[h] = pf2v{cz_s[p], cz_s[p + kBlk]};
  }
  // the block's 64 queries, one per lane (every wave holds all of them: the
  // waves take chunks of kWselChunk consecutive queries from an LDS counter,
  // so a wave that drew expensive queries -- outliers, extra passes -- takes
  // fewer chunks and the workgroup ends with its mean, not its slowest wave)
  const int pq = qblk * kBlk + lane;
  const float qxl = cx_s[pq], qyl = cy_s[pq], qzl = cz_s[pq];
  const int qjl = cj_s[pq];
  auto grab = [&]() {
    int v = 0;
    if (lane == 0)
      v = __hip_atomic_fetch_add(&qnext_s, kWselChunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return v;
  };
  int q0 = __builtin_amdgcn_readfirstlane(grab());
  // first guess: the largest distance from the wave's first query to its own
  // block's box (>= the k-th when the block holds k points), else 10000-
  int tb = kWselTmax;
  if (q0 < kBlk) {
    const float* bx = s.box + ((size_t)b * s.nblk + qblk) * 8;
    const float qx = readlane_f(qxl, q0), qy = readlane_f(qyl, q0), qz = readlane_f(qzl, q0);
    if (min(kBlk, s.n - qblk * kBlk) >= k) {
      const float u = box_ub(qx, qy, qz, bx);
      if (u < PCR_KNN_UNDEF) tb = (int)__float_as_uint(u);
    }
  }
  unsigned* kd = kbuf_s[wv][0];
  int* kj = (int*)kbuf_s[wv][1];
  const unsigned kd_addr =  // LDS byte address of the wave's rows
      (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned*)kd);
  const float tgt = 0.5f * (float)(k + kWselCap);
#pragma unroll 1
  for (int qi = q0; qi < kBlk;) {
    const int qj = __builtin_amdgcn_readlane(qjl, qi);
    if (qj < 0) {
      if (lane < kSortedK) tile_s[qi][lane] = 0;
      if (++qi % kWselChunk == 0) qi = __builtin_amdgcn_readfirstlane(grab());
      continue;
    }
    const float qx = readlane_f(qxl, qi), qy = readlane_f(qyl, qi), qz = readlane_f(qzl, qi);
    const pf2v qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
    // 1. distances, knn.cu:20-23's chain
    unsigned db[R];
#pragma unroll
    for (int h = 0; h < R / 2; h++) {
      const pf2v a = qx2 - cx[h], bq = qy2 - cy[h], c = qz2 - cz[h];
      pf2v d = a * a;
      d = __builtin_elementwise_fma(bq, bq, d);
      d = __builtin_elementwise_fma(c, c, d);
      db[2 * h] = __float_as_uint(d[0]);
      db[2 * h + 1] = __float_as_uint(d[1]);
    }
    // 2. threshold: count(d <= t) by ballots (NaN bits compare above every t)
    // the last pass's ballots are kept for the compaction when they fit in
    // SGPRs (R = 16: 32 of them); R = 32 ballots again there
    constexpr bool kKeep = R <= 16;
    unsigned long long msk[kKeep ? R : 1];
    auto count_le = [&](int bits) {
      // four running popcount sums: a dependency chain a quarter as long
      int pc[4] = {0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < R; r++) {
        const unsigned long long m = __ballot(db[r] <= (unsigned)bits);
        if (kKeep) msk[kKeep ? r : 0] = m;
        pc[r & 3] += __popcll(m);
      }
      return (pc[0] + pc[1]) + (pc[2] + pc[3]);
    };
    int lo = -1, hi = 0x7F800000, cnt_lo = 0, cnt = 0;
    bool exact = false;
#pragma unroll 1
    for (int pass = 0;; pass++) {
      cnt = count_le(tb);
      if (cnt >= k && cnt <= kWselCap) break;
      if (cnt < k) {
        lo = tb;
        cnt_lo = cnt;
        if (tb >= kWselTmax) break;  // fewer than k candidates below 10000: all of them
      } else {
        hi = tb;
      }
      if (hi - lo <= 1) {  // more than 64 - cnt_lo keys tie at distance bits hi
        exact = true;
        break;
      }
      int nb;
      if (pass < 3) {
        // count ~ t^1.5 near the k-th distance (smooth clouds: ~1.6 passes)
        // (raw v_log / v_exp: any estimate is correct here, the bracket
        // below keeps it inside (lo, hi); the library forms add range fixups)
        const float f = __uint_as_float((unsigned)tb) *
                        __builtin_amdgcn_exp2f(0.6666667f * __builtin_amdgcn_logf(
                                                                tgt * __builtin_amdgcn_rcpf((float)max(cnt, 1))));
        nb = f < 1e30f ? (int)__float_as_uint(f) : kWselTmax;
      } else {
        // steep counts (an outlier facing the bulk): bisect the bracket's bits
        nb = lo + ((hi - lo) >> 1);
      }
      nb = min(nb, kWselTmax);
      if (nb <= lo || nb >= hi) nb = lo + ((hi - lo) >> 1);
      tb = __builtin_amdgcn_readfirstlane(nb);
    }
    int ntake;
    if (!exact) {
      // 3. compact the cnt <= 64 keys with d <= t (the last pass's ballots)
      unsigned addr = kd_addr;
#pragma unroll
      for (int r = 0; r < R; r++) {
        const unsigned long long m = kKeep ? msk[kKeep ? r : 0] : __ballot(db[r] <= (unsigned)tb);
        if (m != 0ull) {
          wsel_append(m, addr, db[r], lane, r);
          addr += 4u * (unsigned)__popcll(m);
        }
      }
      ntake = cnt;
    } else {
      // 5. ties: every key below distance bits hi (cnt_lo < k of them), then
      // the need = k - cnt_lo smallest indices among those at exactly hi
      const int need = k - cnt_lo;
      // (rare: the indices are read from LDS where used, no registers held)
      auto cj = [&](int r) { return cj_s[64 * r + lane]; };
      int jl = -1, jh = s.n - 1;
#pragma unroll 1
      while (jh - jl > 1) {
        const int jm = jl + ((jh - jl) >> 1);
        int c = 0;
#pragma unroll
        for (int r = 0; r < R; r++) c += __popcll(__ballot(db[r] == (unsigned)hi && cj(r) <= jm));
        if (c >= need) jh = jm;
        else jl = jm;
      }
      unsigned addr = kd_addr;
#pragma unroll
      for (int r = 0; r < R; r++) {
        const unsigned long long m =
            __ballot(db[r] < (unsigned)hi || (db[r] == (unsigned)hi && cj(r) <= jh));
        if (m != 0ull) {
          wsel_append(m, addr, db[r], lane, r);
          addr += 4u * (unsigned)__popcll(m);
        }
      }
      ntake = k;
    }
    // 4. sort 31-bit keys: d bits >> 6 (25 bits: d < 10000) and the slot as payload
    const unsigned dl = lane < ntake ? kd[lane] : 0xFFFFFFFFu;
    unsigned key = lane < ntake ? ((dl >> 6) << 6) | (unsigned)lane : 0x7FFFFFFFu;
    key = wsel_sort64(key);
    // a truncated-distance tie among the first k (or at the k-th) needs the
    // exact order (lane i sees lane i + 1: DPP wave_shl:1)
    const unsigned nxt = (unsigned)__builtin_amdgcn_mov_dpp((int)key, 0x130, 0xF, 0xF, false);
    const bool tie = lane < k && lane + 1 < ntake && (key >> 6) == (nxt >> 6);
    const bool slow = __any(tie);
    if (!slow) {
      const int jo = lane < ntake ? cj_s[kj[key & 63u]] : 0;
      if (lane < k) tile_s[qi][lane] = jo;
    } else {
      unsigned long long skey = ~0ull;
      if (lane < ntake) skey = ((unsigned long long)kd[lane] << 32) | (unsigned)cj_s[kj[lane]];
      skey = wsel_sort64_exact(skey, lane);
      if (lane < k) tile_s[qi][lane] = lane < ntake ? (int)(unsigned)(skey & 0xFFFFFFFFull) : 0;
    }
    // the rows are read before the next query's appends rewrite them (LDS
    // operations of a wave complete in order; this keeps the compiler's order)
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    if (++qi % kWselChunk == 0) qi = __builtin_amdgcn_readfirstlane(grab());
  }
  __syncthreads();
  for (int sl = wv; sl < k; sl += kWselWaves)
    s.sidx[((size_t)b * kSortedK + sl) * s.npad + (size_t)qblk * kBlk + lane] = tile_s[lane][sl];
}

void launch_wsel(const KnnSet& s, int b, int k, hipStream_t st) {
  if (wsel_narrow(s.nblk, b))
    hipLaunchKernelGGL((knn_wsel_kernel<16, 8>), dim3(s.nblk, b), dim3(8 * 64), 0, st, s, k);
  else
    hipLaunchKernelGGL((knn_wsel_kernel<16, 12>), dim3(s.nblk, b), dim3(12 * 64), 0, st, s, k);
}

}  // namespace pcr
