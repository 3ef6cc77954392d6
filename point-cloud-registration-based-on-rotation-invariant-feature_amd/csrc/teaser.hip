// teaser.hip -- batched TEASER-style robust registration for gfx950: the
// reference's register_one_pair(func='teaserpp') (TEASER++ on the CPU, one
// pair at a time) with a bounded greedy clique search in place of the exact
// one, from the mutual-NN correspondences of the matching.  The contract is
// DESIGN.md 4.8d, the scalar math include/pcr_teaser.h + pcr_rigid.h.
//
//   teaser_graph_kernel<false>  the degrees: kTGRows slots per workgroup, every
//     slot of the pair staged in LDS as fp32: a wave takes a slot, a lane a
//     partner, the ballot's popcount is the degree.
//   teaser_rank_kernel    one workgroup per pair ranks the slots by degree
//     (descending, lowest slot first) by counting: order[rank] = slot.
//   teaser_graph_kernel<true>  the edge tests again with the slots staged in rank
//     order: the ballot is a word of the bit row, rows and bits both in rank
//     order, so the best-ranked member of a set is its lowest bit.
//   teaser_clique_kernel  one workgroup per pair, the rows in LDS when n1 <=
//     kTCLds (else read from the workspace).  A group of lanes (one lane per
//     64-bit word of a row) walks one seed: the lowest bit of P over the
//     group, P &= row.  The largest clique, lowest seed on ties, is an integer
//     maximum; wave 0 walks the winner again and marks its slots, which are
//     then written in ascending order by prefix popcounts.
//   teaser_solve_kernel   one workgroup per pair: the clique's points in LDS
//     (fp32; the TIMs are formed on the fly in fp64), the GNC-TLS loop with
//     the weights recomputed from the previous rotation instead of stored
//     (there are K (K - 1) / 2 of them), the per-axis vote and the report.
//     Sums are per-thread fp64 sums in a fixed order, then block_sum_d: no
//     float atomics, the same bits in every thread, so every thread takes the
//     solve itself and every exit is uniform.
#include "common.hpp"
#include "pcr_teaser.h"
#include "rigid_pair.hpp"

namespace pcr {

constexpr int kTGT = 256;     // degree / graph kernels: threads per workgroup
constexpr int kTGRows = 32;   // ... and slots (rows) per workgroup
constexpr int kTRT = 1024;    // rank kernel
constexpr int kTCT = 1024;    // clique kernel
constexpr int kTCLds = 1024;  // largest n1 whose bit rows are staged in LDS (128 KB)
constexpr int kTST = 512;     // solve kernel
constexpr int kTSW = kTST / kWave;
constexpr int kVL = PCR_TEASER_VOTE_LANES;  // endpoints of the vote a thread takes at once
static_assert(kTGT % kWave == 0 && kTCT % kWave == 0 && kTST % kWave == 0, "teaser launch shape");
static_assert(PCR_TEASER_MAX_N1 <= 64 * kWave, "a wave holds a bit row, one word per lane");

typedef unsigned long long u64;

inline int teaser_words(int n1) { return (n1 + 63) / 64; }
// per pair: the bit rows [n1][W], then deg [n1] and order [n1]
inline size_t teaser_ws_bytes(int p, int n1) {
  return align_up((size_t)p * n1 * ((size_t)teaser_words(n1) * 8 + 8), 256);
}
inline size_t teaser_solve_lds(int n1) {
  return (size_t)n1 * (6 * sizeof(float) + sizeof(double)) + (size_t)kTSW * 16 * sizeof(double);
}

// The slots of a pair staged in LDS as six fp32 planes of stride n1, slot
// order[c] at position c (order == nullptr: slot c).
__device__ inline void teaser_stage(const RigidPair& pr, const int* order, int m, float* pts,
                                    int nthreads) {
  for (int c = threadIdx.x; c < m; c += nthreads) {
    float a[3], b[3];
    const int s = order ? min(max(order[c], 0), pr.n1 - 1) : c;
    rigid_slot(pr, s, a, b);
#pragma unroll
    for (int d = 0; d < 3; d++) {
      pts[(size_t)d * pr.n1 + c] = a[d];
      pts[(size_t)(3 + d) * pr.n1 + c] = b[d];
    }
  }
}

__device__ inline void teaser_point(const float* pts, int n1, int c, float* a, float* b) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    a[d] = pts[(size_t)d * n1 + c];
    b[d] = pts[(size_t)(3 + d) * n1 + c];
  }
}

// kRanked = false: deg[slot]; true: the bit rows in rank order
template <bool kRanked>
__global__ __launch_bounds__(kTGT) void teaser_graph_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n1, int n2,
    const int* __restrict__ idx1, const int* __restrict__ idx2, const int* __restrict__ count,
    double beta, int W, const int* __restrict__ order, int* __restrict__ deg,
    u64* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) char teaser_smem[];
  float* pts = (float*)teaser_smem;  // [6][n1]
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const RigidPair pr = rigid_pair(xyz1, xyz2, n1, n2, idx1, idx2, count, q);
  const int M = pr.m, r0 = blockIdx.y * kTGRows;
  if (r0 >= M) return;  // uniform over the workgroup
  teaser_stage(pr, kRanked ? order + (size_t)q * n1 : nullptr, M, pts, kTGT);
  lds_barrier();
  const int Wm = (M + 63) / 64, r1 = min(r0 + kTGRows, M);
  for (int r = r0 + wv; r < r1; r += kTGT / kWave) {
    float ar[3], br[3];
    teaser_point(pts, n1, r, ar, br);
    int cnt = 0;
    u64 mine = 0;
    for (int w = 0; w < Wm; w++) {
      const int c = 64 * w + lane;
      float ac[3], bc[3];
      teaser_point(pts, n1, min(c, M - 1), ac, bc);
      const bool e = c < M && c != r && pcr_teaser_edge(ar, br, ac, bc, beta);
      const u64 word = __ballot(e);
      cnt += __popcll(word);
      if (lane == w) mine = word;  // Wm <= 64: lane w keeps word w
    }
    if (kRanked) {
      if (lane < Wm) rows[((size_t)q * n1 + r) * W + lane] = mine;
    } else if (lane == 0) {
      deg[(size_t)q * n1 + r] = cnt;
    }
  }
}

__global__ __launch_bounds__(kTRT) void teaser_rank_kernel(const int* __restrict__ count, int n1,
                                                           const int* __restrict__ deg,
                                                           int* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) char teaser_smem[];
  int* deg_s = (int*)teaser_smem;  // [n1]
  const int q = blockIdx.x, tid = threadIdx.x;
  const int M = min(max(count[q], 0), n1);
  for (int i = tid; i < M; i += kTRT) deg_s[i] = deg[(size_t)q * n1 + i];
  lds_barrier();
  for (int i = tid; i < M; i += kTRT) {
    const int d = deg_s[i];
    int rank = 0;
    for (int j = 0; j < M; j++) {
      const int dj = deg_s[j];
      rank += (dj > d || (dj == d && j < i)) ? 1 : 0;
    }
    order[(size_t)q * n1 + rank] = i;  // the ranks are a permutation of [0, M)
  }
}

// One seed's greedy walk by a group of g lanes (a power of two; lane l of the
// group holds word l of P).  Every lane of the wave calls it; `rec(rank)` is
// called for each vertex added after the seed.  Returns the clique's size (0
// for an inactive group).
template <typename Rows, typename Rec>
__device__ inline int teaser_walk(Rows row_word, int M, int Wm, int g, int l, int seed,
                                  bool active, Rec rec) {
  u64 P = (active && l < Wm) ? row_word(seed, l) : 0;
  int size = active ? 1 : 0;
  for (int step = 1; step < M; step++) {  // a clique has at most M vertices
    int cand = P ? 64 * l + (int)__builtin_ctzll(P) : INT32_MAX;
    for (int off = 1; off < g; off <<= 1) cand = min(cand, __shfl_xor(cand, off, kWave));
    const bool go = cand != INT32_MAX;
    if (go) {
      if (l < Wm) P &= row_word(cand, l);  // cand is not its own neighbour: its bit goes too
      size++;
      rec(cand);
    }
    if (!__any(go)) break;  // uniform over the wave
  }
  return size;
}

template <bool kLds>
__global__ __launch_bounds__(kTCT) void teaser_clique_kernel(
    const int* __restrict__ count, int n1, int W, int seeds, const int* __restrict__ order,
    const u64* __restrict__ rows, int* __restrict__ clique, int* __restrict__ clique_size) {
  extern __shared__ __attribute__((aligned(16))) char teaser_smem[];
  u64* rows_s = (u64*)teaser_smem;  // kLds: [M][W]
  __shared__ u64 bits_s[PCR_TEASER_MAX_N1 / 64];  // the clique as a set of slots
  __shared__ int best_s;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int M = min(max(count[q], 0), n1);
  const int Wm = (M + 63) / 64;
  const u64* rq = rows + (size_t)q * n1 * W;
  const int* oq = order + (size_t)q * n1;
  int* cq = clique + (size_t)q * n1;
  if (tid < PCR_TEASER_MAX_N1 / 64) bits_s[tid] = 0;
  if (tid == 0) best_s = -1;
  if (kLds) {
    for (int i = tid; i < M * W; i += kTCT)
      if (i % W < Wm) rows_s[i] = rq[i];
  }
  lds_barrier();
  auto row_word = [&](int r, int w) -> u64 {
    return kLds ? rows_s[(size_t)r * W + w] : rq[(size_t)r * W + w];
  };
  int g = 1;
  while (g < Wm) g <<= 1;  // Wm <= 64
  const int l = tid & (g - 1), groups = kTCT / g, gid = tid / g;
  const int S = seeds == 0 ? M : min(seeds, M);
  // size * 4096 + (4095 - seed): the largest clique, the best-ranked seed on ties
  int best = -1;
  for (int s0 = 0; s0 < S; s0 += groups) {
    const int seed = s0 + gid;
    const int size = teaser_walk(row_word, M, Wm, g, l, seed, seed < S, [](int) {});
    if (seed < S) best = max(best, size * 4096 + (4095 - seed));
  }
  if (l == 0 && best >= 0) atomicMax(&best_s, best);  // integers: order-free
  lds_barrier();
  best = best_s;
  const int K = best < 0 ? 0 : best >> 12;
  if (tid < kWave && best >= 0) {  // wave 0 walks the winner again; thread 0 marks the slots
    const int seed = 4095 - (best & 4095);
    auto mark = [&](int r) {
      if (tid == 0) {
        const int s = min(max(oq[r], 0), n1 - 1);
        bits_s[s >> 6] |= 1ull << (s & 63);
      }
    };
    mark(seed);
    teaser_walk(row_word, M, Wm, g, l, seed, true, mark);
  }
  lds_barrier();
  for (int s = tid; s < n1; s += kTCT) {
    if (s < M && ((bits_s[s >> 6] >> (s & 63)) & 1)) {
      int pos = __popcll(bits_s[s >> 6] & ((1ull << (s & 63)) - 1ull));
      for (int w = 0; w < (s >> 6); w++) pos += __popcll(bits_s[w]);
      cq[pos] = s;
    }
    if (s >= K) cq[s] = -1;
  }
  if (tid == 0) clique_size[q] = K;
}

// the larger of two values; a NaN stays
__device__ inline double teaser_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ inline double teaser_block_max(double v, double (*red_s)[16]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = teaser_max(v, __shfl_xor(v, off, kWave));
  if ((tid & (kWave - 1)) == 0) red_s[tid >> 6][0] = v;
  lds_barrier();
  v = red_s[0][0];
  for (int w = 1; w < kTSW; w++) v = teaser_max(v, red_s[w][0]);
  lds_barrier();
  return v;
}

// the vote's order: lower cost, then the earlier midpoint
__device__ inline bool teaser_better(double c, int r, double bc, int br) {
  return c < bc || (c == bc && r < br);
}

// Endpoint f (value vf) against endpoint e (value ve) in the order by value,
// then number: counts those before e into rank, keeps the first after e.
__device__ inline void teaser_place(double vf, int f, double ve, int e, double& sv, int& sf,
                                    int& rank) {
  const bool less = vf < ve || (vf == ve && f < e);
  const bool more = vf > ve || (vf == ve && f > e);
  rank += less ? 1 : 0;
  if (more && (vf < sv || (vf == sv && f < sf))) {
    sv = vf;
    sf = f;
  }
}

// f(i, j) for the TIMs i < j < K in row-major order, thread t taking the
// t-th, (t + kTST)-th, ... of them: at most K (K - 1) / 2 / kTST + 1 calls and
// K row steps.
template <typename F>
__device__ inline void teaser_tims(int K, F f) {
  int i = 0, c = threadIdx.x;
  for (;;) {
    while (i < K - 1 && c >= K - 1 - i) {
      c -= K - 1 - i;
      i++;
    }
    if (i >= K - 1) break;
    f(i, i + 1 + c);
    c += kTST;
  }
}

__global__ __launch_bounds__(kTST) void teaser_solve_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n1, int n2,
    const int* __restrict__ idx1, const int* __restrict__ idx2, const int* __restrict__ count,
    int select, double nu2, double rho, double gnc_factor, int max_iters, double cost_threshold,
    double* __restrict__ transform, int* __restrict__ clique, int* __restrict__ clique_size,
    int* __restrict__ inliers, int* __restrict__ num_inliers, int* __restrict__ iterations,
    int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char teaser_smem[];
  double* X_s = (double*)teaser_smem;                    // [n1]: one axis of the vote
  double(*red_s)[16] = (double(*)[16])(X_s + n1);        // [kTSW][16]
  float* pts = (float*)(red_s + kTSW);                   // [6][n1]: the clique's points
  __shared__ int cnt_s[kTSW];
  __shared__ unsigned inl_s[PCR_TEASER_MAX_N1 / 32];  // the inliers as a set of slots
  const int q = blockIdx.x, tid = threadIdx.x;
  const RigidPair pr = rigid_pair(xyz1, xyz2, n1, n2, idx1, idx2, count, q);
  int* cq = clique + (size_t)q * n1;
  int* iq = inliers + (size_t)q * n1;
  double* tq = transform + (size_t)q * 16;
  int K;
  if (select) {
    K = min(max(clique_size[q], 0), pr.m);
  } else {  // TEASER++'s NONE: every slot
    K = pr.m;
    for (int s = tid; s < n1; s += kTST) cq[s] = s < K ? s : -1;
    if (tid == 0) clique_size[q] = K;
  }
  if (tid < PCR_TEASER_MAX_N1 / 32) inl_s[tid] = 0;  // published by the barriers below
  if (K < PCR_TEASER_MIN_CLIQUE) {  // uniform
    for (int s = tid; s < n1; s += kTST) iq[s] = 0;
    rigid_store_identity(tq);
    if (tid == 0) {
      num_inliers[q] = 0;
      iterations[q] = 0;
      status[q] = 1;
    }
    return;
  }
  // a thread reads back only the entries of cq it wrote itself (select == 0)
  // or those of the clique kernel's launch
  teaser_stage(pr, select ? cq : nullptr, K, pts, kTST);
  lds_barrier();

  auto tim = [&](int i, int j, double* u, double* v) {
    float ai[3], bi[3], aj[3], bj[3];
    teaser_point(pts, n1, i, ai, bi);
    teaser_point(pts, n1, j, aj, bj);
    pcr_teaser_tim(ai, bi, aj, bj, u, v);
  };

  // every thread carries the same rotation
  double R[9], Rp[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, mup = 0.0;
  double sums[10];
#pragma unroll
  for (int i = 0; i < 10; i++) sums[i] = 0.0;
  teaser_tims(K, [&](int i, int j) {
    double u[3], v[3];
    tim(i, j, u, v);
    pcr_teaser_accumulate(u, v, 1.0, sums);
  });
  block_sum_d<kTSW>(sums, red_s);
  pcr_teaser_rotation(sums, R);
  int iters = 1, st = 0;
  double mx = 0.0;
  teaser_tims(K, [&](int i, int j) {
    double u[3], v[3];
    tim(i, j, u, v);
    mx = teaser_max(mx, pcr_teaser_r2(u, v, R));
  });
  mx = teaser_block_max(mx, red_s);
  if (!(mx < __builtin_inf())) {  // uniform: the same bits in every thread
    for (int s = tid; s < n1; s += kTST) iq[s] = 0;
    rigid_store_identity(tq);
    if (tid == 0) {
      num_inliers[q] = 0;
      iterations[q] = 1;
      status[q] = 2;
    }
    return;
  }
  double mu = pcr_teaser_mu0(mx, nu2);
  if (mu > 0.0 && mu < __builtin_inf()) {
    double prev = __builtin_inf();
    for (;;) {  // at most max_iters rounds: iters counts up to it
      // cost of R under the weights it was solved with (1, or those of Rp at
      // mup), the new weights, and the next H in one walk
      const bool unit = iters == 1;
#pragma unroll
      for (int i = 0; i < 10; i++) sums[i] = 0.0;
      teaser_tims(K, [&](int i, int j) {
        double u[3], v[3];
        tim(i, j, u, v);
        const double wo = unit ? 1.0 : pcr_teaser_weight(pcr_teaser_r2(u, v, Rp), mup, nu2);
        const double r2 = pcr_teaser_r2(u, v, R);
        sums[9] += wo * r2;
        pcr_teaser_accumulate(u, v, pcr_teaser_weight(r2, mu, nu2), sums);
      });
      block_sum_d<kTSW>(sums, red_s);
      const double diff = __builtin_fabs(sums[9] - prev);
      prev = sums[9];
      mup = mu;
      mu *= gnc_factor;
      if (diff < cost_threshold) break;
      if (iters >= max_iters) {
        st = 3;
        break;
      }
#pragma unroll
      for (int i = 0; i < 9; i++) Rp[i] = R[i];
      pcr_teaser_rotation(sums, R);
      iters++;
    }
  }

  // translation: per axis, the vote over the 2 K - 1 midpoints.  A thread
  // takes an endpoint, finds its place in the sorted list and its successor
  // by one pass over the others, and evaluates their midpoint.
  double t[3];
  constexpr int kMine = (PCR_TEASER_MAX_N1 + kTST - 1) / kTST;  // members a thread answers for
  unsigned keep = ~0u;  // bit i: member tid + i * kTST is inside on every axis so far
  for (int axis = 0; axis < 3; axis++) {
    // the axis' row of R picked without indexing R by a variable, which
    // would put R in scratch
    const double row[3] = {axis == 0 ? R[0] : axis == 1 ? R[3] : R[6],
                           axis == 0 ? R[1] : axis == 1 ? R[4] : R[7],
                           axis == 0 ? R[2] : axis == 1 ? R[5] : R[8]};
    for (int k = tid; k < K; k += kTST) {
      const float a[3] = {pts[k], pts[(size_t)n1 + k], pts[(size_t)2 * n1 + k]};
      X_s[k] = pcr_teaser_axis_row(row, a, pts[(size_t)(3 + axis) * n1 + k]);
    }
    lds_barrier();
    double bc = __builtin_inf(), bx = 0.0;
    int br = INT32_MAX;
    // kVL endpoints a thread and pass, so one read of X_s[k] serves them all
    for (int e0 = tid; e0 < 2 * K; e0 += kVL * kTST) {
      double ve[kVL], sv[kVL], m[kVL], x[kVL], c[kVL];
      int sf[kVL], rank[kVL];
#pragma unroll
      for (int j = 0; j < kVL; j++) {
        const int e = min(e0 + j * kTST, 2 * K - 1);  // a lane past the end repeats the last
        ve[j] = pcr_teaser_endpoint(X_s, e, rho);
        sv[j] = __builtin_inf();
        sf[j] = INT32_MAX;
        rank[j] = 0;
      }
      for (int k = 0; k < K; k++) {
        const double lo = pcr_teaser_endpoint(X_s, 2 * k, rho);
        const double hi = pcr_teaser_endpoint(X_s, 2 * k + 1, rho);
#pragma unroll
        for (int j = 0; j < kVL; j++) {
          const int e = min(e0 + j * kTST, 2 * K - 1);
          teaser_place(lo, 2 * k, ve[j], e, sv[j], sf[j], rank[j]);
          teaser_place(hi, 2 * k + 1, ve[j], e, sv[j], sf[j], rank[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < kVL; j++)  // the last endpoint starts no midpoint: any finite value
        m[j] = rank[j] < 2 * K - 1 ? pcr_teaser_midpoint(ve[j], sv[j]) : ve[j];
      pcr_teaser_vote_lanes(X_s, K, m, rho, x, c);
#pragma unroll
      for (int j = 0; j < kVL; j++) {
        if (e0 + j * kTST < 2 * K && rank[j] < 2 * K - 1 && teaser_better(c[j], rank[j], bc, br)) {
          bc = c[j];
          br = rank[j];
          bx = x[j];
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double oc = __shfl_xor(bc, off, kWave), ox = __shfl_xor(bx, off, kWave);
      const int orank = __shfl_xor(br, off, kWave);
      if (teaser_better(oc, orank, bc, br)) {
        bc = oc;
        br = orank;
        bx = ox;
      }
    }
    if ((tid & (kWave - 1)) == 0) {
      red_s[tid >> 6][0] = bc;
      red_s[tid >> 6][1] = bx;
      red_s[tid >> 6][2] = (double)br;  // < 2^13: exact
    }
    lds_barrier();
    bc = red_s[0][0];
    bx = red_s[0][1];
    br = (int)red_s[0][2];
    for (int w = 1; w < kTSW; w++) {
      if (teaser_better(red_s[w][0], (int)red_s[w][2], bc, br)) {
        bc = red_s[w][0];
        bx = red_s[w][1];
        br = (int)red_s[w][2];
      }
    }
    if (axis == 0) t[0] = bx;
    if (axis == 1) t[1] = bx;
    if (axis == 2) t[2] = bx;
#pragma unroll
    for (int i = 0; i < kMine; i++) {
      const int k = tid + i * kTST;
      if (k < K && !(__builtin_fabs(X_s[k] - bx) <= rho)) keep &= ~(1u << i);
    }
    lds_barrier();  // X_s and red_s are rewritten by the next axis
  }

  int mine = 0;
#pragma unroll
  for (int i = 0; i < kMine; i++) {
    const int k = tid + i * kTST;
    if (k < K && ((keep >> i) & 1u)) {
      const int s = select ? min(max(cq[k], 0), n1 - 1) : k;
      atomicOr(&inl_s[s >> 5], 1u << (s & 31));  // integers: order-free
      mine++;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, kWave);
  if ((tid & (kWave - 1)) == 0) cnt_s[tid >> 6] = mine;
  lds_barrier();
  for (int s = tid; s < n1; s += kTST) iq[s] = (int)((inl_s[s >> 5] >> (s & 31)) & 1u);
  if (tid == 0) {
    double out[16];
    int total = 0;
    for (int w = 0; w < kTSW; w++) total += cnt_s[w];
    pcr_teaser_report(R, t, out);
#pragma unroll
    for (int i = 0; i < 16; i++) tq[i] = out[i];
    num_inliers[q] = total;
    iterations[q] = iters;
    status[q] = st;
  }
}

}  // namespace pcr

using namespace pcr;

extern "C" size_t pcr_teaser_workspace_size(int p, int n1) {
  if (p <= 0 || n1 <= 0 || n1 > PCR_TEASER_MAX_N1) return 256;
  return teaser_ws_bytes(p, n1);
}

extern "C" pcr_status pcr_teaser(const float* xyz1, const float* xyz2, int p, int n1, int n2,
                                 const int* idx1, const int* idx2, const int* count,
                                 double noise_bound, double cbar2, double gnc_factor,
                                 int max_iters, double cost_threshold, int seeds,
                                 int inlier_selection, double* transform, int* clique,
                                 int* clique_size, int* inliers, int* num_inliers,
                                 int* iterations, int* status, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  PCR_REQUIRE(p >= 0 && n1 >= 1 && n2 >= 1, "teaser: invalid sizes");
  PCR_REQUIRE(n1 <= PCR_TEASER_MAX_N1, "teaser: n1 (%d) above %d: the graph is n1 * n1 bits a pair",
              n1, PCR_TEASER_MAX_N1);
  PCR_REQUIRE(noise_bound > 0.0 && noise_bound < __builtin_inf(),
              "teaser: noise_bound must be positive and finite");
  PCR_REQUIRE(cbar2 > 0.0 && cbar2 < __builtin_inf(), "teaser: cbar2 must be positive and finite");
  PCR_REQUIRE(gnc_factor > 1.0, "teaser: gnc_factor must exceed 1");
  PCR_REQUIRE(max_iters >= 1 && max_iters <= PCR_TEASER_MAX_ITERS,
              "teaser: max_iters (%d) outside [1, %d]", max_iters, PCR_TEASER_MAX_ITERS);
  PCR_REQUIRE(cost_threshold >= 0.0, "teaser: negative or NaN cost_threshold");
  PCR_REQUIRE(seeds >= 0, "teaser: negative seeds");
  if (p == 0) return PCR_OK;
  PCR_REQUIRE(xyz1 && xyz2 && idx1 && idx2 && count && transform && clique && clique_size &&
                  inliers && num_inliers && iterations && status,
              "teaser: null pointer");
  const size_t need = teaser_ws_bytes(p, n1);
  PCR_REQUIRE(workspace != nullptr && workspace_bytes >= need,
              "teaser: workspace too small (%zu < %zu)", workspace_bytes, need);
  const double bound = noise_bound * __builtin_sqrt(cbar2);
  const double beta = 2.0 * bound, rho = bound;
  hipStream_t st = as_stream(stream);
  const int W = teaser_words(n1);
  u64* rows = (u64*)workspace;
  int* deg = (int*)(rows + (size_t)p * n1 * W);
  int* order = deg + (size_t)p * n1;
  if (inlier_selection) {
    const size_t glds = (size_t)n1 * 6 * sizeof(float);
    const dim3 ggrid(p, ceil_div(n1, kTGRows));
    allow_big_lds(teaser_graph_kernel<false>, glds);
    allow_big_lds(teaser_graph_kernel<true>, glds);
    hipLaunchKernelGGL(teaser_graph_kernel<false>, ggrid, dim3(kTGT), glds, st, xyz1, xyz2, n1, n2,
                       idx1, idx2, count, beta, W, (const int*)nullptr, deg, (u64*)nullptr);
    hipLaunchKernelGGL(teaser_rank_kernel, dim3(p), dim3(kTRT), (size_t)n1 * sizeof(int), st, count,
                       n1, deg, order);
    hipLaunchKernelGGL(teaser_graph_kernel<true>, ggrid, dim3(kTGT), glds, st, xyz1, xyz2, n1, n2,
                       idx1, idx2, count, beta, W, order, (int*)nullptr, rows);
    if (n1 <= kTCLds) {
      const size_t clds = (size_t)n1 * W * sizeof(u64);
      allow_big_lds(teaser_clique_kernel<true>, clds);
      hipLaunchKernelGGL(teaser_clique_kernel<true>, dim3(p), dim3(kTCT), clds, st, count, n1, W,
                         seeds, order, rows, clique, clique_size);
    } else {
      hipLaunchKernelGGL(teaser_clique_kernel<false>, dim3(p), dim3(kTCT), 0, st, count, n1, W,
                         seeds, order, rows, clique, clique_size);
    }
  }
  const size_t slds = teaser_solve_lds(n1);
  allow_big_lds(teaser_solve_kernel, slds);
  hipLaunchKernelGGL(teaser_solve_kernel, dim3(p), dim3(kTST), slds, st, xyz1, xyz2, n1, n2, idx1,
                     idx2, count, inlier_selection ? 1 : 0, beta * beta, rho, gnc_factor, max_iters,
                     cost_threshold, transform, clique, clique_size, inliers, num_inliers,
                     iterations, status);
  return launch_status("teaser");
}
