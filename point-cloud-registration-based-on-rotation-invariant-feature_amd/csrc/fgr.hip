// fgr.hip -- batched Fast Global Registration for gfx950: the reference's
// register_one_pair(func='fgr') (utils/open3d_func.py:34-75, Open3D
// registration_fast_based_on_feature_matching on the CPU, one pair at a
// time), from the mutual-NN correspondences of the matching.  The contract is
// DESIGN.md 4.8c, the scalar math include/pcr_fgr.h + pcr_rigid.h.
//
//   fgr_tuple_kernel  one workgroup per pair builds the correspondence list L.
//     Tuple test: rounds of kFTT trials, one per thread -- the triple of
//     pcr_rigid_triple, its six points gathered through idx1 / idx2, the fp64
//     edge-length check; a block scan compacts the accepted trials in
//     ascending h behind those of the earlier rounds, and the walk stops with
//     the round that reaches max_tuples.  No atomics: the list is the first
//     max_tuples accepted trials whatever the launch shape.  max_tuples = 0:
//     L is the slots themselves.  Besides `slots` it leaves the fp32 point
//     pairs of L in the workspace as six planes, so the loop never gathers.
//   fgr_gnc_kernel    one workgroup per pair runs the whole graduated
//     non-convexity loop.  Prologue: the clouds' fp64 centroids and the scale.
//     Up to kFCap correspondences lie in LDS normalised, as six fp64 planes
//     (a lane reads consecutive 8-byte words: no bank conflict); a longer list
//     is re-read from the workspace and normalised on the fly every
//     iteration.  The 16 moment sums are per-thread fp64 sums in ascending
//     order, a fixed shuffle butterfly, the waves in order (the scheme of
//     rigid_refit_kernel): no float atomics, the same bits every run, and the
//     same bits in every thread, so each thread takes the step itself
//     (pcr_fgr_step): a solve by wave 0 alone with a hand-off through LDS
//     costs a barrier more per iteration and, compiled, spills registers.
#include "common.hpp"
#include "pcr_fgr.h"
#include "rigid_pair.hpp"

namespace pcr {

constexpr int kFTT = 1024;            // tuple kernel: threads = trials per round
constexpr int kFT = PCR_FGR_THREADS;  // loop kernel: threads per workgroup
constexpr int kFW = kFT / kWave;
constexpr int kFCap = 3072;           // correspondences resident in LDS (48 bytes each: 144 KB)
static_assert(kFT % kWave == 0 && kFTT % kWave == 0 && kFTT <= 1024, "fgr launch shape");

inline int fgr_kcap(int n1, int max_tuples) { return max_tuples > 0 ? 3 * max_tuples : n1; }
inline size_t fgr_ws_bytes(int p, int kcap) {
  return align_up((size_t)p * 6 * (size_t)kcap * sizeof(float), 256);
}
inline size_t fgr_lds_bytes(int cap) {
  return (size_t)cap * 6 * sizeof(double) + (size_t)kFW * 16 * sizeof(double);
}

__global__ __launch_bounds__(kFTT) void fgr_tuple_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n1, int n2,
    const int* __restrict__ idx1, const int* __restrict__ idx2, const int* __restrict__ count,
    int max_tuples, int trials_per_corr, float rho, unsigned seed, int kcap,
    int* __restrict__ slots, int* __restrict__ num_corr, int* __restrict__ num_trials,
    float* __restrict__ pts) {
  __shared__ int scan_s[kFTT / kWave + 1];
  __shared__ int tot_s, last_s;
  const int q = blockIdx.x, tid = threadIdx.x;
  const RigidPair pr = rigid_pair(xyz1, xyz2, n1, n2, idx1, idx2, count, q);
  int* sl = slots + (size_t)q * kcap;
  float* pt = pts + (size_t)q * 6 * kcap;
  if (max_tuples == 0) {  // the slots as they are (kcap = n1)
    for (int s = tid; s < kcap; s += kFTT) {
      sl[s] = s < pr.m ? s : -1;
      if (s < pr.m) {
        float a[3], b[3];
        rigid_slot(pr, s, a, b);
#pragma unroll
        for (int d = 0; d < 3; d++) {
          pt[(size_t)d * kcap + s] = a[d];
          pt[(size_t)(3 + d) * kcap + s] = b[d];
        }
      }
    }
    if (tid == 0) {
      num_corr[q] = pr.m;
      num_trials[q] = 0;
    }
    return;
  }
  const long long H = (long long)trials_per_corr * pr.m;  // <= INT_MAX (host check)
  int accepted = 0;  // uniform over the workgroup
  if (pr.m >= 3) {
    for (long long h0 = 0; h0 < H && accepted < max_tuples; h0 += kFTT) {
      const long long h = h0 + tid;
      int s3[3], ok = 0;
      float a[9], b[9];
      if (h < H) {
        pcr_rigid_triple(seed, (unsigned)q, (unsigned)h, (unsigned)pr.m, s3);
#pragma unroll
        for (int k = 0; k < 3; k++) rigid_slot(pr, s3[k], a + 3 * k, b + 3 * k);
        ok = pcr_rigid_edge_ok(a, b, rho);
      }
      const int incl = block_inclusive_scan(ok, scan_s);
      const int pos = accepted + incl - 1;  // this trial's rank among the accepted
      if (ok && pos < max_tuples) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          sl[3 * pos + k] = s3[k];
#pragma unroll
          for (int d = 0; d < 3; d++) {
            pt[(size_t)d * kcap + 3 * pos + k] = a[3 * k + d];
            pt[(size_t)(3 + d) * kcap + 3 * pos + k] = b[3 * k + d];
          }
        }
        if (pos == max_tuples - 1) last_s = (int)h;  // one thread of one round
      }
      if (tid == kFTT - 1) tot_s = incl;
      lds_barrier();
      accepted += tot_s;  // the next write of tot_s lies behind the scan's barriers
    }
  }
  const bool full = accepted >= max_tuples;
  const int K = 3 * (full ? max_tuples : accepted);
  for (int s = K + tid; s < kcap; s += kFTT) sl[s] = -1;
  if (tid == 0) {
    num_corr[q] = K;
    num_trials[q] = full ? last_s + 1 : (int)H;
  }
}

// the larger of two norms; a NaN stays
__device__ inline double fgr_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ inline double fgr_block_max(double v, double (*red_s)[16]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fgr_max(v, __shfl_xor(v, off, kWave));
  if ((tid & (kWave - 1)) == 0) red_s[tid >> 6][0] = v;
  lds_barrier();
  v = red_s[0][0];
  for (int w = 1; w < kFW; w++) v = fgr_max(v, red_s[w][0]);
  lds_barrier();
  return v;
}

// RG: the ragged pack of common.hpp.  The centroids, their
// divisors and the scale run over the valid points v1 / v2; pcr_fgr_sum's
// order depends on the index alone, so a pair gives the bits of the dense
// kernel on the pair trimmed to its counts.  An empty cloud has no scale:
// status 2.
template <typename... RG>
__global__ __launch_bounds__(kFT) void fgr_gnc_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n1, int n2,
    const float* __restrict__ pts, const int* __restrict__ num_corr, int kcap, int cap,
    double max_corr_dist, int iterations, double division_factor, int decrease_mu,
    int absolute_scale, double* __restrict__ transform, double* __restrict__ mu_out,
    int* __restrict__ status, RG... rg) {
  extern __shared__ __attribute__((aligned(16))) char fgr_smem[];
  double* pq_s = (double*)fgr_smem;  // [6][cap]: p x y z, q0 x y z
  double(*red_s)[16] = (double(*)[16])(pq_s + (size_t)6 * cap);
  const int q = blockIdx.x, tid = threadIdx.x;
  const float* A = xyz1 + (size_t)q * 3 * n1;
  const float* B = xyz2 + (size_t)q * 3 * n2;
  const float* pt = pts + (size_t)q * 6 * kcap;
  double* tq = transform + (size_t)q * 16;
  const int K = num_corr[q];
  const bool resident = K <= cap;
  int v1 = n1, v2 = n2;
  ragged_valid(q, v1, v2, rg...);

  double m1[3], m2[3], s = 0.0;
  int st = 0;
  if (K < PCR_FGR_MIN_CORR) {  // uniform
    st = 1;
  } else {
    // centroids: per-thread sums in ascending i, then the block sum
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < v1; i += kFT) {
#pragma unroll
      for (int d = 0; d < 3; d++) acc[d] += (double)A[(size_t)d * n1 + i];
    }
    for (int i = tid; i < v2; i += kFT) {
#pragma unroll
      for (int d = 0; d < 3; d++) acc[3 + d] += (double)B[(size_t)d * n2 + i];
    }
    block_sum_d<kFW>(acc, red_s);
#pragma unroll
    for (int d = 0; d < 3; d++) {
      m1[d] = acc[d] / (double)v1;
      m2[d] = acc[3 + d] / (double)v2;
    }
    for (int i = tid; i < v1; i += kFT)
      s = fgr_max(s, pcr_fgr_norm(A[i], A[(size_t)n1 + i], A[(size_t)2 * n1 + i], m1));
    for (int i = tid; i < v2; i += kFT)
      s = fgr_max(s, pcr_fgr_norm(B[i], B[(size_t)n2 + i], B[(size_t)2 * n2 + i], m2));
    s = fgr_block_max(s, red_s);
    if (!(s > 0.0 && s < __builtin_inf())) st = 2;  // uniform: the same bits in every thread
    if (sizeof...(RG) != 0 && (v1 == 0 || v2 == 0)) st = 2;
  }
  if (st) {
    rigid_store_identity(tq);
    if (tid == 0) {
      mu_out[q] = 0.0;
      status[q] = st;
    }
    return;
  }
  const double dn = absolute_scale ? 1.0 : s;
  double mu = absolute_scale ? s : 1.0;

  // one correspondence of L in normalised units
  auto fetch = [&](int c, double* p, double* q0) {
    if (resident) {
#pragma unroll
      for (int d = 0; d < 3; d++) {
        p[d] = pq_s[(size_t)d * cap + c];
        q0[d] = pq_s[(size_t)(3 + d) * cap + c];
      }
    } else {
      float a[3], b[3];
#pragma unroll
      for (int d = 0; d < 3; d++) {
        a[d] = pt[(size_t)d * kcap + c];
        b[d] = pt[(size_t)(3 + d) * kcap + c];
      }
      pcr_fgr_unit(a, m1, dn, p);
      pcr_fgr_unit(b, m2, dn, q0);
    }
  };
  if (resident) {
    for (int c = tid; c < K; c += kFT) {
      float a[3], b[3];
      double p[3], q0[3];
#pragma unroll
      for (int d = 0; d < 3; d++) {
        a[d] = pt[(size_t)d * kcap + c];
        b[d] = pt[(size_t)(3 + d) * kcap + c];
      }
      pcr_fgr_unit(a, m1, dn, p);
      pcr_fgr_unit(b, m2, dn, q0);
#pragma unroll
      for (int d = 0; d < 3; d++) {
        pq_s[(size_t)d * cap + c] = p[d];
        pq_s[(size_t)(3 + d) * cap + c] = q0[d];
      }
    }
    lds_barrier();
  }

  // every thread carries the same transform
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  for (int it = 0; it < iterations; it++) {
    double sums[PCR_FGR_NSUM];
#pragma unroll
    for (int i = 0; i < PCR_FGR_NSUM; i++) sums[i] = 0.0;
    for (int c = tid; c < K; c += kFT) {
      double p[3], q0[3];
      fetch(c, p, q0);
      pcr_fgr_accumulate(p, q0, R, t, mu, sums);
    }
    block_sum_d<kFW>(sums, red_s);
    // the sums are the same bits in every thread, so every thread takes the
    // same step: no hand-off, and the exit below is uniform
    if (pcr_fgr_step(sums, R, t)) {
      st = 3;
      break;
    }
    if (decrease_mu && it % 4 == 0 && mu > max_corr_dist) mu /= division_factor;
  }

  if (tid == 0) {
    double out[16];
    pcr_fgr_report(R, t, m1, m2, dn, out);
#pragma unroll
    for (int i = 0; i < 16; i++) tq[i] = out[i];
    mu_out[q] = mu;
    status[q] = st;
  }
}

}  // namespace pcr

using namespace pcr;

extern "C" size_t pcr_fgr_workspace_size(int p, int n1, int max_tuples) {
  if (p <= 0 || n1 <= 0 || max_tuples < 0 || max_tuples > INT32_MAX / 3) return 256;
  return fgr_ws_bytes(p, fgr_kcap(n1, max_tuples));
}

// both entry points: counts1 / counts2 are read only when `ragged`
static pcr_status fgr_run(bool ragged, const float* xyz1, const float* xyz2, int p, int n1, int n2,
                          const int* counts1, const int* counts2, const int* idx1,
                          const int* idx2, const int* count, double max_corr_dist, int iterations,
                          double division_factor, int decrease_mu, float tuple_scale,
                          int max_tuples, int trials_per_corr, int absolute_scale, unsigned seed,
                          double* transform, int* slots, int* num_corr, int* num_trials,
                          double* mu, int* status, void* workspace, size_t workspace_bytes,
                          void* stream) {
  PCR_REQUIRE(p >= 0 && n1 >= 1 && n2 >= 1, "fgr: invalid sizes");
  PCR_REQUIRE(iterations >= 0 && iterations <= PCR_FGR_MAX_ITERS,
              "fgr: iterations (%d) outside [0, %d]", iterations, PCR_FGR_MAX_ITERS);
  PCR_REQUIRE(division_factor > 1.0, "fgr: division_factor must exceed 1");
  PCR_REQUIRE(max_corr_dist >= 0.0, "fgr: negative or NaN max_corr_dist");
  PCR_REQUIRE(tuple_scale >= 0.0f && tuple_scale < 1.0f, "fgr: tuple_scale outside [0, 1)");
  PCR_REQUIRE(max_tuples >= 0 && max_tuples <= INT32_MAX / 3, "fgr: invalid max_tuples (%d)",
              max_tuples);
  PCR_REQUIRE(trials_per_corr >= 0, "fgr: negative trials_per_corr");
  PCR_REQUIRE(max_tuples == 0 || (long long)trials_per_corr * n1 <= INT32_MAX,
              "fgr: trials_per_corr * n1 (%d * %d) passes 2^31 - 1", trials_per_corr, n1);
  if (p == 0) return PCR_OK;
  PCR_REQUIRE(xyz1 && xyz2 && idx1 && idx2 && count && transform && slots && num_corr &&
                  num_trials && mu && status,
              "fgr: null pointer");
  const int kcap = fgr_kcap(n1, max_tuples);
  const size_t need = fgr_ws_bytes(p, kcap);
  PCR_REQUIRE(workspace != nullptr && workspace_bytes >= need,
              "fgr: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  float* pts = (float*)workspace;
  hipLaunchKernelGGL(fgr_tuple_kernel, dim3(p), dim3(kFTT), 0, st, xyz1, xyz2, n1, n2, idx1, idx2,
                     count, max_tuples, trials_per_corr, tuple_scale, seed, kcap, slots, num_corr,
                     num_trials, pts);
  const int cap = min(kcap, kFCap);
  const size_t lds = fgr_lds_bytes(cap);
  if (ragged) {
    const RaggedCounts rc = {counts1, counts2};
    allow_big_lds(fgr_gnc_kernel<RaggedCounts>, lds);
    hipLaunchKernelGGL(fgr_gnc_kernel<RaggedCounts>, dim3(p), dim3(kFT), lds, st, xyz1, xyz2, n1,
                       n2, pts, num_corr, kcap, cap, max_corr_dist, iterations, division_factor,
                       decrease_mu, absolute_scale, transform, mu, status, rc);
  } else {
    allow_big_lds(fgr_gnc_kernel<>, lds);
    hipLaunchKernelGGL(fgr_gnc_kernel<>, dim3(p), dim3(kFT), lds, st, xyz1, xyz2, n1, n2, pts,
                       num_corr, kcap, cap, max_corr_dist, iterations, division_factor, decrease_mu,
                       absolute_scale, transform, mu, status);
  }
  return launch_status("fgr");
}

extern "C" pcr_status pcr_fgr(const float* xyz1, const float* xyz2, int p, int n1, int n2,
                              const int* idx1, const int* idx2, const int* count,
                              double max_corr_dist, int iterations, double division_factor,
                              int decrease_mu, float tuple_scale, int max_tuples,
                              int trials_per_corr, int absolute_scale, unsigned seed,
                              double* transform, int* slots, int* num_corr, int* num_trials,
                              double* mu, int* status, void* workspace, size_t workspace_bytes,
                              void* stream) {
  return fgr_run(false, xyz1, xyz2, p, n1, n2, nullptr, nullptr, idx1, idx2, count, max_corr_dist,
                 iterations, division_factor, decrease_mu, tuple_scale, max_tuples,
                 trials_per_corr, absolute_scale, seed, transform, slots, num_corr, num_trials, mu,
                 status, workspace, workspace_bytes, stream);
}

extern "C" pcr_status pcr_fgr_ragged(const float* xyz1, const float* xyz2, int p, int n1, int n2,
                                     const int* counts1, const int* counts2, const int* idx1,
                                     const int* idx2, const int* count, double max_corr_dist,
                                     int iterations, double division_factor, int decrease_mu,
                                     float tuple_scale, int max_tuples, int trials_per_corr,
                                     int absolute_scale, unsigned seed, double* transform,
                                     int* slots, int* num_corr, int* num_trials, double* mu,
                                     int* status, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return fgr_run(true, xyz1, xyz2, p, n1, n2, counts1, counts2, idx1, idx2, count, max_corr_dist,
                 iterations, division_factor, decrease_mu, tuple_scale, max_tuples,
                 trials_per_corr, absolute_scale, seed, transform, slots, num_corr, num_trials, mu,
                 status, workspace, workspace_bytes, stream);
}
