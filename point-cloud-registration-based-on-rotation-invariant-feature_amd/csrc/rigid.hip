// rigid.hip -- batched rigid-transform estimation from the mutual-NN
// correspondences, for gfx950: the step after the matching in the reference's
// registration evaluation (datasets/deepgmr_mn40.py:165-231 register_one_pair,
// there Open3D RANSAC on the CPU, one pair at a time).  A seeded, deterministic
// RANSAC -- 3-point closed-form solve, edge-length check, inlier count -- and
// a least-squares refit on the inliers; the contract is DESIGN.md 4.8a, the
// scalar math include/pcr_rigid.h.
//
//   rigid_hyp_kernel    one workgroup per (pair, block of 256 hypotheses):
//     one hypothesis per thread is drawn and edge-checked; the survivors
//     (typically 6-15 % at edge_ratio 0.9) are compacted in ascending h, solved
//     on dense lanes, and scored against the pair's correspondences, staged
//     through LDS in chunks of kRChunk slots.  The scoring threads are laid
//     out as (survivor, slot segment): the lanes of one segment read the same
//     LDS address (a broadcast), neighbouring segments neighbouring banks.
//     Counts meet in integer LDS atomics; the block's best (score, lowest h)
//     goes to the workspace.
//   rigid_refit_kernel  one workgroup per pair: best block result, its
//     transform again, refine_iters rounds of mask + fp64 least squares (per
//     thread strided partial sums in ascending slot order, a fixed shuffle
//     tree, the four waves in order: no float atomics, the same bits every
//     run), then the mask and count under the final transform.
#include "common.hpp"
#include "pcr_rigid.h"
#include "rigid_pair.hpp"

namespace pcr {

constexpr int kRB = 256;       // threads = hypotheses per workgroup
constexpr int kRChunk = 1024;  // correspondence slots per LDS chunk (6 floats each: 24 KB)
constexpr int kRW = kRB / kWave;

// block result key: larger is better -- score first, then the lower h; 0: none
__device__ inline unsigned long long rigid_key(int score, int h) {
  return ((unsigned long long)(unsigned)(score + 1) << 32) | (0xFFFFFFFFu - (unsigned)h);
}

__global__ __launch_bounds__(kRB) void rigid_hyp_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n1, int n2,
    const int* __restrict__ idx1, const int* __restrict__ idx2, const int* __restrict__ count,
    int hyps, float tau2, float rho, unsigned seed, int* __restrict__ scores,
    unsigned long long* __restrict__ wsbest) {
  __shared__ float pts_s[6][kRChunk];
  __shared__ float t_s[kRB][13];  // survivors' fp32 transforms (odd stride: no bank conflicts)
  __shared__ int hyp_s[kRB];
  __shared__ int cnt_s[kRB];
  __shared__ int scan_s[kRW + 1];
  __shared__ int nsurv_s;
  __shared__ unsigned long long best_s[kRW];
  const int q = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  const int h = g * kRB + tid;
  const RigidPair pr = rigid_pair(xyz1, xyz2, n1, n2, idx1, idx2, count, q);
  int* sc = scores ? scores + (size_t)q * hyps : nullptr;
  unsigned long long* out = wsbest + (size_t)q * gridDim.y + g;
  if (pr.m < 3) {  // uniform over the workgroup
    if (sc && h < hyps) sc[h] = -1;
    if (tid == 0) *out = 0ull;
    return;
  }
  // draw and edge-check one hypothesis per thread; survivors in ascending h
  int ok = 0;
  if (h < hyps) {
    float a[9], b[9];
    rigid_triple_points(pr, seed, q, h, a, b);
    ok = pcr_rigid_edge_ok(a, b, rho);
    if (sc && !ok) sc[h] = -1;
  }
  const int incl = block_inclusive_scan(ok, scan_s);
  if (ok) hyp_s[incl - 1] = h;
  if (tid == kRB - 1) nsurv_s = incl;
  cnt_s[tid] = 0;
  lds_barrier();
  const int ns = nsurv_s;
  if (ns == 0) {  // uniform
    if (tid == 0) *out = 0ull;
    return;
  }
  if (tid < ns) {
    float a[9], b[9], T[12];
    double R[9], t[3];
    rigid_triple_points(pr, seed, q, hyp_s[tid], a, b);
    pcr_rigid_solve3(a, b, R, t);
    pcr_rigid_round(R, t, T);
#pragma unroll
    for (int i = 0; i < 12; i++) t_s[tid][i] = T[i];
  }
  lds_barrier();
  // score: thread = (survivor sv, slot segment seg), seg strides the chunk
  const int nseg = kRB / ns;
  const int sv = tid % ns, seg = tid / ns;
  const bool active = seg < nseg;
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = t_s[sv][i];
  int c = 0;
  for (int s0 = 0; s0 < pr.m; s0 += kRChunk) {
    const int len = min(kRChunk, pr.m - s0);
    for (int s = tid; s < len; s += kRB) {
      float a[3], b[3];
      rigid_slot(pr, s0 + s, a, b);
#pragma unroll
      for (int d = 0; d < 3; d++) {
        pts_s[d][s] = a[d];
        pts_s[3 + d][s] = b[d];
      }
    }
    lds_barrier();
    if (active)
      for (int s = seg; s < len; s += nseg)
        c += pcr_rigid_resid2(T, pts_s[0][s], pts_s[1][s], pts_s[2][s], pts_s[3][s], pts_s[4][s],
                              pts_s[5][s]) <= tau2
                 ? 1
                 : 0;
    lds_barrier();
  }
  if (active && c) atomicAdd(&cnt_s[sv], c);
  lds_barrier();
  unsigned long long key = 0ull;
  if (tid < ns) {
    const int score = cnt_s[tid], hh = hyp_s[tid];
    if (sc) sc[hh] = score;
    key = rigid_key(score, hh);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = shfl_xor_u64(key, off);
    key = o > key ? o : key;
  }
  if ((tid & (kWave - 1)) == 0) best_s[tid >> 6] = key;
  lds_barrier();
  if (tid == 0) {
    for (int w = 1; w < kRW; w++) key = best_s[w] > key ? best_s[w] : key;
    *out = key;
  }
}

__global__ __launch_bounds__(kRB) void rigid_refit_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n1, int n2,
    const int* __restrict__ idx1, const int* __restrict__ idx2, const int* __restrict__ count,
    int nblocks, float tau2, int refine_iters, unsigned seed,
    const unsigned long long* __restrict__ wsbest, double* __restrict__ transform,
    int* __restrict__ inliers, int* __restrict__ num_inliers, int* __restrict__ best_hyp,
    int* __restrict__ status) {
  __shared__ double red_s[kRW][16];
  __shared__ int cnt_s[kRW];
  const int q = blockIdx.x, tid = threadIdx.x;
  const RigidPair pr = rigid_pair(xyz1, xyz2, n1, n2, idx1, idx2, count, q);
  double* tq = transform + (size_t)q * 16;
  int* inl = inliers + (size_t)q * n1;
  int st = 0, bh = -1;
  if (pr.m < 3) {
    st = 1;
  } else {
    unsigned long long key = 0ull;
    for (int g = 0; g < nblocks; g++) {
      const unsigned long long o = wsbest[(size_t)q * nblocks + g];
      key = o > key ? o : key;
    }
    if (key == 0ull)
      st = 2;
    else
      bh = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
  }
  if (st) {  // uniform: identity, no inliers
    for (int s = tid; s < n1; s += kRB) inl[s] = 0;
    rigid_store_identity(tq);
    if (tid == 0) {
      num_inliers[q] = 0;
      best_hyp[q] = -1;
      status[q] = st;
    }
    return;
  }
  // every thread carries the same transform (same inputs, same operations)
  double R[9], t[3];
  float T[12];
  {
    float a[9], b[9];
    rigid_triple_points(pr, seed, q, bh, a, b);
    pcr_rigid_solve3(a, b, R, t);
    pcr_rigid_round(R, t, T);
  }
  for (int it = 0; it < refine_iters; it++) {
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = tid; s < pr.m; s += kRB) {
      float a[3], b[3];
      rigid_slot(pr, s, a, b);
      if (pcr_rigid_resid2(T, a[0], a[1], a[2], b[0], b[1], b[2]) <= tau2) {
        acc[0] += 1.0;
#pragma unroll
        for (int d = 0; d < 3; d++) {
          acc[1 + d] += (double)a[d];
          acc[4 + d] += (double)b[d];
        }
      }
    }
    block_sum_d<kRW>(acc, red_s);
    if (acc[0] < 3.0) break;  // uniform
    double ca[3], cb[3], cov[9];
#pragma unroll
    for (int d = 0; d < 3; d++) {
      ca[d] = acc[1 + d] / acc[0];
      cb[d] = acc[4 + d] / acc[0];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) cov[i] = 0.0;
    for (int s = tid; s < pr.m; s += kRB) {
      float a[3], b[3];
      rigid_slot(pr, s, a, b);
      if (pcr_rigid_resid2(T, a[0], a[1], a[2], b[0], b[1], b[2]) <= tau2) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++)
            cov[3 * i + j] += ((double)a[i] - ca[i]) * ((double)b[j] - cb[j]);
      }
    }
    block_sum_d<kRW>(cov, red_s);
    pcr_rigid_from_cov(ca, cb, cov, R, t);
    pcr_rigid_round(R, t, T);
  }
  // the mask and the count under the final transform
  int c = 0;
  for (int s = tid; s < n1; s += kRB) {
    int m = 0;
    if (s < pr.m) {
      float a[3], b[3];
      rigid_slot(pr, s, a, b);
      m = pcr_rigid_resid2(T, a[0], a[1], a[2], b[0], b[1], b[2]) <= tau2 ? 1 : 0;
    }
    inl[s] = m;
    c += m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
  if ((tid & (kWave - 1)) == 0) cnt_s[tid >> 6] = c;
  lds_barrier();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < kRW; w++) tot += cnt_s[w];
    num_inliers[q] = tot;
    best_hyp[q] = bh;
    status[q] = 0;
    rigid_store_transform(tq, R, t);
  }
}

static size_t rigid_ws_bytes(int p, int hyps) {
  const size_t nb = (size_t)ceil_div(hyps, kRB);
  return ((size_t)p * nb * 8 + 255) / 256 * 256;
}

}  // namespace pcr

using namespace pcr;

extern "C" size_t pcr_rigid_ransac_workspace_size(int p, int n1, int hyps) {
  (void)n1;
  if (p <= 0 || hyps <= 0) return 256;
  return rigid_ws_bytes(p, hyps);
}

extern "C" pcr_status pcr_rigid_ransac(const float* xyz1, const float* xyz2, int p, int n1, int n2,
                                       const int* idx1, const int* idx2, const int* count,
                                       int hyps, float inlier_dist, float edge_ratio,
                                       int refine_iters, unsigned seed, double* transform,
                                       int* inliers, int* num_inliers, int* best_hyp, int* scores,
                                       int* status, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  PCR_REQUIRE(p >= 0 && n1 >= 1 && n2 >= 1, "rigid_ransac: invalid sizes");
  PCR_REQUIRE(hyps >= 1 && ceil_div(hyps, kRB) <= 65535, "rigid_ransac: invalid hyps (%d)", hyps);
  PCR_REQUIRE(inlier_dist > 0.0f, "rigid_ransac: inlier_dist must be positive");
  PCR_REQUIRE(edge_ratio >= 0.0f && edge_ratio < 1.0f, "rigid_ransac: edge_ratio outside [0, 1)");
  PCR_REQUIRE(refine_iters >= 0, "rigid_ransac: negative refine_iters");
  if (p == 0) return PCR_OK;
  PCR_REQUIRE(xyz1 && xyz2 && idx1 && idx2 && count && transform && inliers && num_inliers &&
                  best_hyp && status,
              "rigid_ransac: null pointer");
  const size_t need = rigid_ws_bytes(p, hyps);
  PCR_REQUIRE(workspace != nullptr && workspace_bytes >= need,
              "rigid_ransac: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const int nb = ceil_div(hyps, kRB);
  const float tau2 = inlier_dist * inlier_dist;
  unsigned long long* wsbest = (unsigned long long*)workspace;
  hipLaunchKernelGGL(rigid_hyp_kernel, dim3(p, nb), dim3(kRB), 0, st, xyz1, xyz2, n1, n2, idx1,
                     idx2, count, hyps, tau2, edge_ratio, seed, scores, wsbest);
  hipLaunchKernelGGL(rigid_refit_kernel, dim3(p), dim3(kRB), 0, st, xyz1, xyz2, n1, n2, idx1, idx2,
                     count, nb, tau2, refine_iters, seed, wsbest, transform, inliers, num_inliers,
                     best_hyp, status);
  return launch_status("rigid_ransac");
}
