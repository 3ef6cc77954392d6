// neighbors.hip -- ball query, grouping and the math self-test hooks, for
// gfx950.
//
// Replaces (relative to the reference's PVCNN/modules/functional/src):
//   ball_query/ball_query.cu:19-59
//   grouping/grouping.cu:18-85
#include "common.hpp"

namespace pcr {

// ball_query.cu:30-49: points staged through LDS tiles; per-centre early exit
constexpr int kBqTile = 1024;
__global__ __launch_bounds__(256) void ball_query_kernel(const float* __restrict__ centers,
                                                         const float* __restrict__ points, int m,
                                                         int n, float r2, int u,
                                                         int* __restrict__ idx) {
  __shared__ float tile_s[3 * kBqTile];
  const int b = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = j < m;
  const float* C = centers + (size_t)b * 3 * m;
  const float* P = points + (size_t)b * 3 * n;
  int* I = idx + (size_t)b * m * u + (size_t)j * u;
  float cx = 0.f, cy = 0.f, cz = 0.f;
  if (active) {
    cx = C[j];
    cy = C[j + m];
    cz = C[j + 2 * m];
  }
  int cnt = 0, first = 0;
  bool done = !active;
  for (int t0 = 0; t0 < n; t0 += kBqTile) {
    if (!__syncthreads_or(!done)) break;
    const int tl = min(kBqTile, n - t0);
    for (int t = threadIdx.x; t < tl; t += blockDim.x) {
      tile_s[t] = P[t0 + t];
      tile_s[kBqTile + t] = P[n + t0 + t];
      tile_s[2 * kBqTile + t] = P[2 * n + t0 + t];
    }
    __syncthreads();
    if (!done) {
      for (int t = 0; t < tl && cnt < u; t++) {
        const float dx = cx - tile_s[t], dy = cy - tile_s[kBqTile + t],
                    dz = cz - tile_s[2 * kBqTile + t];
        const float d2 = pcr_sumsq3f(dx, dy, dz);
        if (d2 < r2 && (double)d2 > 1e-5) {
          if (cnt == 0) first = t0 + t;
          I[cnt] = t0 + t;
          ++cnt;
        }
      }
      if (cnt >= u) done = true;
    }
    __syncthreads();
  }
  if (active)
    for (int v = cnt; v < u; v++) I[v] = first;
}

// The same query, one wave per 64 centres (lane = centre) and NW waves per
// workgroup.  The cloud is staged in LDS once per workgroup and read as
// broadcast float4s (four candidates per read); the squared distances run
// two candidates per packed instruction in the reference's contraction order
// (pcr_sumsq3f: y*y, then +x*x, then +z*z).  Each wave scans a contiguous
// range of 32-point words and keeps, per centre, one hit bit per point: a
// register word stored once per 32 candidates, no per-hit work.  The output
// pass then turns every centre's bit row into its first u hit indices in
// index order (a popcount prefix over the words, one wave per centre row),
// padded with the first hit (0 if none): the reference's slots, whatever the
// count of hits.  (double)d2 > 1e-5 is evaluated as d2 > 1e-5f: float(1e-5)
// lies below 1e-5, so for every float d2 the two agree.
constexpr int kBqWaves = 4;
template <int NW>
__global__ __launch_bounds__(NW * 64) void ball_query_mask_kernel(
    const float* __restrict__ centers, const float* __restrict__ points, int m, int n, int nwords,
    float r2, int u, int* __restrict__ idx) {
  extern __shared__ __align__(16) unsigned char bq_s[];
  const int npad = nwords * 32;
  float* px = (float*)bq_s;
  float* py = px + npad;
  float* pz = py + npad;
  unsigned* msk = (unsigned*)(pz + npad);  // [nwords][64]: bit i of word w = point 32 w + i
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * kWave;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* P = points + (size_t)b * 3 * n;
  for (int i = tid; i < npad; i += NW * kWave) {
    const bool ok = i < n;
    px[i] = ok ? P[i] : __builtin_nanf("");
    py[i] = ok ? P[n + i] : __builtin_nanf("");
    pz[i] = ok ? P[2 * n + i] : __builtin_nanf("");
  }
  const int j = c0 + lane;
  const bool live = j < m;
  const float* C = centers + (size_t)b * 3 * m;
  const float cx = live ? C[j] : 0.0f, cy = live ? C[m + j] : 0.0f, cz = live ? C[2 * m + j] : 0.0f;
  __syncthreads();
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 cx2 = {cx, cx}, cy2 = {cy, cy}, cz2 = {cz, cz};
  const int wpw = (nwords + NW - 1) / NW;
  const int w0 = min(nwords, wv * wpw), w1 = min(nwords, w0 + wpw);
  for (int w = w0; w < w1; w++) {
    unsigned bits = 0u;
#pragma unroll
    for (int t4 = 0; t4 < 32; t4 += 4) {
      const int t = w * 32 + t4;
      const float4 X = *(const float4*)(px + t);
      const float4 Y = *(const float4*)(py + t);
      const float4 Z = *(const float4*)(pz + t);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const f2 dx = cx2 - (h ? f2{X.z, X.w} : f2{X.x, X.y});
        const f2 dy = cy2 - (h ? f2{Y.z, Y.w} : f2{Y.x, Y.y});
        const f2 dz = cz2 - (h ? f2{Z.z, Z.w} : f2{Z.x, Z.y});
        f2 a = dy * dy;
        a = __builtin_elementwise_fma(dx, dx, a);
        const f2 d = __builtin_elementwise_fma(dz, dz, a);
        bits |= (d[0] < r2 && d[0] > 1e-5f ? 1u : 0u) << (t4 + 2 * h);
        bits |= (d[1] < r2 && d[1] > 1e-5f ? 1u : 0u) << (t4 + 2 * h + 1);
      }
    }
    msk[w * kWave + lane] = bits;
  }
  __syncthreads();
  // output: one wave per centre row; lane l takes word 64 q + l of chunk q
  for (int row = wv; row < kWave; row += NW) {
    const int jj = c0 + row;
    if (jj >= m) break;
    int* I = idx + ((size_t)b * m + jj) * u;
    int base = 0, first = -1;
    for (int q0 = 0; q0 < nwords && base < u; q0 += kWave) {
      const int w = q0 + lane;
      unsigned bits = w < nwords ? msk[w * kWave + row] : 0u;
      const int pc = __popc(bits);
      int incl = pc;
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const int o = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += o;
      }
      if (first < 0) {
        const unsigned long long any = __ballot(bits != 0u);
        if (any) {
          const int l0 = __builtin_ctzll(any);
          const unsigned b0 = __shfl(bits, l0, kWave);
          first = (q0 + l0) * 32 + __builtin_ctz(b0);
        }
      }
      int s = base + incl - pc;
      while (bits && s < u) {
        I[s++] = w * 32 + __builtin_ctz(bits);
        bits &= bits - 1u;
      }
      base += __shfl(incl, kWave - 1, kWave);
    }
    const int fill = first < 0 ? 0 : first;
    for (int s = min(base, u) + lane; s < u; s += kWave) I[s] = fill;
  }
}

// grouping.cu:29-35: one thread per output element, coalesced stores
__global__ __launch_bounds__(256) void grouping_kernel(const float* __restrict__ feat,
                                                       const int* __restrict__ idx, int c, int n,
                                                       int m, int u, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over m*u
  const int l = blockIdx.y;
  const int b = blockIdx.z;
  const int64_t mu = (int64_t)m * u;
  if (e >= mu) return;
  const int s = idx[(size_t)b * mu + e];
  const float v = (s >= 0 && s < n) ? feat[((size_t)b * c + l) * n + s] : 0.0f;
  out[((size_t)b * c + l) * mu + e] = v;
}

// grouping.cu:69-76
__global__ __launch_bounds__(256) void grouping_grad_kernel(const float* __restrict__ grad_y,
                                                            const int* __restrict__ idx, int c,
                                                            int n, int m, int u,
                                                            float* __restrict__ grad_x) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int l = blockIdx.y;
  const int b = blockIdx.z;
  const int64_t mu = (int64_t)m * u;
  if (e >= mu) return;
  const int s = idx[(size_t)b * mu + e];
  if (s < 0 || s >= n) return;
  atomicAdd(grad_x + ((size_t)b * c + l) * n + s, grad_y[((size_t)b * c + l) * mu + e]);
}

// ---------------------------------------------------------- self tests
__global__ void selftest_f_kernel(int op, const float* x, const float* y, int n, int aux,
                                  float* of, int* oi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  switch (op) {
    case 0: of[i] = pcr_acosf(x[i]); break;
    case 1: of[i] = pcr_atanf(x[i]); break;
    case 2: of[i] = __builtin_sqrtf(x[i]); break;
    case 3: of[i] = x[i] / y[i]; break;
    case 4: oi[i] = pcr_sph_index(x[i], x[i + n], x[i + 2 * n], aux); break;
    default: break;
  }
}
__global__ void selftest_d_kernel(int op, const double* x, const double* y, int n, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  switch (op) {
    case 0: o[i] = pcr_acos_d(x[i]); break;
    case 1: o[i] = pcr_atan_d(x[i]); break;
    case 2: o[i] = __builtin_sqrt(x[i]); break;
    case 3: o[i] = x[i] / y[i]; break;
    case 4: o[i] = __builtin_fma(x[i], y[i], x[i]); break;
    default: break;
  }
}

}  // namespace pcr

using namespace pcr;

extern "C" pcr_status pcr_ball_query(const float* centers, const float* points, int b, int m,
                                     int n, float radius, int u, int* idx, void* stream) {
  PCR_REQUIRE(b >= 0 && m >= 0 && n >= 0 && u >= 1, "ball_query: invalid sizes");
  if (b == 0 || m == 0) return PCR_OK;
  const float r2 = radius * radius;  // ball_query.cpp:24 (float * float)
  const int nwords = (n + 31) / 32;
  // staged cloud (12 B per point) + hit bits (64 centres x 1 bit per point)
  const size_t smem = (size_t)nwords * 32 * 12 + (size_t)nwords * kWave * 4;
  if (n >= 1 && smem <= 96 * 1024) {
    allow_big_lds(ball_query_mask_kernel<kBqWaves>, smem);
    hipLaunchKernelGGL(ball_query_mask_kernel<kBqWaves>, dim3(ceil_div(m, kWave), b),
                       dim3(kBqWaves * kWave), smem, as_stream(stream), centers, points, m, n,
                       nwords, r2, u, idx);
  } else {
    hipLaunchKernelGGL(ball_query_kernel, dim3(ceil_div(m, 256), b), dim3(256), 0,
                       as_stream(stream), centers, points, m, n, r2, u, idx);
  }
  return launch_status("ball_query");
}

extern "C" pcr_status pcr_grouping_forward(const float* features, const int* indices, int b, int c,
                                           int n, int m, int u, float* out, void* stream) {
  PCR_REQUIRE(b >= 0 && c >= 0 && n >= 0 && m >= 0 && u >= 0, "grouping_forward: invalid sizes");
  PCR_REQUIRE(c <= 65535, "grouping_forward: c too large");
  const int64_t mu = (int64_t)m * u;
  if (b == 0 || c == 0 || mu == 0) return PCR_OK;
  hipLaunchKernelGGL(grouping_kernel, dim3((unsigned)ceil_div64(mu, 256), c, b), dim3(256), 0,
                     as_stream(stream), features, indices, c, n, m, u, out);
  return launch_status("grouping_forward");
}

extern "C" pcr_status pcr_grouping_backward(const float* grad_y, const int* indices, int b, int c,
                                            int n, int m, int u, float* grad_x, void* stream) {
  PCR_REQUIRE(b >= 0 && c >= 0 && n >= 0 && m >= 0 && u >= 0, "grouping_backward: invalid sizes");
  PCR_REQUIRE(c <= 65535, "grouping_backward: c too large");
  if (b == 0 || c == 0) return PCR_OK;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(grad_x, 0, sizeof(float) * (size_t)b * c * n, st) != hipSuccess)
    return launch_status("grouping_backward memset");
  const int64_t mu = (int64_t)m * u;
  if (mu == 0) return PCR_OK;
  hipLaunchKernelGGL(grouping_grad_kernel, dim3((unsigned)ceil_div64(mu, 256), c, b), dim3(256),
                     0, st, grad_y, indices, c, n, m, u, grad_x);
  return launch_status("grouping_backward");
}

extern "C" pcr_status pcr_selftest_math(int op, const float* x, const float* y, int n, int aux,
                                        float* out_f, int* out_i, void* stream) {
  PCR_REQUIRE(n >= 0 && op >= 0 && op <= 4, "selftest_math: invalid args");
  if (n == 0) return PCR_OK;
  hipLaunchKernelGGL(selftest_f_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, as_stream(stream),
                     op, x, y, n, aux, out_f, out_i);
  return launch_status("selftest_math");
}

extern "C" pcr_status pcr_selftest_math_d(int op, const double* x, const double* y, int n,
                                          double* out, void* stream) {
  PCR_REQUIRE(n >= 0 && op >= 0 && op <= 4, "selftest_math_d: invalid args");
  if (n == 0) return PCR_OK;
  hipLaunchKernelGGL(selftest_d_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, as_stream(stream),
                     op, x, y, n, out);
  return launch_status("selftest_math_d");
}
