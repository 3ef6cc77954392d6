// knn.hip -- the KNN entry points, the brute-force KNN kernels behind the
// spatial search (knn_spatial.hip) and the KNN backward, for gfx950.
//
// Replaces knn/knn.cu:5-98 (KnnKernel / KnnGradKernel) of the reference's
// PVCNN/modules/functional/src.
//
// KNN: the reference keeps each query's top-k in GLOBAL memory and runs an
// O(k) bubble pass per candidate with one workgroup per cloud.  Here each
// thread owns one query and keeps its top-k in registers (a compile-time
// sized, statically indexed sorted array, branch-free insertion), the
// candidate cloud is staged through LDS in coalesced tiles shared by the
// 256 queries of the workgroup, and the grid spans (query blocks x clouds).
// Candidates are scanned in ascending index with a strict `<` test, which is
// exactly the reference's tie rule (lower index first); slots that never fill
// keep (10000, 0) as the reference's ones*10000 / zeros init.
#include "knn_spatial.hpp"

namespace pcr {

constexpr int kKnnThreads = 256;
constexpr int kKnnTile = 1024;
constexpr int kMaxC = 8;

// Sorted ascending; valid region is the LAST k slots, the first KMAX-k slots
// hold -inf and are never displaced.  Insert (d, j) if d < D[KMAX-1].
template <int KMAX>
struct TopK {
  float d[KMAX];
  int j[KMAX];
  __device__ void init(int k) {
#pragma unroll
    for (int q = 0; q < KMAX; q++) {
      d[q] = (q < KMAX - k) ? -__builtin_inff() : PCR_KNN_UNDEF;
      j[q] = 0;
    }
  }
  __device__ float thr() const { return d[KMAX - 1]; }
  // Insertion as a compare-exchange carry chain: the new element passes every
  // slot it is not strictly smaller than (equal distances keep the earlier,
  // lower index first); from its slot on, every element shifts by one
  // (`ins`), so equal displaced elements keep their order.  A non-qualifying
  // x (>= D[KMAX-1], or NaN) falls off the end unchanged.  Lane masks are
  // short-lived (no SGPR pressure, unlike a hoisted compare-all form).
  __device__ void insert(float x, int jx) {
    bool ins = false;
#pragma unroll
    for (int q = 0; q < KMAX; q++) {
      const bool lt = ins || (x < d[q]);
      const float nd = lt ? x : d[q];
      const int nj = lt ? jx : j[q];
      x = lt ? d[q] : x;
      jx = lt ? j[q] : jx;
      d[q] = nd;
      j[q] = nj;
      ins = lt;
    }
  }
};

// Distance with the reference's contraction: d = t0*t0, d = fma(tp, tp, d)
// (knn.cu:20-24 under nvcc --fmad=true).
template <int KMAX, bool PPF, int CC>
__global__ __launch_bounds__(kKnnThreads) void knn_kernel(
    const float* __restrict__ xyz1, const float* __restrict__ xyz2, int c, int n, int m, int k,
    float* __restrict__ dist, int* __restrict__ idx,
    // fused local PPF (self KNN): normals of xyz1 (== xyz2), output [b,4,k,n]
    const float* __restrict__ normals, int relative, float* __restrict__ ppf) {
  __shared__ float tile_s[kMaxC * kKnnTile];
  const int b = blockIdx.y;
  const int i = blockIdx.x * kKnnThreads + threadIdx.x;
  const bool active = i < n;
  const float* x1 = xyz1 + (size_t)b * c * n;
  const float* x2 = xyz2 + (size_t)b * c * m;
  // CC == 3: the xyz specialisation; CC == kMaxC: generic c <= kMaxC
  float q[CC];
#pragma unroll
  for (int p = 0; p < CC; p++) q[p] = (p < c && active) ? x1[i + (size_t)p * n] : 0.0f;
  TopK<KMAX> top;
  top.init(k);
  for (int t0 = 0; t0 < m; t0 += kKnnTile) {
    const int tl = min(kKnnTile, m - t0);
    __syncthreads();
    for (int p = 0; p < c; p++)
      for (int t = threadIdx.x; t < tl; t += kKnnThreads)
        tile_s[p * kKnnTile + t] = x2[(size_t)p * m + t0 + t];
    __syncthreads();
    if (active) {
      if (CC == 3) {
#pragma unroll 1
        for (int t = 0; t < tl; t++) {
          const float a = q[0] - tile_s[t];
          const float bb = q[1] - tile_s[kKnnTile + t];
          const float cc = q[2] - tile_s[2 * kKnnTile + t];
          float d = a * a;
          d = __builtin_fmaf(bb, bb, d);
          d = __builtin_fmaf(cc, cc, d);
          if (__any(d < top.thr())) top.insert(d, t0 + t);  // no-op for d >= thr
        }
      } else {
#pragma unroll 1
        for (int t = 0; t < tl; t++) {
          float d = 0.0f;
#pragma unroll
          for (int p = 0; p < CC; p++) {
            if (p < c) {
              const float a = q[p] - tile_s[p * kKnnTile + t];
              d = (p == 0) ? a * a : __builtin_fmaf(a, a, d);
            }
          }
          if (__any(d < top.thr())) top.insert(d, t0 + t);  // no-op for d >= thr
        }
      }
    }
  }
  if (!active) return;
  const int base = KMAX - k;
#pragma unroll
  for (int s = 0; s < KMAX; s++) {
    if (s >= base) {
      const size_t o = ((size_t)b * k + (s - base)) * n + i;
      if (dist) dist[o] = top.d[s];
      if (idx) idx[o] = top.j[s];
    }
  }
  if (PPF) {
    // neighbour ids re-read from the rows this thread just wrote (idx is
    // required for the fused variant) to keep the slot loop rolled
    const float* nb = normals + (size_t)b * 3 * n;
    const float cnx = nb[i], cny = nb[i + n], cnz = nb[i + 2 * n];
#pragma unroll 1
    for (int slot = 0; slot < k; slot++) {
      const int jn = idx[((size_t)b * k + slot) * n + i];
      float o[4];
      pcr_local_ppf(q[0], q[1], q[2], cnx, cny, cnz, x2[jn], x2[jn + m], x2[jn + 2 * m], nb[jn],
                    nb[jn + n], nb[jn + 2 * n], relative, o);
#pragma unroll
      for (int ch = 0; ch < 4; ch++) ppf[(((size_t)b * 4 + ch) * k + slot) * n + i] = o[ch];
    }
  }
}

// k > 128: the reference algorithm itself (top-k in the output buffers).
__global__ __launch_bounds__(256) void knn_generic_kernel(const float* __restrict__ xyz1,
                                                          const float* __restrict__ xyz2, int c,
                                                          int n, int m, int k,
                                                          float* __restrict__ dist,
                                                          int* __restrict__ idx) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* x1 = xyz1 + (size_t)b * c * n;
  const float* x2 = xyz2 + (size_t)b * c * m;
  float* D = dist + (size_t)b * k * n;
  int* I = idx + (size_t)b * k * n;
  for (int q = 0; q < k; q++) {
    D[i + (size_t)q * n] = PCR_KNN_UNDEF;
    I[i + (size_t)q * n] = 0;
  }
  for (int j = 0; j < m; j++) {
    float d = 0.0f;
    for (int p = 0; p < c; p++) {
      const float a = x1[i + (size_t)p * n] - x2[j + (size_t)p * m];
      d = (p == 0) ? a * a : __builtin_fmaf(a, a, d);
    }
    if (d < D[i + (size_t)(k - 1) * n]) {
      int q = k - 1;
      while (q > 0 && d < D[i + (size_t)(q - 1) * n]) {
        D[i + (size_t)q * n] = D[i + (size_t)(q - 1) * n];
        I[i + (size_t)q * n] = I[i + (size_t)(q - 1) * n];
        q--;
      }
      D[i + (size_t)q * n] = d;
      I[i + (size_t)q * n] = j;
    }
  }
}

// knn.cu:52-78: one direction, atomically accumulated into both grads.
__global__ __launch_bounds__(256) void knn_grad_kernel(const float* __restrict__ x1,
                                                       const float* __restrict__ x2, int c, int n,
                                                       int m, int k, const float* __restrict__ gd,
                                                       const int* __restrict__ id,
                                                       float* __restrict__ g1,
                                                       float* __restrict__ g2) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  x1 += (size_t)b * c * n;
  x2 += (size_t)b * c * m;
  gd += (size_t)b * k * n;
  id += (size_t)b * k * n;
  g1 += (size_t)b * c * n;
  g2 += (size_t)b * c * m;
  for (int q = 0; q < k; q++) {
    const float g = gd[i + (size_t)q * n] * 2.0f;
    if (g >= 20000.0f) continue;
    const int j = id[i + (size_t)q * n];
    if (j < 0 || j >= m) continue;
    for (int p = 0; p < c; p++) {
      const float t = g * (x1[i + (size_t)p * n] - x2[j + (size_t)p * m]);
      atomicAdd(g1 + i + (size_t)p * n, t);
      atomicAdd(g2 + j + (size_t)p * m, -t);
    }
  }
}

// KNN backward without atomics (contract knn.cu:52-78, both launches of
// knn.cu:88-98): every output element is a gather of its own terms in a
// fixed order, so the gradient is bit-repeatable.  Point i of cloud A gets
//   sum_q  g(q,i) (xA[i] - xB[idxA(q,i)])                    own slots
//   - sum over the pairs (q, i') of cloud B's direction with idxB(q,i') = i
//         of g(q,i') (xB[i'] - xA[i])                         as a neighbour
// with g = 2 graddist skipped at >= 20000, every term the reference's own
// product.  The second sum needs, per target point, the list of pairs that
// name it: knn_bwd_sort_kernel counts each direction's pairs per target (one
// workgroup per (cloud, direction), LDS counters: the segment starts) and
// orders them by target, ascending pair id within a target, with a stable
// workgroup radix sort (O(P) per pass), and knn_bwd_gather_kernel sums, one
// thread per point.
constexpr int kKnnBwdThreads = 1024;
constexpr int kKnnBwdMaxT = 16384;  // targets per cloud the LDS counters hold

struct KnnBwdWs {
  int* start[2];  // [b][T_d + 1] segment starts of direction d (by target)
  int* list[2];   // [b][k N_d] pair ids (q N_d + i) by target, ascending within a target
  int* tmp[2];    // [b][k N_d] the radix sort's second buffer
};

static size_t knn_bwd_ws_layout(int b, int n, int m, int k, KnnBwdWs* w, char* base) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* q = base ? base + off : nullptr;
    off = (off + bytes + 255) / 256 * 256;
    return (int*)q;
  };
  const int N[2] = {n, m}, T[2] = {m, n};
  for (int d = 0; d < 2; d++) {
    int* s = take((size_t)b * (T[d] + 1) * 4);
    int* l = take((size_t)b * k * N[d] * 4);
    int* t = take((size_t)b * k * N[d] * 4);
    if (w) {
      w->start[d] = s;
      w->list[d] = l;
      w->tmp[d] = t;
    }
  }
  return off;
}

__global__ __launch_bounds__(kKnnBwdThreads) void knn_bwd_sort_kernel(
    const float* __restrict__ gd0, const int* __restrict__ idx0, const float* __restrict__ gd1,
    const int* __restrict__ idx1, int n, int m, int k, KnnBwdWs ws) {
  extern __shared__ int cnt_s[];  // [T]
  __shared__ int scan_s[kKnnBwdThreads / kWave + 1];
  __shared__ int rs_lds[(2 + kKnnBwdThreads / kWave) * 256];  // wg_radix_sort
  const int b = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
  const int N = d ? m : n, T = d ? n : m;
  const size_t P = (size_t)k * N;
  const float* gd = (d ? gd1 : gd0) + (size_t)b * P;
  const int* idx = (d ? idx1 : idx0) + (size_t)b * P;
  int* start = ws.start[d] + (size_t)b * (T + 1);
  int* list = ws.list[d] + (size_t)b * P;
  int* tmp = ws.tmp[d] + (size_t)b * P;
  auto target = [&](size_t p) {
    const float g = gd[p] * 2.0f;
    const int j = idx[p];
    return (!(g >= 20000.0f) && j >= 0 && j < T) ? j : -1;  // knn.cu:68: NaN is not skipped
  };
  for (int t = tid; t < T; t += kKnnBwdThreads) cnt_s[t] = 0;
  __syncthreads();
  for (size_t p = tid; p < P; p += kKnnBwdThreads) {
    const int j = target(p);
    if (j >= 0) atomicAdd(&cnt_s[j], 1);
  }
  __syncthreads();
  {
    const int chunk = (T + kKnnBwdThreads - 1) / kKnnBwdThreads;
    const int t0 = min(T, tid * chunk), t1 = min(T, t0 + chunk);
    int sum = 0;
    for (int t = t0; t < t1; t++) sum += cnt_s[t];
    const int incl = block_inclusive_scan(sum, scan_s);
    int run = incl - sum;
    for (int t = t0; t < t1; t++) {
      const int c = cnt_s[t];
      start[t] = run;
      run += c;
    }
    if (tid == kKnnBwdThreads - 1) start[T] = incl;
  }
  __syncthreads();
  // the pairs by target, ascending pair id within a target: a stable LSD
  // radix sort of the pair ids keyed by target (invalid pairs key T: last).
  // O(P) per pass, whatever the targets' multiplicities (a hub neighbour
  // named by thousands of pairs costs no more than any other target)
  for (size_t p = tid; p < P; p += kKnnBwdThreads) list[p] = (int)p;
  __threadfence_block();
  __syncthreads();
  const int kbits = 32 - __clz(T);  // keys 0 .. T
  int* res = wg_radix_sort<kKnnBwdThreads>(
      list, tmp, (int)P, kbits,
      [&](int p) {
        const int j = target((size_t)p);
        return j >= 0 ? j : T;
      },
      rs_lds);
  if (res != list) {
    const int total = start[T];
    for (int e = tid; e < total; e += kKnnBwdThreads) list[e] = res[e];
  }
}

template <int CG>
__global__ __launch_bounds__(256) void knn_bwd_gather_kernel(
    const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ gd0,
    const int* __restrict__ idx0, const float* __restrict__ gd1, const int* __restrict__ idx1,
    int c, int n, int m, int k, KnnBwdWs ws, float* __restrict__ g1, float* __restrict__ g2) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n + m) return;
  const int side = t < n ? 0 : 1;  // cloud A of this point: 0 = xyz1, 1 = xyz2
  const int i = side ? t - n : t;
  const int Na = side ? m : n, Nb = side ? n : m;
  const float* xa = (side ? x2 : x1) + (size_t)b * c * Na;
  const float* xb = (side ? x1 : x2) + (size_t)b * c * Nb;
  const float* gdo = (side ? gd1 : gd0) + (size_t)b * k * Na;  // own direction
  const int* ido = (side ? idx1 : idx0) + (size_t)b * k * Na;
  const float* gdt = (side ? gd0 : gd1) + (size_t)b * k * Nb;  // cloud B's direction
  const int* lst = ws.list[1 - side] + (size_t)b * k * Nb;
  const int* st = ws.start[1 - side] + (size_t)b * (Na + 1);
  float* out = (side ? g2 : g1) + (size_t)b * c * Na;
  const int s0 = st[i], s1 = st[i + 1];
  for (int c0 = 0; c0 < c; c0 += CG) {
    float acc[CG], xi[CG];
#pragma unroll
    for (int p = 0; p < CG; p++) {
      acc[p] = 0.0f;
      xi[p] = c0 + p < c ? xa[(size_t)(c0 + p) * Na + i] : 0.0f;
    }
    for (int q = 0; q < k; q++) {
      const float g = gdo[(size_t)q * Na + i] * 2.0f;
      const int j = ido[(size_t)q * Na + i];
      if (g >= 20000.0f || j < 0 || j >= Nb) continue;
#pragma unroll
      for (int p = 0; p < CG; p++)
        if (c0 + p < c) acc[p] += g * (xi[p] - xb[(size_t)(c0 + p) * Nb + j]);
    }
    // the pairs naming this point, ascending: four at a time with their
    // loads issued ahead of the in-order sums (a hub point named by
    // thousands of pairs waits a quarter of the load round trips)
    int e = s0;
    for (; e + 4 <= s1; e += 4) {
      int pp[4];
      float g[4], xv[4][CG];
#pragma unroll
      for (int u = 0; u < 4; u++) pp[u] = lst[e + u];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i2 = pp[u] % Nb;
        g[u] = gdt[pp[u]] * 2.0f;
#pragma unroll
        for (int p = 0; p < CG; p++) xv[u][p] = c0 + p < c ? xb[(size_t)(c0 + p) * Nb + i2] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int p = 0; p < CG; p++)
          if (c0 + p < c) acc[p] += -(g[u] * (xv[u][p] - xi[p]));
    }
    for (; e < s1; e++) {
      const int pp = lst[e];
      const int i2 = pp % Nb;
      const float g = gdt[pp] * 2.0f;
#pragma unroll
      for (int p = 0; p < CG; p++)
        if (c0 + p < c) acc[p] += -(g * (xb[(size_t)(c0 + p) * Nb + i2] - xi[p]));
    }
#pragma unroll
    for (int p = 0; p < CG; p++)
      if (c0 + p < c) out[(size_t)(c0 + p) * Na + i] = acc[p];
  }
}

template <bool PPF, int CC>
static pcr_status launch_knn_c(const float* xyz1, const float* xyz2, int b, int c, int n, int m,
                               int k, float* dist, int* idx, const float* normals, int relative,
                               float* ppf, hipStream_t st) {
  const dim3 grid(ceil_div(n, kKnnThreads), b);
  const bool ok = with_kmax(k, [&](auto km) {
    hipLaunchKernelGGL((knn_kernel<decltype(km)::value, PPF, CC>), grid, dim3(kKnnThreads), 0, st,
                       xyz1, xyz2, c, n, m, k, dist, idx, normals, relative, ppf);
  });
  return ok ? PCR_OK : PCR_ERR_UNSUPPORTED;
}

template <bool PPF>
static pcr_status launch_knn(const float* xyz1, const float* xyz2, int b, int c, int n, int m,
                             int k, float* dist, int* idx, const float* normals, int relative,
                             float* ppf, hipStream_t st) {
  if (c == 3)
    return launch_knn_c<PPF, 3>(xyz1, xyz2, b, c, n, m, k, dist, idx, normals, relative, ppf, st);
  if (PPF) return PCR_ERR_UNSUPPORTED;
  return launch_knn_c<false, kMaxC>(xyz1, xyz2, b, c, n, m, k, dist, idx, normals, relative, ppf,
                                    st);
}

}  // namespace pcr

using namespace pcr;

extern "C" pcr_status pcr_knn_forward(const float* xyz1, const float* xyz2, int b, int c, int n,
                                      int m, int k, float* dist1, float* dist2, int* idx1,
                                      int* idx2, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  PCR_REQUIRE(b >= 0 && c >= 1 && n >= 0 && m >= 0 && k >= 1, "knn_forward: invalid sizes");
  PCR_REQUIRE(dist1 && dist2 && idx1 && idx2, "knn_forward: all four outputs required");
  if (b == 0) return PCR_OK;
  hipStream_t st = as_stream(stream);
  KnnIO io;
  io.dist1 = dist1, io.idx1 = idx1, io.dist2 = dist2, io.idx2 = idx2;
  if (c == 3 && n > 0 && m > 0 &&
      knn_spatial(xyz1, xyz2, b, n, m, k, io, workspace, workspace_bytes, xyz1 == xyz2 && n == m,
                  st) == PCR_OK)
    return launch_status("knn_forward");
  if (c <= kMaxC && k <= 128) {
    if (n > 0) launch_knn<false>(xyz1, xyz2, b, c, n, m, k, dist1, idx1, nullptr, 0, nullptr, st);
    if (m > 0) launch_knn<false>(xyz2, xyz1, b, c, m, n, k, dist2, idx2, nullptr, 0, nullptr, st);
  } else {
    if (n > 0)
      hipLaunchKernelGGL(knn_generic_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, xyz1,
                         xyz2, c, n, m, k, dist1, idx1);
    if (m > 0)
      hipLaunchKernelGGL(knn_generic_kernel, dim3(ceil_div(m, 256), b), dim3(256), 0, st, xyz2,
                         xyz1, c, m, n, k, dist2, idx2);
  }
  return launch_status("knn_forward");
}

extern "C" pcr_status pcr_knn_backward(const float* xyz1, const float* xyz2,
                                       const float* graddist1, const float* graddist2,
                                       const int* idx1, const int* idx2, int b, int c, int n,
                                       int m, int k, float* gradxyz1, float* gradxyz2,
                                       void* stream) {
  PCR_REQUIRE(b >= 0 && c >= 1 && n >= 0 && m >= 0 && k >= 1, "knn_backward: invalid sizes");
  if (b == 0) return PCR_OK;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(gradxyz1, 0, sizeof(float) * (size_t)b * c * n, st) != hipSuccess ||
      hipMemsetAsync(gradxyz2, 0, sizeof(float) * (size_t)b * c * m, st) != hipSuccess)
    return launch_status("knn_backward memset");
  if (n > 0)
    hipLaunchKernelGGL(knn_grad_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, xyz1, xyz2,
                       c, n, m, k, graddist1, idx1, gradxyz1, gradxyz2);
  if (m > 0)
    hipLaunchKernelGGL(knn_grad_kernel, dim3(ceil_div(m, 256), b), dim3(256), 0, st, xyz2, xyz1,
                       c, m, n, k, graddist2, idx2, gradxyz2, gradxyz1);
  return launch_status("knn_backward");
}

// clouds past the LDS counters (or empty ones) take the atomic kernel, which
// needs no workspace
static bool knn_bwd_sorted_applies(int n, int m, int k) {
  return !(n > kKnnBwdMaxT || m > kKnnBwdMaxT || n == 0 || m == 0 ||
           (size_t)k * (n > m ? n : m) >= (1u << 31));
}

extern "C" size_t pcr_knn_backward_workspace_size(int b, int n, int m, int k) {
  if (b <= 0 || n < 0 || m < 0 || k <= 0 || !knn_bwd_sorted_applies(n, m, k)) return 256;
  return knn_bwd_ws_layout(b, n, m, k, nullptr, nullptr);
}

extern "C" pcr_status pcr_knn_backward_ws(const float* xyz1, const float* xyz2,
                                          const float* graddist1, const float* graddist2,
                                          const int* idx1, const int* idx2, int b, int c, int n,
                                          int m, int k, float* gradxyz1, float* gradxyz2,
                                          void* workspace, size_t workspace_bytes,
                                          void* stream) {
  PCR_REQUIRE(b >= 0 && c >= 1 && n >= 0 && m >= 0 && k >= 1,
              "knn_backward_ws: invalid sizes");
  if (b == 0) return PCR_OK;
  // clouds past the LDS counters: the atomic kernel (same contract)
  if (!knn_bwd_sorted_applies(n, m, k))
    return pcr_knn_backward(xyz1, xyz2, graddist1, graddist2, idx1, idx2, b, c, n, m, k,
                            gradxyz1, gradxyz2, stream);
  KnnBwdWs ws;
  const size_t need = knn_bwd_ws_layout(b, n, m, k, &ws, (char*)workspace);
  PCR_REQUIRE(workspace != nullptr && workspace_bytes >= need,
              "knn_backward_ws: workspace too small (%zu < %zu)", workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  const size_t lds = (size_t)(n > m ? n : m) * 4;
  allow_big_lds(knn_bwd_sort_kernel, lds);
  hipLaunchKernelGGL(knn_bwd_sort_kernel, dim3(b, 2), dim3(kKnnBwdThreads), lds, st, graddist1,
                     idx1, graddist2, idx2, n, m, k, ws);
  const dim3 grid(ceil_div(n + m, 256), b);
  if (c <= 3)
    hipLaunchKernelGGL((knn_bwd_gather_kernel<3>), grid, dim3(256), 0, st, xyz1, xyz2, graddist1,
                       idx1, graddist2, idx2, c, n, m, k, ws, gradxyz1, gradxyz2);
  else
    hipLaunchKernelGGL((knn_bwd_gather_kernel<4>), grid, dim3(256), 0, st, xyz1, xyz2, graddist1,
                       idx1, graddist2, idx2, c, n, m, k, ws, gradxyz1, gradxyz2);
  return launch_status("knn_backward_ws");
}

extern "C" pcr_status pcr_knn_local_ppf(const float* xyz, const float* normals, int b, int n,
                                        int k, int relative, int* idx, float* dist, float* ppf,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 1 && k >= 1 && k <= 128, "knn_local_ppf: invalid sizes (k<=128)");
  PCR_REQUIRE(ppf != nullptr && idx != nullptr, "knn_local_ppf: idx and ppf outputs required");
  if (b == 0) return PCR_OK;
  KnnIO io;
  io.dist1 = dist, io.idx1 = idx, io.ppf1 = ppf;
  io.nrm1 = io.nrm2 = normals, io.relative = relative;
  if (knn_spatial(xyz, xyz, b, n, n, k, io, workspace, workspace_bytes, true,
                  as_stream(stream)) == PCR_OK)
    return launch_status("knn_local_ppf");
  launch_knn<true>(xyz, xyz, b, 3, n, n, k, dist, idx, normals, relative, ppf, as_stream(stream));
  return launch_status("knn_local_ppf");
}

extern "C" pcr_status pcr_knn_prepare(const float* xyz, int b, int n, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 1, "knn_prepare: invalid sizes");
  if (b == 0) return PCR_OK;
  const pcr_status rc = knn_spatial(xyz, xyz, b, n, n, 1, KnnIO{}, workspace, workspace_bytes,
                                    true, as_stream(stream), kKnnSort);
  if (rc == PCR_ERR_UNSUPPORTED) {
    set_error("knn_prepare: no sorted path for n=%d (use pcr_knn_local_ppf)", n);
    return rc;
  }
  return launch_status("knn_prepare");
}

extern "C" pcr_status pcr_knn_local_ppf_prepared(const float* xyz, const float* normals, int b,
                                                 int n, int k, int relative, int* idx, float* dist,
                                                 float* ppf, const void* workspace,
                                                 size_t workspace_bytes, void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 1 && k >= 1 && k <= 128,
              "knn_local_ppf_prepared: invalid sizes (k<=128)");
  PCR_REQUIRE(idx != nullptr, "knn_local_ppf_prepared: idx required");
  if (b == 0) return PCR_OK;
  KnnIO io;
  io.dist1 = dist, io.idx1 = idx, io.ppf1 = ppf;
  io.nrm1 = io.nrm2 = normals, io.relative = relative;
  const pcr_status rc = knn_spatial(xyz, xyz, b, n, n, k, io, const_cast<void*>(workspace),
                                    workspace_bytes, true, as_stream(stream), kKnnSelect);
  if (rc == PCR_ERR_UNSUPPORTED) {
    set_error("knn_local_ppf_prepared: no sorted path for n=%d, k=%d", n, k);
    return rc;
  }
  return launch_status("knn_local_ppf_prepared");
}

// The two launches of pcr_knn_select_ppf as entry points of their own (the
// c3 bench times the selection in step between them).  select_sorted returns
// PCR_ERR_UNSUPPORTED, launching nothing, when the sorted-rows path does not
// apply (k > 32, clouds of more than 2048 points, no sorted views).
extern "C" pcr_status pcr_knn_select_sorted(const float* xyz, int b, int n, int k,
                                            const void* workspace, size_t workspace_bytes,
                                            void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 1 && k >= 1 && k <= 128, "knn_select_sorted: invalid sizes");
  if (b == 0) return PCR_OK;
  const int* sidx = nullptr;
  const int* inv = nullptr;
  int npad = 0;
  if (workspace == nullptr || n > kPpfSelfMaxN ||
      !knn_sorted_views(const_cast<void*>(workspace), b, n, &sidx, &inv, &npad))
    return PCR_ERR_UNSUPPORTED;
  return knn_spatial(xyz, xyz, b, n, n, k, KnnIO{}, const_cast<void*>(workspace), workspace_bytes,
                     true, as_stream(stream), kKnnSelect | kKnnSortedRows);
}

// The one ladder of selection + local PPF from a prepared workspace
// (knn_spatial.hpp): the sorted-rows pair when distances are not wanted and it
// applies, else prepared selection + the PPF launch.
pcr_status pcr::knn_select_ppf_prepared(const float* xyz, const float* normals, int b, int n, int k,
                                        int relative, int* idx, float* dist, float* ppf,
                                        const void* workspace, size_t workspace_bytes,
                                        void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 1 && k >= 1 && k <= 128, "knn_select_ppf: invalid sizes (k<=128)");
  PCR_REQUIRE(idx != nullptr && ppf != nullptr, "knn_select_ppf: idx and ppf required");
  if (b == 0) return PCR_OK;
  if (dist == nullptr &&
      pcr_knn_select_sorted(xyz, b, n, k, workspace, workspace_bytes, stream) == PCR_OK)
    return pcr_knn_ppf_sorted(xyz, normals, b, n, k, relative, idx, ppf, workspace,
                              workspace_bytes, stream);
  const pcr_status rc = pcr_knn_local_ppf_prepared(xyz, normals, b, n, k, relative, idx, dist,
                                                   nullptr, workspace, workspace_bytes, stream);
  if (rc != PCR_OK) return rc;
  return pcr_local_ppf_forward(xyz, normals, xyz, normals, idx, b, n, n, k, 1, relative, ppf,
                               stream);
}

extern "C" pcr_status pcr_knn_select_ppf(const float* xyz, const float* normals, int b, int n,
                                         int k, int relative, int* idx, float* ppf,
                                         const void* workspace, size_t workspace_bytes,
                                         void* stream) {
  return knn_select_ppf_prepared(xyz, normals, b, n, k, relative, idx, nullptr, ppf, workspace,
                                 workspace_bytes, stream);
}
