// local_ppf.hip -- point-pair features, global and local, for gfx950.
//
// Replaces spherical_ppf/ppf.cu:19-99 (spherical_ppf_kernel) of the
// reference's PVCNN/modules/functional/src and the PyTorch local-PPF block
// of PVCNN/models/pvcnn_classify.py:252-269.
#include "knn_spatial.hpp"

namespace pcr {

// ppf.cu:28-90
__global__ __launch_bounds__(256) void global_ppf_kernel(const float* __restrict__ coords,
                                                         const float* __restrict__ center,
                                                         const float* __restrict__ normals,
                                                         const float* __restrict__ cnormals, int n,
                                                         float* __restrict__ feat) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t o3 = (size_t)b * 3 * n, o4 = (size_t)b * 4 * n;
  float out[4];
  pcr_global_ppf(coords[o3 + i], coords[o3 + i + n], coords[o3 + i + 2 * n], center[o3 + i],
                 center[o3 + i + n], center[o3 + i + 2 * n], normals[o3 + i],
                 normals[o3 + i + n], normals[o3 + i + 2 * n], cnormals[o3 + i],
                 cnormals[o3 + i + n], cnormals[o3 + i + 2 * n], out);
#pragma unroll
  for (int ch = 0; ch < 4; ch++) feat[o4 + i + (size_t)ch * n] = out[ch];
}

// pvcnn_classify.py:258-269 with explicit neighbour indices; out [b,4,u,m]
// buffer resource over [p, p + bytes): raw buffer loads / stores take a
// 32-bit byte offset (no 64-bit address arithmetic per access)
__device__ inline __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes,
                                           0x00020000);
}
__device__ inline float bld(__amdgpu_buffer_rsrc_t r, unsigned i) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)(i * 4u), 0, 0));
}

__global__ __launch_bounds__(256) void local_ppf_kernel(
    const float* __restrict__ pts, const float* __restrict__ nrm, const float* __restrict__ ctr,
    const float* __restrict__ cnrm, const int* __restrict__ idx, int n, int m, int u, int kmajor,
    int relative, float* __restrict__ out) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned q = blockIdx.y;
  const unsigned b = blockIdx.z;
  if (j >= (unsigned)m) return;
  const unsigned un = (unsigned)n, um = (unsigned)m, uu = (unsigned)u;
  const auto P = buf_rsrc(pts + (size_t)b * 3 * un, 12u * un);
  const auto Nn = buf_rsrc(nrm + (size_t)b * 3 * un, 12u * un);
  const auto C = buf_rsrc(ctr + (size_t)b * 3 * um, 12u * um);
  const auto Cn = buf_rsrc(cnrm + (size_t)b * 3 * um, 12u * um);
  const int* I = idx + (size_t)b * um * uu;
  const int si = kmajor ? I[q * um + j] : I[j * uu + q];
  const unsigned s = (si < 0 || si >= n) ? 0u : (unsigned)si;
  float o[4];
  pcr_local_ppf(bld(C, j), bld(C, j + um), bld(C, j + 2 * um), bld(Cn, j), bld(Cn, j + um),
                bld(Cn, j + 2 * um), bld(P, s), bld(P, s + un), bld(P, s + 2 * un), bld(Nn, s),
                bld(Nn, s + un), bld(Nn, s + 2 * un), relative, o);
  float* O = out + (size_t)b * 4 * uu * um;
#pragma unroll
  for (unsigned ch = 0; ch < 4; ch++) O[(ch * uu + q) * um + j] = o[ch];
}

// The same local PPF when the centres are the points themselves and the
// indices are k-major [B, k, N] (the extractor's self-KNN neighbours): one
// workgroup per (cloud, 256 points, SL slots).  The cloud's coordinates and
// normals are staged in LDS in the same round trip as the workgroup's index
// rows, so every neighbour gather is an LDS read: no dependent global loads,
// which under the grid kernel's write stream take microseconds each.
template <int SL, int NT = 256>
__global__ __launch_bounds__(NT) void local_ppf_self_kernel(const float* __restrict__ xyz,
                                                             const float* __restrict__ nrm,
                                                             const int* __restrict__ idx, int n,
                                                             int k, int relative,
                                                             float* __restrict__ out,
                                                             const int* __restrict__ sidx,
                                                             const int* __restrict__ inv,
                                                             int npad, int* __restrict__ idx_out) {
  extern __shared__ __align__(16) float cl_s[];  // [6][n]: x y z nx ny nz
  (void)PCR_PRIO(2);
  const int tid = threadIdx.x;
  const int j = blockIdx.x * NT + tid;
  const int q0 = blockIdx.y * SL;
  const int b = blockIdx.z;
  const float* P = xyz + (size_t)b * 3 * n;
  const float* Nn = nrm + (size_t)b * 3 * n;
  int id[SL];
  if (sidx) {
    // neighbour ids in the selection's sorted query order: this point's row
    // position from the sort's inverse permutation; the ids are written out
    // in original order here, whole rows (the KNN output knn_idx)
    const int p = j < n ? inv[(size_t)b * n + j] : 0;
#pragma unroll
    for (int s = 0; s < SL; s++)
      id[s] = (j < n && q0 + s < k) ? sidx[((size_t)b * kKnnSortedK + q0 + s) * npad + p] : 0;
#pragma unroll
    for (int s = 0; s < SL; s++)
      if (j < n && q0 + s < k) idx_out[((size_t)b * k + q0 + s) * n + j] = id[s];
  } else {
#pragma unroll
    for (int s = 0; s < SL; s++)
      id[s] = (j < n && q0 + s < k) ? idx[((size_t)b * k + q0 + s) * n + j] : 0;
  }
  constexpr int E = kPpfSelfMaxN / NT;
  float st[E][6];
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = e * NT + tid;
    if (i < n) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        st[e][a] = P[(size_t)a * n + i];
        st[e][3 + a] = Nn[(size_t)a * n + i];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int i = e * NT + tid;
    if (i < n)
#pragma unroll
      for (int a = 0; a < 6; a++) cl_s[(size_t)a * n + i] = st[e][a];
  }
  __syncthreads();
  if (j >= n) return;
  const float cx = cl_s[j], cy = cl_s[n + j], cz = cl_s[2 * n + j];
  const float cnx = cl_s[3 * n + j], cny = cl_s[4 * n + j], cnz = cl_s[5 * n + j];
  float* O = out + (size_t)b * 4 * k * n;
#pragma unroll
  for (int s = 0; s < SL; s++) {
    const int q = q0 + s;
    if (q < k) {
      const unsigned si = (id[s] < 0 || id[s] >= n) ? 0u : (unsigned)id[s];
      float o[4];
      pcr_local_ppf(cx, cy, cz, cnx, cny, cnz, cl_s[si], cl_s[n + si], cl_s[2 * n + si],
                    cl_s[3 * n + si], cl_s[4 * n + si], cl_s[5 * n + si], relative, o);
      // nontemporal: the PPF rows are streamed out (c3 KNN + PPF 0.91 -> 0.85 ms)
#pragma unroll
      for (int ch = 0; ch < 4; ch++)
        __builtin_nontemporal_store(o[ch], &O[((size_t)ch * k + q) * n + j]);
    }
  }
}

// The same local PPF from the selection's sorted-order id rows
// (pcr_knn_select_ppf), one workgroup per (cloud, SL slots) covering every
// point of the cloud: the cloud's coordinates + normals and the SL id rows
// (sorted query order, KnnSet::sidx) are staged in LDS by coalesced loads,
// each exactly once per workgroup, and every neighbour / id lookup is an LDS
// read.  The per-256-point workgroups of local_ppf_self_kernel gathered the
// id rows through the sort's inverse permutation from global memory, each
// 4-byte gather on its own line, and the four workgroups of a (cloud, slot
// group) sat on different XCDs, so every XCD's L2 fetched the rows again:
// 44.6 MB of HBM traffic per c2 launch against 21.8 MB algorithmic
// (profiles/r03_pmc_traffic.json).  XCD-aware: the dispatcher deals
// workgroups round-robin over the 8 XCDs, so unit (id % 8) * (U / 8) + id / 8
// puts a cloud's slot groups on one XCD (its cloud is fetched into one L2).
// pcr_local_ppf (include/pcr_math.h) with the same bits, in fewer gfx950
// instructions:
//  - the three IEEE divisions by |d| share one refined reciprocal.  The
//    compiler's f32 division is v_div_scale, v_rcp, two FMA refining the
//    reciprocal, five FMA for the quotient, v_div_fmas and v_div_fixup; with
//    |d| and every nonzero numerator in [2^-60, 2^60] the scales are 1, fmas
//    is a plain FMA and fixup passes the quotient through, so the unscaled
//    sequence below yields the same bits (a zero numerator keeps its signed
//    zero, as fixup does).  A wave with any lane outside that range (|d| = 0
//    for the self pair, NaN, extreme scales) takes the plain divisions.
//  - the acos tails are selects, not branches.
__device__ inline float ppf_acos_sel(float x) {
  const float pio2_hi = 1.57079637e+00f, pio2_lo = -4.37113883e-08f;
  const float pi_hi = 3.14159274e+00f, pi_lo = -8.74227766e-08f;
  const float ax = __builtin_fabsf(x);
  const bool mid = ax <= 0.5f;
  const float s = mid ? x : __builtin_sqrtf((1.0f - ax) * 0.5f);
  const float p = pcr_asinf_core(s);
  const float t2 = 2.0f * p;
  const float rm = pio2_hi - (p - pio2_lo);
  const float rn = pi_hi - (t2 - pi_lo);
  const float rt = x > 0.0f ? t2 : rn;
  return mid ? rm : rt;
}
// |v| in [2^-60, 2^60] (NaN / inf excluded) by one unsigned range test on
// the bits; `zero_ok` also accepts +-0.  Bitwise, so no short-circuit branches.
__device__ inline bool ppf_div_safe(float v, bool zero_ok) {
  const unsigned a = __float_as_uint(v) & 0x7FFFFFFFu;
  constexpr unsigned lo = 0x21800000u, hi = 0x5D800000u;  // 2^-60, 2^60
  return ((a - lo) <= (hi - lo)) | (zero_ok & (a == 0u));
}
__device__ inline float ppf_div_shared(float a, float b, float y) {
  float q = a * y;
  float r = __builtin_fmaf(-b, q, a);
  q = __builtin_fmaf(r, y, q);
  r = __builtin_fmaf(-b, q, a);
  q = __builtin_fmaf(r, y, q);
  return a == 0.0f ? a : q;
}
// M pairs of one centre in lockstep (every step written for all M before the
// next), so their dependent chains interleave: the scheduler does not
// interleave whole calls by itself.  c[m] / p[m] = {x, y, z, nx, ny, nz} of
// pair m's centre / neighbour.
template <int M>
__device__ inline void ppf_local_dev(const float (&c)[M][6], const float (&p)[M][6], int relative,
                                     float (&out)[M][4]) {
  float dx[M], dy[M], dz[M], dn[M];
  int safe = 1;  // bitwise ANDs of the range tests: no short-circuit branches
#pragma unroll
  for (int m = 0; m < M; m++) {
    const float gx = relative ? p[m][0] - c[m][0] : p[m][0];
    const float gy = relative ? p[m][1] - c[m][1] : p[m][1];
    const float gz = relative ? p[m][2] - c[m][2] : p[m][2];
    dx[m] = c[m][0] - gx;
    dy[m] = c[m][1] - gy;
    dz[m] = c[m][2] - gz;
  }
#pragma unroll
  for (int m = 0; m < M; m++) dn[m] = __builtin_sqrtf(pcr_sumsq3f(dx[m], dy[m], dz[m]));
#pragma unroll
  for (int m = 0; m < M; m++)
    safe &= (int)ppf_div_safe(dn[m], false) & (int)ppf_div_safe(dx[m], true) &
            (int)ppf_div_safe(dy[m], true) & (int)ppf_div_safe(dz[m], true);
  float ux[M], uy[M], uz[M];
  if (__builtin_expect(__all(safe != 0), 1)) {
    float y[M];
#pragma unroll
    for (int m = 0; m < M; m++) y[m] = __builtin_amdgcn_rcpf(dn[m]);
#pragma unroll
    for (int m = 0; m < M; m++) y[m] = __builtin_fmaf(__builtin_fmaf(-dn[m], y[m], 1.0f), y[m], y[m]);
#pragma unroll
    for (int m = 0; m < M; m++) {
      ux[m] = ppf_div_shared(dx[m], dn[m], y[m]);
      uy[m] = ppf_div_shared(dy[m], dn[m], y[m]);
      uz[m] = ppf_div_shared(dz[m], dn[m], y[m]);
    }
  } else {
#pragma unroll
    for (int m = 0; m < M; m++) {
      ux[m] = dx[m] / dn[m];
      uy[m] = dy[m] / dn[m];
      uz[m] = dz[m] / dn[m];
    }
  }
#pragma unroll
  for (int m = 0; m < M; m++) {
    out[m][0] = pcr_clamp1f(pcr_dot3f(p[m][3], p[m][4], p[m][5], ux[m], uy[m], uz[m]));
    out[m][1] = pcr_clamp1f(pcr_dot3f(c[m][3], c[m][4], c[m][5], ux[m], uy[m], uz[m]));
    out[m][2] = pcr_clamp1f(pcr_dot3f(p[m][3], p[m][4], p[m][5], c[m][3], c[m][4], c[m][5]));
    out[m][3] = dn[m];
  }
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int m = 0; m < M; m++) out[m][a] = ppf_acos_sel(out[m][a]);
}

// LDS layout of local_ppf_cloud_kernel: [3][n] coordinates, [3][n] normals,
// [SL][npad] id rows, each region padded to whole LDS-DMA pieces of width V
struct PpfLds {
  int nrm_off, ids_off, bytes;  // byte offsets / total
};
__host__ __device__ inline PpfLds ppf_lds_layout(int n, int sl, int npad, int v) {
  PpfLds l;
  l.nrm_off = lds_dma_pad(12 * n, v);
  l.ids_off = 2 * l.nrm_off;
  l.bytes = l.ids_off + lds_dma_pad(4 * sl * npad, v);
  return l;
}

template <int SL, int V, int NT = 512>
__global__ __launch_bounds__(NT) void local_ppf_cloud_kernel(const float* __restrict__ xyz,
                                                              const float* __restrict__ nrm, int n,
                                                              int k, int relative,
                                                              float* __restrict__ out,
                                                              const int* __restrict__ sidx,
                                                              const int* __restrict__ inv,
                                                              int npad, int* __restrict__ idx_out,
                                                              int pr) {
  extern __shared__ __align__(16) float cl_s[];  // PpfLds: x y z | nx ny nz | id rows
  constexpr int PT = kPpfSelfMaxN / NT;  // points per thread at most
  const int G = (k + SL - 1) / SL;
  const int U = gridDim.x;
  const int id = blockIdx.x;
  const int u = (U % 8 == 0) ? (id % 8) * (U / 8) + id / 8 : id;
  // unit u = (cloud, slot group, point range): a cloud's units are
  // consecutive, so the XCD-aware order keeps them on one XCD
  const int b = u / (G * pr);
  const int rem = u - b * G * pr;
  const int q0 = (rem / pr) * SL;
  const int span = (n + pr - 1) / pr;  // points of this workgroup's range
  const int j0 = (rem % pr) * span, j1 = min(n, j0 + span);
  const int sl = min(SL, k - q0);
  const int tid = threadIdx.x;
  // this thread's points' rows in sorted order, loaded before the staging
  int p[PT];
#pragma unroll
  for (int e = 0; e < PT; e++) {
    const int j = j0 + e * NT + tid;
    p[e] = j < j1 ? inv[(size_t)b * n + j] : 0;
  }
  // the cloud and the id rows straight into LDS (LDS-DMA: every piece in
  // flight at once, one round trip; a loop of loads and LDS stores waited for
  // each of its ~14 trips in turn)
  const PpfLds L = ppf_lds_layout(n, SL, npad, V);
  const float* nl_s = cl_s + L.nrm_off / 4;
  const int* id_s = (const int*)(cl_s + L.ids_off / 4);
  lds_dma_copy<V>(cl_s, xyz + (size_t)b * 3 * n, 12 * n);
  lds_dma_copy<V>((float*)nl_s, nrm + (size_t)b * 3 * n, 12 * n);
  lds_dma_copy<V>((int*)id_s, sidx + ((size_t)b * kKnnSortedK + q0) * npad, 4 * sl * npad);
  wait_vmcnt<0>();
  __syncthreads();
  float* O = out + (size_t)b * 4 * k * n;
  int* I = idx_out + (size_t)b * k * n;
#pragma unroll
  for (int e = 0; e < PT; e++) {
    const int j = j0 + e * NT + tid;
    if (j >= j1) break;
    const float cx = cl_s[j], cy = cl_s[n + j], cz = cl_s[2 * n + j];
    const float cnx = nl_s[j], cny = nl_s[n + j], cnz = nl_s[2 * n + j];
    // the SL slots in lockstep (slots past sl compute on neighbour 0 and are
    // not stored)
    float nb[SL][6];
#pragma unroll
    for (int s = 0; s < SL; s++) {
      const int jd = s < sl ? id_s[s * npad + p[e]] : 0;
      if (s < sl) I[(size_t)(q0 + s) * n + j] = jd;
      const unsigned si = (jd < 0 || jd >= n) ? 0u : (unsigned)jd;
      nb[s][0] = cl_s[si];
      nb[s][1] = cl_s[n + si];
      nb[s][2] = cl_s[2 * n + si];
      nb[s][3] = nl_s[si];
      nb[s][4] = nl_s[n + si];
      nb[s][5] = nl_s[2 * n + si];
    }
    float ce[SL][6], o[SL][4];
#pragma unroll
    for (int s = 0; s < SL; s++) {
      ce[s][0] = cx;
      ce[s][1] = cy;
      ce[s][2] = cz;
      ce[s][3] = cnx;
      ce[s][4] = cny;
      ce[s][5] = cnz;
    }
    ppf_local_dev<SL>(ce, nb, relative, o);
    // nontemporal: the PPF rows are streamed out
#pragma unroll
    for (int s = 0; s < SL; s++)
      if (s < sl)
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
          __builtin_nontemporal_store(o[s][ch], &O[((size_t)ch * k + q0 + s) * n + j]);
  }
}

// The same with four consecutive points per thread and one slot (needs n %
// 4 == 0 and 16-byte aligned rows): every output store is a 16-byte vector
// (five per thread instead of twenty 4-byte stores, the id row included), and
// the four pairs run in lockstep.  Work item f = (slot s, quad qd) of the
// workgroup's SL slots x span / 4 quads, taken in turn by its threads.
typedef float ppf_f4 __attribute__((ext_vector_type(4)));
typedef int ppf_i4 __attribute__((ext_vector_type(4)));
template <int SL, int NT = 512>
__global__ __launch_bounds__(NT) void local_ppf_quad_kernel(const float* __restrict__ xyz,
                                                             const float* __restrict__ nrm, int n,
                                                             int k, int relative,
                                                             float* __restrict__ out,
                                                             const int* __restrict__ sidx,
                                                             const int* __restrict__ inv,
                                                             int npad, int* __restrict__ idx_out,
                                                             int pr) {
  extern __shared__ __align__(16) float cl_s[];  // PpfLds: x y z | nx ny nz | id rows
  const int G = (k + SL - 1) / SL;
  const int U = gridDim.x;
  const int id = blockIdx.x;
  const int u = (U % 8 == 0) ? (id % 8) * (U / 8) + id / 8 : id;
  const int b = u / (G * pr);
  const int rem = u - b * G * pr;
  const int q0 = (rem / pr) * SL;
  const int span = ((n + pr - 1) / pr + 3) & ~3;  // whole quads
  const int j0 = (rem % pr) * span, j1 = min(n, j0 + span);
  const int nq = (j1 - j0) >> 2;
  const int sl = min(SL, k - q0);
  const int tid = threadIdx.x;
  const PpfLds L = ppf_lds_layout(n, SL, npad, 16);
  const float* nl_s = cl_s + L.nrm_off / 4;
  const int* id_s = (const int*)(cl_s + L.ids_off / 4);
  lds_dma_copy<16>(cl_s, xyz + (size_t)b * 3 * n, 12 * n);
  lds_dma_copy<16>((float*)nl_s, nrm + (size_t)b * 3 * n, 12 * n);
  lds_dma_copy<16>((int*)id_s, sidx + ((size_t)b * kKnnSortedK + q0) * npad, 4 * sl * npad);
  wait_vmcnt<0>();
  __syncthreads();
  float* O = out + (size_t)b * 4 * k * n;
  int* I = idx_out + (size_t)b * k * n;
  const int* pinv = inv + (size_t)b * n;
  for (int f = tid; f < sl * nq; f += NT) {
    const int s = f / nq;
    const int j = j0 + 4 * (f - s * nq);
    const int q = q0 + s;
    // the quad's rows in sorted order (inv), its ids, centres and neighbours
    const int4 pv = *(const int4*)(pinv + j);
    const int pp[4] = {pv.x, pv.y, pv.z, pv.w};
    int jd[4];
    float ce[4][6], nb[4][6], o[4][4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      jd[m] = id_s[s * npad + pp[m]];
      const unsigned si = (jd[m] < 0 || jd[m] >= n) ? 0u : (unsigned)jd[m];
      nb[m][0] = cl_s[si];
      nb[m][1] = cl_s[n + si];
      nb[m][2] = cl_s[2 * n + si];
      nb[m][3] = nl_s[si];
      nb[m][4] = nl_s[n + si];
      nb[m][5] = nl_s[2 * n + si];
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float4 cv = *(const float4*)(cl_s + a * n + j);
      const float4 nv = *(const float4*)(nl_s + a * n + j);
      ce[0][a] = cv.x;
      ce[1][a] = cv.y;
      ce[2][a] = cv.z;
      ce[3][a] = cv.w;
      ce[0][3 + a] = nv.x;
      ce[1][3 + a] = nv.y;
      ce[2][3 + a] = nv.z;
      ce[3][3 + a] = nv.w;
    }
    __builtin_nontemporal_store(ppf_i4{jd[0], jd[1], jd[2], jd[3]}, (ppf_i4*)(I + (size_t)q * n + j));
    ppf_local_dev<4>(ce, nb, relative, o);
#pragma unroll
    for (int ch = 0; ch < 4; ch++)
      __builtin_nontemporal_store(ppf_f4{o[0][ch], o[1][ch], o[2][ch], o[3][ch]},
                                  (ppf_f4*)(O + ((size_t)ch * k + q) * n + j));
  }
}

}  // namespace pcr

using namespace pcr;

extern "C" pcr_status pcr_knn_ppf_sorted(const float* xyz, const float* normals, int b, int n,
                                         int k, int relative, int* idx, float* ppf,
                                         const void* workspace, size_t workspace_bytes,
                                         void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 1 && k >= 1 && k <= kKnnSortedK && n <= kPpfSelfMaxN,
              "knn_ppf_sorted: invalid sizes (k <= 32, n <= 2048)");
  PCR_REQUIRE(idx != nullptr && ppf != nullptr, "knn_ppf_sorted: idx and ppf required");
  if (b == 0) return PCR_OK;
  const int* sidx = nullptr;
  const int* inv = nullptr;
  int npad = 0;
  PCR_REQUIRE(workspace != nullptr && workspace_bytes >= pcr_knn_workspace_size(b, n, n) &&
                  knn_sorted_views(const_cast<void*>(workspace), b, n, &sidx, &inv, &npad),
              "knn_ppf_sorted: workspace without sorted neighbour rows");
  // clouds of <= 1024 points: one workgroup per (cloud, 2 slots, 512
  // points), 256 threads of four points each (round 6: 2 slots x 256 threads
  // rather than 4 x 512, twice the workgroups -- c2 +0.5%, pairs +2%, c3
  // within noise, profiles/r06_ab_ppf_shape.log; 4 slots over 256-point
  // ranges was slower).  At 2048 points splitting a workgroup's points
  // re-stages the 48 KB cloud per range (c3: 100 -> 160 us), so those keep
  // one workgroup per (cloud, 2 slots).
  constexpr int SL = 2;
  constexpr int NT = 256;
  const int pr = n <= 1024 ? ceil_div(n, 512) : 1;
  // 16-byte LDS-DMA pieces and output vectors when every row is 16-byte
  // aligned: four points per thread (local_ppf_quad_kernel)
  const bool v16 = n % 4 == 0 && npad % 4 == 0 &&
                   (((uintptr_t)xyz | (uintptr_t)normals | (uintptr_t)sidx | (uintptr_t)inv |
                     (uintptr_t)idx | (uintptr_t)ppf) & 15) == 0;
  const dim3 grid(b * ceil_div(k, SL) * pr);
  if (v16) {
    const size_t lds = ppf_lds_layout(n, SL, npad, 16).bytes;
    allow_big_lds(local_ppf_quad_kernel<SL, NT>, lds);
    hipLaunchKernelGGL((local_ppf_quad_kernel<SL, NT>), grid, dim3(NT), lds, as_stream(stream),
                       xyz, normals, n, k, relative, ppf, sidx, inv, npad, idx, pr);
  } else {
    const size_t lds = ppf_lds_layout(n, SL, npad, 4).bytes;
    allow_big_lds(local_ppf_cloud_kernel<SL, 4>, lds);
    hipLaunchKernelGGL((local_ppf_cloud_kernel<SL, 4>), grid, dim3(512), lds, as_stream(stream),
                       xyz, normals, n, k, relative, ppf, sidx, inv, npad, idx, pr);
  }
  return launch_status("knn_ppf_sorted");
}

extern "C" pcr_status pcr_spherical_ppf_forward(const float* coords, const float* center,
                                                const float* normals, const float* center_normal,
                                                int b, int n, float* feat, void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 0, "spherical_ppf_forward: invalid sizes");
  if (b == 0 || n == 0) return PCR_OK;
  hipLaunchKernelGGL(global_ppf_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0,
                     as_stream(stream), coords, center, normals, center_normal, n, feat);
  return launch_status("spherical_ppf_forward");
}

extern "C" pcr_status pcr_local_ppf_forward(const float* points, const float* normals,
                                            const float* centers, const float* center_normals,
                                            const int* idx, int b, int n, int m, int u,
                                            int idx_kmajor, int relative, float* out,
                                            void* stream) {
  PCR_REQUIRE(b >= 0 && n >= 1 && m >= 0 && u >= 0, "local_ppf_forward: invalid sizes");
  PCR_REQUIRE(u <= 65535, "local_ppf_forward: u too large");
  if (b == 0 || m == 0 || u == 0) return PCR_OK;
  PCR_PRIO_INIT();
  if (points == centers && normals == center_normals && n == m && idx_kmajor &&
      n <= kPpfSelfMaxN) {
#define PCR_PPF_SELF(SLV)                                                                     \
  hipLaunchKernelGGL((local_ppf_self_kernel<SLV>), dim3(ceil_div(n, 256), ceil_div(u, SLV), b), \
                     dim3(256), (size_t)6 * n * 4, as_stream(stream), points, normals, idx, n,  \
                     u, relative, out, nullptr, nullptr, 0, nullptr)
    PCR_PPF_SELF(8);
#undef PCR_PPF_SELF
    return launch_status("local_ppf_forward");
  }
  hipLaunchKernelGGL(local_ppf_kernel, dim3(ceil_div(m, 256), u, b), dim3(256), 0,
                     as_stream(stream), points, normals, centers, center_normals, idx, n, m, u,
                     idx_kmajor, relative, out);
  return launch_status("local_ppf_forward");
}
