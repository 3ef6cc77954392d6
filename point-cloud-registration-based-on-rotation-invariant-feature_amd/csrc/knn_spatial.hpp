// knn_spatial.hpp -- what the files of the Morton-sorted exact KNN share
// (knn_spatial.hip: the entry, its ladder and the threshold selection;
// knn_sort.hip, knn_block.hip, knn_wsel.hip: one kernel family each, with its
// launcher) and what knn.hip, local_ppf.hip and the runner call of it.
#pragma once

#include "common.hpp"

namespace pcr {

// knn_spatial.hip: Morton-sorted exact KNN of xyz1 [b,3,n] in xyz2 [b,3,m]
// (self: the same set).  Returns PCR_ERR_UNSUPPORTED without launching
// anything when it does not apply.
enum KnnStage : int {
  kKnnSort = 1,        // sort the point sets into the workspace
  kKnnSelect = 2,      // select from an already sorted workspace
  kKnnSortedRows = 4,  // with kKnnSelect: the selection only writes its neighbour
                       // ids in sorted query order into the workspace (self,
                       // k <= 32, clouds of <= 2048 points, idx1 alone)
};
// Its optional outputs and PPF inputs; anything may stay null.
struct KnnIO {
  float* dist1 = nullptr;  // [b,k,n] xyz1's neighbours in xyz2
  int* idx1 = nullptr;
  float* dist2 = nullptr;  // [b,k,m] the other direction, run when idx2 is set
  int* idx2 = nullptr;
  // fused local PPF of direction 1 into ppf1 [b,4,k,n]: both sets' normals
  const float *nrm1 = nullptr, *nrm2 = nullptr;
  int relative = 0;
  float* ppf1 = nullptr;
};
pcr_status knn_spatial(const float* xyz1, const float* xyz2, int b, int n, int m, int k,
                       const KnnIO& io, void* ws, size_t ws_bytes, bool self, hipStream_t st,
                       int stages = kKnnSort | kKnnSelect);
// views of kKnnSortedRows' output and of the sort's inverse permutation
constexpr int kKnnSortedK = 32;
bool knn_sorted_views(void* ws, int b, int n, const int** sidx, const int** inv, int* npad);
// the local PPF kernels that read those rows stage a whole cloud in LDS
constexpr int kPpfSelfMaxN = 2048;

// knn.hip: selection + local PPF of a prepared (sorted) workspace, the
// one ladder behind pcr_knn_select_ppf and the runner.  Without dist: the
// selection writes its neighbour ids in sorted query order -- whole rows --
// and the PPF kernel reads them back through the sort's inverse permutation
// while it writes knn_idx [b,k,n] (original order) and the PPF [b,4,k,n].
// With dist, or on shapes outside that path (k > 32, clouds of more than 2048
// points, no sorted views): pcr_knn_local_ppf_prepared (selection only) +
// pcr_local_ppf_forward, same outputs.
pcr_status knn_select_ppf_prepared(const float* xyz, const float* normals, int b, int n, int k,
                                   int relative, int* idx, float* dist, float* ppf,
                                   const void* workspace, size_t workspace_bytes, void* stream);

// ------------------------------------------------------------- workspace
constexpr int kKnnMaxSortN = 4096;        // single-workgroup LDS sort up to here
constexpr int kBigCellBits = 15;          // top Morton bits of the global sort (32^3 cells)
constexpr int kBigCells = 1 << kBigCellBits;
constexpr int kBlk = 64;

struct KnnSet {
  float* x;   // [b][npad] sorted coordinates (NaN padding)
  float* y;
  float* z;
  int* j;     // [b][npad] original index (-1 padding)
  float* box; // [b][nblk][8] min xyz, max xyz, -, -
  // clouds of more than kKnnMaxSortN points (global counting sort):
  int* cell;     // [b][kBigCells] counts, then starts
  int* pcell;    // [b][n] cell of each point
  int* pslot;    // [b][n] arrival slot inside the cell
  float* frame;  // [b][8] lo xyz, scale xyz
  int* inv;   // [b][n] sorted position of every point (the sort's inverse)
  // clouds of <= kSortedMaxN points (the LDS-cached selection):
  int* sidx;  // [b][kSortedK][npad] neighbour ids in sorted query order
  // larger clouds: the selection's keys, query-major in sorted query order
  double* skey;  // [b][npad][kSkeyK] (d bits << 32 | index), see make_key
  float* rec;    // [b][n][8] x y z nx ny nz - -: the emit kernel's neighbour gathers
  int n, npad, nblk;
};

// the cached selection can emit its neighbour ids in sorted (Morton) query
// order -- whole 256-byte rows -- and the local PPF kernel un-permutes them
// while it writes its own outputs (knn_select_ppf_sorted); writing them in
// original order from the selection is one scattered 4-byte store per
// (query, slot): ~7x the write requests of the 4 MB they carry at c2
constexpr int kSortedMaxN = 2048;
constexpr int kSortedK = kKnnSortedK;
// past kSortedMaxN queries the selection writes its k keys per query as one
// contiguous row in sorted query order (a workgroup's 64 rows are one
// contiguous range) and knn_emit_kernel un-permutes them into the outputs:
// writing them from the selection in original order was one scattered
// 4-byte store per (query, slot, output) -- at c5 5 x 134 M stores, which
// slowed the whole launch by ~30%
constexpr int kSkeyK = 64;

inline size_t knn_set_layout(int b, int n, KnnSet* s, char* base, size_t off) {
  const int nblk = (n + kBlk - 1) / kBlk;
  const int npad = nblk * kBlk;
  auto take = [&](size_t bytes) {
    char* q = base ? base + off : nullptr;
    off = align_up(off + bytes, 256);
    return q;
  };
  float* x = (float*)take((size_t)b * npad * 4);
  float* y = (float*)take((size_t)b * npad * 4);
  float* z = (float*)take((size_t)b * npad * 4);
  int* j = (int*)take((size_t)b * npad * 4);
  float* box = (float*)take((size_t)b * nblk * 8 * 4);
  const bool big = n > kKnnMaxSortN;
  int* cell = big ? (int*)take((size_t)b * kBigCells * 4) : nullptr;
  int* pcell = big ? (int*)take((size_t)b * n * 4) : nullptr;
  int* pslot = big ? (int*)take((size_t)b * n * 4) : nullptr;
  float* frame = big ? (float*)take((size_t)b * 8 * 4) : nullptr;
  const bool sorted_out = n <= kSortedMaxN;
  int* inv = (int*)take((size_t)b * n * 4);
  int* sidx = sorted_out ? (int*)take((size_t)b * kSortedK * npad * 4) : nullptr;
  double* skey = sorted_out ? nullptr : (double*)take((size_t)b * npad * kSkeyK * 8);
  float* rec = (float*)take((size_t)b * n * 8 * 4);
  if (s) {
    s->rec = rec;
    s->inv = inv;
    s->sidx = sidx;
    s->skey = skey;
    s->cell = cell;
    s->pcell = pcell;
    s->pslot = pslot;
    s->frame = frame;
    s->x = x;
    s->y = y;
    s->z = z;
    s->j = j;
    s->box = box;
    s->n = n;
    s->npad = npad;
    s->nblk = nblk;
  }
  return off;
}

// ------------------------------------------------------------------ keys
// Top-k in registers as packed keys (float bits of the squared distance << 32
// | index).  Squared distances are >= +0 or NaN, so unsigned key order is the
// lexicographic (distance, index) order.  The same 64 bits read as an IEEE
// double have the same order (positive, non-NaN doubles order like their
// bits), so compare-exchanges are one v_min_f64 + one v_max_f64 -- no lane
// masks, no VCC hazards, full ILP -- instead of two 64-bit integer compares
// and four selects.  Keys of NaN distances never enter the array (they fail
// the `< k-th` test).  f64 denormals (distance 0 with small index) are
// preserved by the default float mode.  Valid region = the last k slots; the
// first KMAX-k hold +0.0 and are never displaced.
typedef double kkey;
#define PCR_KEY_PAD 1.7976931348623157e308  // DBL_MAX: above every real key

__device__ inline kkey make_key(float d, int j) {
  // sign cleared: a NaN distance (e.g. a NaN-padded candidate; subtraction
  // flips the NaN's sign) must read as a huge positive key, never negative
  return __longlong_as_double((long long)(((unsigned long long)(__float_as_uint(d) & 0x7FFFFFFFu)
                                           << 32) | (unsigned)j));
}
// a taken key (d below a finite cut: never NaN, and a sum of squares is
// never negative) needs no sign clearing
__device__ inline kkey make_key_finite(float d, int j) {
  return __longlong_as_double(
      (long long)(((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j));
}
__device__ inline float key_dist(kkey k) {
  return __uint_as_float((unsigned)((unsigned long long)__double_as_longlong(k) >> 32));
}
__device__ inline int key_idx(kkey k) {
  return (int)(unsigned)((unsigned long long)__double_as_longlong(k) & 0xFFFFFFFFull);
}

// ------------------------------------------------- distances and boxes
__device__ inline float readlane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Lower bound of the FMA-chain squared distance from q to any point of box.
__device__ inline float box_lb(float qx, float qy, float qz, const float* bx) {
  const float gx = qx < bx[0] ? bx[0] - qx : (qx > bx[3] ? qx - bx[3] : 0.0f);
  const float gy = qy < bx[1] ? bx[1] - qy : (qy > bx[4] ? qy - bx[4] : 0.0f);
  const float gz = qz < bx[2] ? bx[2] - qz : (qz > bx[5] ? qz - bx[5] : 0.0f);
  float d = gx * gx;
  d = __builtin_fmaf(gy, gy, d);
  d = __builtin_fmaf(gz, gz, d);
  return d;
}

// Upper bound of the FMA-chain squared distance from q to any point of box.
__device__ inline float box_ub(float qx, float qy, float qz, const float* bx) {
  const float gx = fmaxf(fabsf(qx - bx[0]), fabsf(qx - bx[3]));
  const float gy = fmaxf(fabsf(qy - bx[1]), fabsf(qy - bx[4]));
  const float gz = fmaxf(fabsf(qz - bx[2]), fabsf(qz - bx[5]));
  float d = gx * gx;
  d = __builtin_fmaf(gy, gy, d);
  d = __builtin_fmaf(gz, gz, d);
  return d;
}

// -------------------------------------------------------------- launchers
// Each file launches its own kernels and picks the instantiation from these
// runtime arguments; knn_spatial.hip's ladder decides which of them run.

// One direction of a selection (queries qs against candidates cs): its
// outputs and, for the fused local PPF, both sets' original coordinates and
// normals.  Anything may be null.
struct KnnDir {
  float* dist = nullptr;
  int* idx = nullptr;
  const float *qxyz = nullptr, *qnrm = nullptr, *cxyz = nullptr, *cnrm = nullptr;
  int relative = 0;
  float* ppf = nullptr;
};

// knn_sort.hip: sorts pts [b,3,n] into s
void launch_sort(const float* pts, int b, int n, const KnnSet& s, hipStream_t st);
// knn_block.hip: knn_block_kernel, 32 < k <= 128; ppf: with the fused local PPF
void launch_block_kernel(const KnnSet& qs, const KnnSet& cs, int b, int k, const KnnDir& d,
                         hipStream_t st, bool ppf);
// knn_wsel.hip: knn_wsel_kernel, self KNN of clouds of <= 1024 points,
// k <= kSortedK, neighbour ids into s.sidx
void launch_wsel(const KnnSet& s, int b, int k, hipStream_t st);

}  // namespace pcr
