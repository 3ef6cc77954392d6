/*
 * pcr_amd.h -- C ABI of libpcr_amd.so, the MI355X (gfx950) implementation of
 * the rotation-invariant-feature hot path of
 * Gilgamesh666666/Point-cloud-registration-based-on-rotation-invariant-feature.
 *
 * Each entry point replaces one function of the reference's pybind11 module
 * `_multi_shape_pvcnn_backend` (PVCNN/modules/functional/src/bindings.cpp) or
 * one PyTorch block of the reference model; the citation above every
 * declaration names the interface it replaces (paths relative to the
 * reference's PVCNN/ directory).
 *
 * Conventions
 *  - Plain device pointers (HIP device memory), sizes as int, layouts exactly
 *    as the reference's tensors (channel-major [B, C, N] fp32, int32 indices).
 *  - The caller owns every buffer.  Outputs are FULLY written by the library,
 *    including the slots the reference leaves at their torch::zeros /
 *    ones*10000 fill, so callers may pass uninitialised (torch.empty) memory.
 *  - `stream` is a hipStream_t (NULL = legacy default stream).  Work is only
 *    enqueued; nothing synchronises, allocates or frees, so every call is
 *    hipGraph-capturable.  Calls needing scratch take a caller-provided
 *    workspace whose size comes from the matching *_workspace_size().
 *  - Return value: PCR_OK or a negative pcr_status; pcr_last_error() holds a
 *    message (thread-local).  The reference instead exit(-1)s on a launch
 *    failure (src/cuda_utils.cuh:28-37).
 */
#ifndef PCR_AMD_H
#define PCR_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int pcr_status;
#define PCR_OK 0
#define PCR_ERR_INVALID (-1)
#define PCR_ERR_LAUNCH (-2)
#define PCR_ERR_UNSUPPORTED (-3)

/* Last error message of the calling thread ("" when none). */
const char *pcr_last_error(void);
/* Library version string. */
const char *pcr_version(void);
/* A HIP stream restricted to the CUs set in mask (nwords 32-bit words, bit
 * i = CU i of the runtime's numbering; hipExtStreamCreateWithCUMask), and its
 * release.  No reference counterpart: a scheduling tool for the runner's
 * queues. */
pcr_status pcr_stream_create_cu_mask(const unsigned *mask, int nwords, void **stream);
pcr_status pcr_stream_destroy(void *stream);

/* ---------------------------------------------------------------- KNN ----
 * knn_forward_cuda (modules/functional/src/knn/knn.cpp:6-25, kernel
 * knn/knn.cu:5-49, both directions): xyz1 [b,c,n], xyz2 [b,c,m] ->
 * dist1 [b,k,n], idx1 [b,k,n] (into xyz2), dist2 [b,k,m], idx2 [b,k,m].
 * Squared L2, ascending, ties by lower index, unfilled slots (10000, 0). */
pcr_status pcr_knn_forward(const float *xyz1, const float *xyz2, int b, int c, int n, int m,
                           int k, float *dist1, float *dist2, int *idx1, int *idx2,
                           void *workspace, size_t workspace_bytes, void *stream);
/* Scratch of the spatially pruned KNN (Morton-sorted copies + block boxes of
 * both point sets).  With workspace == NULL (or c != 3, or more than 4096
 * points per cloud) a brute-force kernel is used instead, same results. */
size_t pcr_knn_workspace_size(int b, int n, int m);

/* knn_backward_cuda (knn/knn.cpp:27-52, kernel knn/knn.cu:52-78, :88-98).
 * gradxyz1 [b,c,n], gradxyz2 [b,c,m]; both directions accumulate into both. */
pcr_status pcr_knn_backward(const float *xyz1, const float *xyz2, const float *graddist1,
                            const float *graddist2, const int *idx1, const int *idx2, int b,
                            int c, int n, int m, int k, float *gradxyz1, float *gradxyz2,
                            void *stream);
/* The same without atomics (bit-repeatable): each direction's (query, slot)
 * pairs counting-sorted by neighbour in `workspace`
 * (pcr_knn_backward_workspace_size bytes), then one gather per point of its
 * own terms and of the pairs naming it.  Clouds of more than 16384 points
 * take pcr_knn_backward. */
size_t pcr_knn_backward_workspace_size(int b, int n, int m, int k);
pcr_status pcr_knn_backward_ws(const float *xyz1, const float *xyz2, const float *graddist1,
                               const float *graddist2, const int *idx1, const int *idx2, int b,
                               int c, int n, int m, int k, float *gradxyz1, float *gradxyz2,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- PPF ----
 * spherical_ppf_forward (modules/functional/src/spherical_ppf/ppf.cpp:17-36,
 * kernel ppf.cu:19-92).  Argument order of the BACKEND (points first); the
 * Python ppf() wrapper swaps (modules/functional/ppf.py:20).
 * coords/center/normals/center_normal [b,3,n] -> feat [b,4,n]. */
pcr_status pcr_spherical_ppf_forward(const float *coords, const float *center,
                                     const float *normals, const float *center_normal, int b,
                                     int n, float *feat, void *stream);

/* Local k-neighbour PPF of the model (models/pvcnn_classify.py:252-269:
 * BallQuery grouping of coords+normals, d = c - (p - c), three acos + |d|),
 * fused with the grouping.  points/normals [b,3,n]; centers/center_normals
 * [b,3,m]; idx either [b,m,u] (ball_query layout, idx_kmajor=0) or [b,u,m]
 * (knn layout, idx_kmajor=1).  relative=1 reproduces the model (grouped
 * coordinates are relative to the centre), relative=0 uses d = c - p.
 * out [b,4,u,m] = (nr_d, ni_d, nr_ni, |d|). */
pcr_status pcr_local_ppf_forward(const float *points, const float *normals, const float *centers,
                                 const float *center_normals, const int *idx, int b, int n,
                                 int m, int u, int idx_kmajor, int relative, float *out,
                                 void *stream);

/* Fused self-KNN + local PPF (the extractor's neighbour stage): for every
 * point of xyz [b,3,n] its k nearest points (self included, knn semantics)
 * -> idx [b,k,n], dist [b,k,n] (may be NULL) and the local PPF
 * [b,4,k,n] of (point, neighbour) with `relative` as above.  Workspace:
 * pcr_knn_workspace_size(b, n, n). */
pcr_status pcr_knn_local_ppf(const float *xyz, const float *normals, int b, int n, int k,
                             int relative, int *idx, float *dist, float *ppf, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The two launches of pcr_knn_local_ppf, separately, so a pipelined caller
 * can sort step i+1 while step i selects (double-buffered workspaces):
 * prepare = Morton sort of xyz into the workspace, prepared = selection +
 * PPF from that workspace (ppf == NULL: selection only; the PPF can then
 * come from pcr_local_ppf_forward with idx_kmajor = 1, one thread per
 * output, coalesced).  Both return PCR_ERR_UNSUPPORTED (nothing
 * launched) where the sorted path does not apply (n > 4096); use
 * pcr_knn_local_ppf there. */
pcr_status pcr_knn_prepare(const float *xyz, int b, int n, void *workspace,
                           size_t workspace_bytes, void *stream);
pcr_status pcr_knn_local_ppf_prepared(const float *xyz, const float *normals, int b, int n, int k,
                                      int relative, int *idx, float *dist, float *ppf,
                                      const void *workspace, size_t workspace_bytes,
                                      void *stream);
/* Selection + local PPF of a prepared workspace in two launches whose only
 * scattered traffic is a read: the selection emits its neighbour ids in
 * sorted (Morton) query order into the workspace -- whole rows -- and the PPF
 * kernel reads them back through the sort's inverse permutation while it
 * writes knn_idx [b,k,n] (original order) and ppf [b,4,k,n].  k <= 32 and
 * n <= 2048 take that path; other shapes run pcr_knn_local_ppf_prepared +
 * pcr_local_ppf_forward.  Same outputs as those two calls. */
pcr_status pcr_knn_select_ppf(const float *xyz, const float *normals, int b, int n, int k,
                              int relative, int *idx, float *ppf, const void *workspace,
                              size_t workspace_bytes, void *stream);
/* The two launches of pcr_knn_select_ppf separately: the selection into the
 * workspace's sorted-order rows (PCR_ERR_UNSUPPORTED, nothing launched, when
 * that path does not apply), then the PPF launch that writes knn_idx and
 * ppf from them (k <= 32, n <= 2048). */
pcr_status pcr_knn_select_sorted(const float *xyz, int b, int n, int k, const void *workspace,
                                 size_t workspace_bytes, void *stream);
pcr_status pcr_knn_ppf_sorted(const float *xyz, const float *normals, int b, int n, int k,
                              int relative, int *idx, float *ppf, const void *workspace,
                              size_t workspace_bytes, void *stream);

/* ------------------------------------------------ ball query / grouping --
 * ball_query (ball_query/ball_query.cpp:6-30, kernel ball_query.cu:19-50):
 * centers [b,3,m], points [b,3,n] -> idx [b,m,u]. */
pcr_status pcr_ball_query(const float *centers, const float *points, int b, int m, int n,
                          float radius, int u, int *idx, void *stream);

/* grouping_forward (grouping/grouping.cpp:6-24, grouping.cu:18-36):
 * features [b,c,n], indices [b,m,u] -> out [b,c,m,u]. */
pcr_status pcr_grouping_forward(const float *features, const int *indices, int b, int c, int n,
                                int m, int u, float *out, void *stream);

/* grouping_backward (grouping.cpp:26-44, grouping.cu:58-85):
 * grad_y [b,c,m,u], indices [b,m,u] -> grad_x [b,c,n]. */
pcr_status pcr_grouping_backward(const float *grad_y, const int *indices, int b, int c, int n,
                                 int m, int u, float *grad_x, void *stream);

/* ------------------------------------------------------- voxelization ----
 * Scratch for the voxelizers: per-cloud sort permutation, occupied-voxel
 * segments and an occupancy bitmap with word prefix counts. */
size_t pcr_voxelize_workspace_size(int b, int n, int r);
/* The same for c feature channels.  Clouds of more than 4096 points use the
 * sorted large-cloud path; with this size it also keeps a point-major copy
 * of the features, so each voxel reads its points' channels contiguously
 * (several times faster).  The results are identical either way. */
size_t pcr_voxelize_workspace_size_c(int b, int c, int n, int r);

/* spherical_avg_voxelize_forward (spherical_voxelization/spherical_vox.cpp:17-46,
 * kernels spherical_vox.cu:19-125): features [b,c,n], normalised coords
 * [b,3,n] -> out [b,c,r^3] (voxel mean), ind [b,n] (-1 = dropped),
 * cnt [b,r^3].  Means are accumulated in ascending point order. */
pcr_status pcr_spherical_avg_voxelize_forward(const float *features, const float *coords, int b,
                                              int c, int n, int r, float *out, int *ind, int *cnt,
                                              void *workspace, size_t workspace_bytes,
                                              void *stream);

/* avg_voxelize_forward (voxelization/vox.cpp:17-46, vox.cu:18-73): cube
 * variant on int voxel coords [b,3,n]. */
pcr_status pcr_avg_voxelize_forward(const float *features, const int *coords, int b, int c,
                                    int n, int r, float *out, int *ind, int *cnt,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* spherical_avg_voxelize_backward (spherical_vox.cpp:57-79, spherical_vox.cu:139-163)
 * and avg_voxelize_backward (vox.cpp:57-76, vox.cu:87-111): grad_y [b,c,r3],
 * ind [b,n], cnt [b,r3] -> grad_x [b,c,n]. */
pcr_status pcr_avg_voxelize_backward(const float *grad_y, const int *ind, const int *cnt, int b,
                                     int c, int n, int r3, float *grad_x, void *stream);

/* Spherical_Voxelization's coordinate normalisation
 * (modules/spherical_vox.py:16-20) with a fixed reduction order:
 * coords [b,3,n] -> norm_coords [b,3,n]. */
pcr_status pcr_spherical_normalize(const float *coords, int b, int n, float *norm_coords,
                                   void *stream);

/* ----------------------------------------------------- devoxelization ----
 * spherical_trilinear_devoxelize_forward
 * (interpolate/spherical_trilinear_devox.cpp:19-56, .cu:23-136): coords
 * [b,3,n], features [b,c,r^3], g_inds [b,n] -> outs [b,c,n], inds [b,8,n],
 * wgts [b,8,n].  is_training is ignored, as in the reference. */
pcr_status pcr_spherical_trilinear_devoxelize_forward(int r, int is_training, const float *coords,
                                                      const float *features, const int *g_inds,
                                                      int b, int c, int n, float *outs, int *inds,
                                                      float *wgts, void *stream);

/* trilinear_devoxelize_forward (interpolate/trilinear_devox.cpp:18-56,
 * .cu:22-106): cube variant on continuous voxel coords [b,3,n]. */
pcr_status pcr_trilinear_devoxelize_forward(int r, int is_training, const float *coords,
                                            const float *features, int b, int c, int n,
                                            float *outs, int *inds, float *wgts, void *stream);

/* spherical_trilinear_devoxelize_backward (spherical_trilinear_devox.cpp:68-92,
 * .cu:150-194; skip_neg=1: points with inds[0]==-1 are skipped) and
 * trilinear_devoxelize_backward (trilinear_devox.cpp:58-91, .cu:120-163;
 * skip_neg=0): grad_y [b,c,n] -> grad_x [b,c,r^3]. */
pcr_status pcr_devoxelize_backward(const float *grad_y, const int *inds, const float *wgts, int b,
                                   int c, int n, int r, int skip_neg, float *grad_x,
                                   void *stream);
/* The same with a workspace of pcr_devoxelize_backward_workspace_size(b, n)
 * bytes: spherical grads of clouds of <= 4096 points first sort each cloud's
 * points by corner set once (instead of every channel-group workgroup
 * sorting every 64 points), so the backward only sums runs.  Same results
 * up to the fp32 summation order of the atomics (as the reference's). */
size_t pcr_devoxelize_backward_workspace_size(int b, int n);
/* Workspace for pcr_devoxelize_backward_ws that also covers the cube
 * gather path (spherical=0, r <= 32): each cloud's 8n (point, corner) pairs
 * are counting-sorted by voxel once and every voxel sums its own segment, so
 * grad_x is written once with no atomics (trilinear_devox.cu:120-163 does one
 * global float atomic per pair and channel).  Same results up to the fp32
 * summation order within a voxel.  With only
 * pcr_devoxelize_backward_workspace_size(b, n) bytes the cube grads take
 * the LDS-atomic kernel. */
size_t pcr_devoxelize_backward_workspace_size_r(int b, int n, int r, int spherical);
pcr_status pcr_devoxelize_backward_ws(const float *grad_y, const int *inds, const float *wgts,
                                      int b, int c, int n, int r, int skip_neg, float *grad_x,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* PVConv dgcnn centre term (modules/pvconv.py:68-89): related[b,c,i] =
 * features[b,c,i] - avg_grid[b,c,ind[b,i]], 0 where ind == -1. */
pcr_status pcr_dgcnn_center_gather(const float *features, const float *avg_grid, const int *ind,
                                   int b, int c, int n, int r3, float *related, void *stream);

/* ---------------------------------------------------- fused extractor ----
 * The spherical voxel stage of the sph-dg extractor forward, fused:
 * normalise coords -> spherical voxel index -> voxel mean grid (written
 * once, coalesced) -> spherical devoxelisation of that grid -> per-cloud
 * max-pooled descriptor.  Outputs (any may be NULL except grid):
 * norm_coords [b,3,n], ind [b,n], cnt [b,r^3], grid [b,c,r^3],
 * devox [b,c,n], dinds [b,8,n], dwgts [b,8,n], desc [b,c] (max over points of
 * devox).  Equivalent to pcr_spherical_normalize + ..._avg_voxelize_forward +
 * ..._trilinear_devoxelize_forward on the produced grid. */
size_t pcr_extractor_workspace_size(int b, int n, int c, int r);
pcr_status pcr_extractor_voxel_stage(const float *xyz, const float *features, int b, int c,
                                     int n, int r, float *norm_coords, int *ind, int *cnt,
                                     float *grid, float *devox, int *dinds, float *dwgts,
                                     float *desc, void *workspace, size_t workspace_bytes,
                                     void *stream);

/* The launches of pcr_extractor_voxel_stage, separately, so a caller can run
 * the grid and devox launches on two streams (they are independent once prep
 * is done) and time the grid kernel with events on its stream:
 *   prep  = normalise + voxel index + occupancy/segments + devox corners
 *   grid  = voxel means -> dense grid [b,c,r^3] + cnt, written once
 *   devox = voxel means -> spherical devoxelisation [b,c,n] + descriptor
 * The workspace carries the prep results to the other two. */
pcr_status pcr_extractor_voxel_prep(const float *xyz, int b, int n, int r, float *norm_coords,
                                    int *ind, int *dinds, float *dwgts, void *workspace,
                                    size_t workspace_bytes, void *stream);
pcr_status pcr_extractor_voxel_grid(const float *features, int b, int c, int n, int r, int *cnt,
                                    float *grid, void *workspace, size_t workspace_bytes,
                                    void *stream);
pcr_status pcr_extractor_voxel_devox(const float *features, int b, int c, int n, int r,
                                     float *devox, const int *dinds, const float *dwgts,
                                     float *desc, void *workspace, size_t workspace_bytes,
                                     void *stream);
/* devox + descriptor from the dense grid the grid launch wrote (on the same
 * stream, after it): every spherical corner lies in a fixed set of 80 voxels
 * (spherical_trilinear_devox.cu:67-105), whose values are staged in LDS per
 * channel; corners from prep's dinds / dwgts.  n <= 4096.  Same outputs as
 * pcr_extractor_voxel_devox (which re-forms the voxel means from the
 * features instead of reading the grid). */
pcr_status pcr_extractor_grid_devox(const float *grid, const int *dinds, const float *dwgts,
                                    int b, int c, int n, int r, float *devox, float *desc,
                                    void *stream);
/* grid + devox + descriptor in one launch after prep (the devox tail gathers
 * the voxel means the workgroup already holds in LDS, through prep's corner
 * -> segment map): what pcr_extractor_voxel_stage launches after prep. */
pcr_status pcr_extractor_voxel_grid_devox(const float *features, int b, int c, int n, int r,
                                          int *cnt, float *grid, float *devox, const int *dinds,
                                          const float *dwgts, float *desc, void *workspace,
                                          size_t workspace_bytes, void *stream);

/* The voxel stage split so the dense grid streams beside the KNN selection
 * (what vox_grid_kernel<3> does in one launch, in two):
 *   means_devox: the voxel means of every occupied segment (fixed ascending
 *     point order) into the workspace, spherical_trilinear_devoxelize of them
 *     (spherical_trilinear_devox.cu:23-136) and the per-cloud descriptor;
 *   stream: the dense [B, C, r^3] grid + cnt [B, r^3] of
 *     spherical_avg_voxelize_forward (spherical_vox.cu:19-125) from those
 *     means, written once, zeros included.
 * Both read the workspace pcr_extractor_voxel_prep filled; its size is
 * pcr_extractor_workspace_size(b, n, c, r).  r^3 <= 65536, r^3 % 4 == 0. */
pcr_status pcr_extractor_voxel_means_devox(const float *features, int b, int c, int n, int r,
                                           float *devox, const int *dinds, const float *dwgts,
                                           float *desc, void *workspace, size_t workspace_bytes,
                                           void *stream);
pcr_status pcr_extractor_voxel_stream(int b, int c, int n, int r, int *cnt, float *grid,
                                      void *workspace, size_t workspace_bytes, void *stream);
/* The same back half with the spherical devox moved into the grid stream:
 * pcr_extractor_voxel_means writes only the compact means rows (no devox,
 * no descriptor), then pcr_extractor_voxel_stream_devox writes grid + cnt,
 * devox [b,c,n] (from dwgts and prep's corner segments) and desc [b,c]
 * (NULL: none) -- the outputs of means_devox + stream, bit for bit, with the
 * cloud's corner data read once per grid workgroup instead of once per
 * channel pair.  pcr_extractor_stream_devox_ok(n, c, r) is nonzero where it
 * applies (n <= 1024, r^3 <= 32768). */
int pcr_extractor_stream_devox_ok(int n, int c, int r);
pcr_status pcr_extractor_voxel_means(const float *features, int b, int c, int n, int r,
                                     void *workspace, size_t workspace_bytes, void *stream);
pcr_status pcr_extractor_voxel_stream_devox(int b, int c, int n, int r, int *cnt, float *grid,
                                            float *devox, const float *dwgts, float *desc,
                                            void *workspace, size_t workspace_bytes,
                                            void *stream);

/* ------------------------------------------- mutual-NN matching (8f f1) ----
 * datasets/deepgmr_mn40.py:232-244 find_correspondence_one_pair, for p pairs:
 * f1 [p, n1, c], f2 [p, n2, c] (rows = points, channels contiguous, as the
 * numpy [n, c] arrays).  diff = |f1_i|^2 + |f2_j|^2 - 2 f1_i . f2_j;
 * corr12 [p, n1] = argmin_j, corr21 [p, n2] = argmin_i (first index on ties,
 * NaN first as np.argmin); idx1 / idx2 [p, n1] = the mutual pairs
 * (corr21[corr12[i]] == i) in ascending i, -1 after count[p] of them.
 * Channel sums are k-ordered fmaf chains (fp32 MFMA), include/pcr_math.h.
 *
 * Workspace keys (guaranteed): once the call's work on `stream` is done, the
 * workspace holds the winning 64-bit key of every row and column, as
 * include/pcr_math.h defines pcr_match_key: the mapped diff bits in the high
 * word, the index in the low word.  rowbest [p][n1] at byte offset 0, colbest [p][n2] at byte
 * offset p * n1 * 8 rounded up to a multiple of 256.  corr12 / corr21 are
 * their low words.  Bytes of the workspace past colbest are never touched,
 * and whatever the workspace held before the call does not matter.
 *
 * Alignment: f1 / f2 need only the alignment of a float.  With c % 4 == 0
 * the row-major kernel reads the features as 16-byte vectors at addresses
 * that are multiples of 4 bytes, not necessarily of 16: gfx950 global loads
 * are dword-granular in the unaligned access mode ROCm configures, so a base
 * pointer off a 16-byte boundary (a torch view starting at element 1) is
 * legal and gives the same results, at more cache lines per load.  The
 * workspace must be 8-byte aligned. */
size_t pcr_mutual_nn_workspace_size(int p, int n1, int n2);
pcr_status pcr_mutual_nn_match(const float *f1, const float *f2, int p, int n1, int n2, int c,
                               int *corr12, int *corr21, int *idx1, int *idx2, int *count,
                               void *workspace, size_t workspace_bytes, void *stream);
/* The same on channel-major per-point features -- f1 [p, c, n1], f2
 * [p, c, n2], the [B, C, N] layout the extractor / PVConv produce -- so the
 * registration step matches the devoxelised features in place (same sums,
 * same results as pcr_mutual_nn_match on the transposes). */
pcr_status pcr_mutual_nn_match_cm(const float *f1, const float *f2, int p, int n1, int n2, int c,
                                  int *corr12, int *corr21, int *idx1, int *idx2, int *count,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* The same on ragged pairs: counts1 / counts2 [p] int32 on
 * the device; pair q's valid rows are the first v1 = counts1[q] of f1 and the
 * first v2 = counts2[q] of f2, both clamped to [0, n]; a NULL pointer: all n
 * of that side.  The strides stay n1 / n2 (channel_major != 0: the layout of
 * pcr_mutual_nn_match_cm).  Pair q's result is that of the dense call on
 * f1[q, :v1, :], f2[q, :v2, :] -- diff bits, tie order, NaN first -- and a
 * fixed fill past the counts: corr12[q, i] = -1 for i >= v1 and everywhere
 * when v2 = 0 (corr21 with the roles swapped); idx1 / idx2 / count: the
 * mutual pairs among the valid rows in ascending i, then -1.  Whatever the
 * rows past the counts hold (zeros, NaN, Inf, copies of valid rows) changes
 * nothing.  Workspace: pcr_mutual_nn_workspace_size bytes, the layout above;
 * the keys of rows < v1 and columns < v2 are the winning keys, every other
 * entry is all-ones.  Every output pointer must be non-NULL. */
pcr_status pcr_mutual_nn_match_ragged(const float *f1, const float *f2, int p, int n1, int n2,
                                      int c, const int *counts1, const int *counts2,
                                      int channel_major, int *corr12, int *corr21, int *idx1,
                                      int *idx2, int *count, void *workspace,
                                      size_t workspace_bytes, void *stream);

/* ------------------------- rigid transform from the correspondences -------
 * The step after the matching (datasets/deepgmr_mn40.py:165-231
 * register_one_pair, there Open3D RANSAC on the CPU), for p pairs: a seeded,
 * deterministic RANSAC and a least-squares refit (the scalar
 * math is include/pcr_rigid.h).
 *   xyz1 [p,3,n1], xyz2 [p,3,n2]; idx1 / idx2 [p,n1] and count [p] as the
 *   matching emits them: slot s < count[q] pairs xyz1[q,:,idx1[q,s]] with
 *   xyz2[q,:,idx2[q,s]].
 *   Hypothesis h of pair q takes the three distinct slots its integer sampler
 *   draws from (seed, q, h, count[q]); it is rejected (score -1) by the edge-length check
 *   (edge_ratio in [0, 1), 0: only zero-length edges reject), else solved in
 *   fp64 (b ~ R a + t, det R = +1) and scored by the number of slots whose
 *   fp32 residual is <= inlier_dist.  The best score wins, ties to the lowest
 *   h; refine_iters times: mask under the current transform, least squares
 *   over the mask (stops when fewer than 3 slots remain).
 *   transform [p,4,4] fp64 row-major; inliers [p,n1] 0/1 per slot and
 *   num_inliers [p] under the final transform; best_hyp [p] (-1: none);
 *   scores [p,hyps] (NULL: not wanted); status [p]: 0 ok, 1 count < 3,
 *   2 every hypothesis rejected (1 / 2: identity, no inliers).
 * Bit-identical from run to run.  Runs on `stream`; the workspace is the
 * caller's. */
size_t pcr_rigid_ransac_workspace_size(int p, int n1, int hyps);
pcr_status pcr_rigid_ransac(const float *xyz1, const float *xyz2, int p, int n1, int n2,
                            const int *idx1, const int *idx2, const int *count,
                            int hyps, float inlier_dist, float edge_ratio, int refine_iters,
                            unsigned seed, double *transform, int *inliers, int *num_inliers,
                            int *best_hyp, int *scores, int *status,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------ point-to-point ICP ------------------
 * utils/open3d_func.py:63-72 (register_one_pair with func='icp': Open3D
 * registration_icp, point to point), for p pairs, as a solver of its own or as
 * the refinement of pcr_rigid_ransac's transform (the scalar
 * math is include/pcr_rigid.h and pcr_sumsq3f of include/pcr_math.h).
 *   xyz1 [p,3,n1] source, xyz2 [p,3,n2] target; init [p,4,4] fp64 row-major
 *   (the upper 3 x 4 is used as it is; NULL: the identity).
 *   Evaluate(T): T rounded to fp32; every source point moved by the fp32 fmaf
 *   chain of the residual; its nearest target by the fp32 squared distance
 *   (lowest index on ties, a non-finite distance never wins) is its
 *   correspondence when that distance is <= max_dist * max_dist (an fp32
 *   product), else -1.  M = their number, fitness = M / n1, rmse =
 *   sqrt(sum of the squared distances / M) in fp64 (0 when M = 0).
 *   Iterate from Evaluate(init), at most max_iters times: stop with status 1
 *   when M < 3; T = the fp64 least-squares R, t of the original source points
 *   onto their correspondences; Evaluate(T); stop with status 0 when
 *   |fitness change| < rel_fitness and |rmse change| < rel_rmse.  Status 2:
 *   the iteration limit (max_iters = 0: a pure evaluation of init).
 *   transform [p,4,4] fp64 (bottom row 0 0 0 1); corr [p,n1], num_corr [p],
 *   fitness [p], rmse [p]: Evaluate at the reported transform; iterations [p]:
 *   solves made; status [p].  0 <= max_iters <= 100000; max_dist > 0; the
 *   tolerances >= 0.  A bad pair (far apart, NaN) never fails the call.
 * Bit-identical from run to run.  Runs on `stream`; needs no workspace. */
pcr_status pcr_icp_point_to_point(const float *xyz1, const float *xyz2, int p, int n1, int n2,
                                  const double *init, float max_dist, int max_iters,
                                  double rel_fitness, double rel_rmse, double *transform,
                                  int *corr, int *num_corr, double *fitness, double *rmse,
                                  int *iterations, int *status, void *stream);
/* The same on ragged pairs (counts1 / counts2 as for
 * pcr_mutual_nn_match_ragged): only the source points i < v1
 * and the targets j < v2 exist, fitness = M / v1, corr[q, i] = -1 for
 * i >= v1.  v1 = 0: the transform is the init, M 0, fitness 0, rmse 0,
 * iterations 0, status 1.  v2 = 0: no target is within reach (the dense rule:
 * M = 0, status 1, or 2 with max_iters = 0).  Otherwise every output of pair q
 * is, bit for bit, that of the dense call on the pair trimmed to its counts.
 * The points past the counts may hold anything. */
pcr_status pcr_icp_point_to_point_ragged(const float *xyz1, const float *xyz2, int p, int n1,
                                         int n2, const int *counts1, const int *counts2,
                                         const double *init, float max_dist, int max_iters,
                                         double rel_fitness, double rel_rmse, double *transform,
                                         int *corr, int *num_corr, double *fitness, double *rmse,
                                         int *iterations, int *status, void *stream);

/* ------------------------------------ point-to-plane ICP ------------------
 * Open3D's registration_icp with TransformationEstimationPointToPlane, for p
 * pairs, dense or ragged through one entry point (the scalar
 * math is include/pcr_icp_plane.h on the Cholesky, delta and compose of
 * include/pcr_fgr.h, include/pcr_rigid.h and pcr_sumsq3f).
 *   normals2 [p,3,n2] fp32: the target's normals.  counts1 / counts2 [p]
 *   int32 on the device, or NULL for all n1 / n2 points, clamped to [0, n] as
 *   for pcr_icp_point_to_point_ragged: v1 / v2 below.  Every other argument
 *   is as there.
 *   Evaluate(T) is the point-to-point one, word for word: T rounded to fp32,
 *   the fp32 fmaf chain, the nearest target by the fp32 squared distance
 *   (lowest index on ties, a non-finite distance never wins) within
 *   max_dist * max_dist, M, fitness = M / v1 and the Euclidean rmse.  The
 *   normals play no part in it.
 *   Step: every correspondence (i, j) gives, widened to fp64, the fp32 moved
 *   point m Evaluate searched with, the target b and the normal n =
 *   normals2[:, j]; r = ((m0-b0) n0 + (m1-b1) n1) + (m2-b2) n2, J = (m x n, n).
 *   The 27 sums (the upper triangle of J J^T in row order, then J r; each
 *   thread its points in ascending order, then the workgroup in a fixed order)
 *   make A and g; A x = g by pcr_fgr_cholesky_solve, x = -x, and
 *   T <- Delta(x) T in fp64 with pcr_fgr_delta and pcr_fgr_compose: Open3D's
 *   TransformVector6dToMatrix4d update.
 *   Iterate from Evaluate(init), at most max_iters times: stop with status 1
 *   when M < 6; take a step, and stop with status 3 when the Cholesky meets a
 *   pivot that is not finite and positive (T stays the last evaluated one);
 *   Evaluate(T); stop with status 0 when |fitness change| < rel_fitness and
 *   |rmse change| < rel_rmse.  Status 2: the iteration limit (max_iters = 0:
 *   a pure evaluation of init).  The M < 6 rule and status 3 are this
 *   library's: Open3D applies the identity update in both cases and goes on.
 *   The outputs always describe Evaluate at the reported transform;
 *   corr[q, i] = -1 for i >= v1.  v1 = 0: the transform is the init, M 0,
 *   fitness 0, rmse 0, iterations 0, status 1.  v2 = 0: M = 0, status 1 (2
 *   with max_iters = 0).  Otherwise every output of pair q is, bit for bit,
 *   that of the call on the pair trimmed to its counts; the points and the
 *   normals past the counts may hold anything.  A bad pair (far apart, NaN, a
 *   planar target) never fails the call.
 * Bit-identical from run to run.  Runs on `stream`; needs no workspace. */
pcr_status pcr_icp_point_to_plane(const float *xyz1, const float *xyz2, const float *normals2,
                                  int p, int n1, int n2, const int *counts1, const int *counts2,
                                  const double *init, float max_dist, int max_iters,
                                  double rel_fitness, double rel_rmse, double *transform,
                                  int *corr, int *num_corr, double *fitness, double *rmse,
                                  int *iterations, int *status, void *stream);

/* ------------------------------- Fast Global Registration -----------------
 * utils/open3d_func.py:34-75 (register_one_pair with func='fgr': Open3D
 * registration_fast_based_on_feature_matching), for p pairs, from the
 * matching's correspondences (the scalar math is
 * include/pcr_fgr.h and the sampler and edge check of include/pcr_rigid.h).
 *   xyz1 [p,3,n1], xyz2 [p,3,n2]; idx1 / idx2 [p,n1] and count [p] as for
 *   pcr_rigid_ransac: M = count[q] clamped to [0, n1] slots.
 *   Tuple test: max_tuples = 0: the list L is the slots 0 .. M-1.  Else
 *   H = trials_per_corr * M trials (none when M < 3); trial h takes the three
 *   slots pcr_rigid_triple draws from (seed, q, h, M) and is accepted iff
 *   pcr_rigid_edge_ok holds at tuple_scale; the first max_tuples accepted trials
 *   in ascending h count, L is their slots in that order (three per trial,
 *   duplicates kept); num_trials = the last counted h + 1 when the cap was
 *   reached, else H (0 with max_tuples = 0).  K = |L|.
 *   K < 10: status 1.  Else the clouds' fp64 centroids m1 / m2 (over all their
 *   points, in the summation order of pcr_fgr_sum) and s = the largest
 *   distance of a point to its cloud's centroid; s zero or not finite:
 *   status 2.  d = s, mu = 1 (absolute_scale: d = 1, mu = s); L's points in
 *   units of d about the centroids.
 *   Loop, `iterations` times from T = identity: the moved target points, the
 *   weights (mu / (|r|^2 + mu))^2, the 6 x 6 normal equations of
 *   J = [[q]x, -I], their fp64 Cholesky solve (a pivot not finite and
 *   positive: status 3, T as reached so far), T <- Delta T with
 *   Delta = [Rz Ry Rx, translation]; then, with decrease_mu, every fourth
 *   iteration (it % 4 == 0) while mu > max_corr_dist (compared in normalised
 *   units, unscaled, as Open3D does): mu /= division_factor.
 *   transform [p,4,4] fp64: the inverse of T in original units, xyz2 ~ R xyz1
 *   + t, bottom row 0 0 0 1 (status 1 / 2: the identity, mu 0); slots
 *   [p, kcap], kcap = 3 * max_tuples (max_tuples = 0: n1): L, then -1;
 *   num_corr [p] = K; num_trials [p]; mu [p] fp64: the final value;
 *   status [p].  0 <= iterations <= 100000; division_factor > 1;
 *   0 <= tuple_scale < 1; max_tuples >= 0; trials_per_corr >= 0 and
 *   trials_per_corr * n1 <= 2^31 - 1; max_corr_dist >= 0.  A bad pair (NaN,
 *   degenerate) never fails the call and touches no other pair.
 * Bit-identical from run to run.  Runs on `stream`; the workspace
 * (pcr_fgr_workspace_size bytes: L's point pairs) is the caller's. */
size_t pcr_fgr_workspace_size(int p, int n1, int max_tuples);
pcr_status pcr_fgr(const float *xyz1, const float *xyz2, int p, int n1, int n2, const int *idx1,
                   const int *idx2, const int *count, double max_corr_dist, int iterations,
                   double division_factor, int decrease_mu, float tuple_scale, int max_tuples,
                   int trials_per_corr, int absolute_scale, unsigned seed, double *transform,
                   int *slots, int *num_corr, int *num_trials, double *mu, int *status,
                   void *workspace, size_t workspace_bytes, void *stream);
/* The same on ragged pairs (counts1 / counts2 as for
 * pcr_mutual_nn_match_ragged): the centroids, their divisors
 * and the scale s run over the valid points only, so pair q's result is, bit
 * for bit, that of the dense call on the pair trimmed to its counts.  The
 * rest is unchanged: malformed indices are clamped into the strides n1 / n2,
 * as before.  A pair with K >= 10 and an empty cloud has no scale: status 2. */
pcr_status pcr_fgr_ragged(const float *xyz1, const float *xyz2, int p, int n1, int n2,
                          const int *counts1, const int *counts2, const int *idx1,
                          const int *idx2, const int *count, double max_corr_dist, int iterations,
                          double division_factor, int decrease_mu, float tuple_scale,
                          int max_tuples, int trials_per_corr, int absolute_scale, unsigned seed,
                          double *transform, int *slots, int *num_corr, int *num_trials,
                          double *mu, int *status, void *workspace, size_t workspace_bytes,
                          void *stream);

/* ------------------------------- TEASER-style robust registration ---------
 * datasets/modelnet40_registration.py:274-327 (register_one_pair with
 * func='teaserpp': TEASER++ with GNC-TLS at noise_bound 0.02, cbar2 1), for p
 * pairs, from the matching's correspondences, with a bounded greedy clique
 * search in place of TEASER++'s exact one (the scalar math is
 * include/pcr_teaser.h and the edge length and rotation solve of
 * include/pcr_rigid.h).
 *   xyz1 [p,3,n1], xyz2 [p,3,n2]; idx1 / idx2 [p,n1] and count [p] as for
 *   pcr_fgr: M = count[q] clamped to [0, n1] slots, slot s pairs a_s with b_s.
 *   beta = 2 noise_bound sqrt(cbar2), rho = noise_bound sqrt(cbar2) (fp64, host).
 *   Graph: slots i != j are joined iff | |a_j - a_i| - |b_j - b_i| | <= beta
 *   (pcr_teaser_edge: fp64 lengths of the fp32 points; a NaN never joins).
 *   Clique: the slots ranked by degree, descending, lowest slot first; seed r <
 *   S is the slot of rank r, S = M (seeds = 0) or min(seeds, M).  From a seed v:
 *   C = {v}, P = N(v); while P is not empty its best-ranked member u joins C and
 *   P <- P & N(u).  The largest C wins, the best-ranked seed on ties.
 *   inlier_selection = 0: C is all M slots.  K = |C|; K < 3: status 1.
 *   Rotation: GNC-TLS over the K (K - 1) / 2 TIMs u = a_j - a_i, v = b_j - b_i
 *   (i < j in C), nu^2 = beta^2, weights 1 at first; at most max_iters times:
 *   H = sum w u v^T, R from H (pcr_teaser_rotation), r^2 = |v - R u|^2; in the
 *   first iteration mu from max r^2 (pcr_teaser_mu0; max r^2 not finite: status
 *   2; mu <= 0 or not finite: done); cost = sum w r^2, the new w from r^2 and mu
 *   (pcr_teaser_weight), mu *= gnc_factor; done when |cost - previous cost| <
 *   cost_threshold.
 *   Status 3: the iteration limit (R is reported).
 *   Translation, per axis: X_k = b_k - (R a_k); over the midpoints of the 2 K
 *   endpoints X_k -+ rho sorted by value, then number (pcr_teaser_vote_at): the
 *   mean of {k : |X_k - m| <= rho} with the lowest sum_k min((X_k - mean)^2,
 *   rho^2), the earliest midpoint on ties.  Slot k of C is an inlier iff
 *   |X_k - t| <= rho on all three axes.
 *   transform [p,4,4] fp64, xyz2 ~ R xyz1 + t, bottom row 0 0 0 1 (status 1 / 2:
 *   the identity, no inliers); clique [p,n1]: C as ascending slots, then -1;
 *   clique_size [p] = K; inliers [p,n1]: 0 / 1 per slot; num_inliers [p];
 *   iterations [p]: rotation solves made (0 with status 1); status [p].
 *   n1 <= 4096; noise_bound, cbar2 > 0; gnc_factor > 1; 1 <= max_iters <= 1000;
 *   cost_threshold >= 0; seeds >= 0.  A bad pair (NaN, M < 3, coincident
 *   points) never fails the call and touches no other pair.
 * Bit-identical from run to run and alone or inside a batch.  Runs on
 * `stream`; the workspace (pcr_teaser_workspace_size bytes: per pair the bit
 * rows, n1 * ceil(n1 / 64) * 8 bytes, and two ints per slot; the total rounded
 * up to 256) is the caller's. */
size_t pcr_teaser_workspace_size(int p, int n1);
pcr_status pcr_teaser(const float *xyz1, const float *xyz2, int p, int n1, int n2, const int *idx1,
                      const int *idx2, const int *count, double noise_bound, double cbar2,
                      double gnc_factor, int max_iters, double cost_threshold, int seeds,
                      int inlier_selection, double *transform, int *clique, int *clique_size,
                      int *inliers, int *num_inliers, int *iterations, int *status,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------- grid subsampling --------------------------
 * cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp
 * (utils/grid_subsampleing.py grid_sub_sampling: KPConv's voxel-grid
 * barycentres), for b ragged clouds (the scalar math and the
 * deviations from the reference are include/pcr_gridsub.h).
 *   xyz [b,3,n], features [b,c,n] (NULL with c = 0); counts_in [b]: cloud q's
 *   valid points are its first counts_in[q] (NULL: all n).  cell: the cell size.
 *   Per cloud, in fp32: origin_d = floorf(min_d * (1.0f / cell)) * cell over
 *   the valid points, N_d = max(0, floorf((max_d - origin_d) / cell)) + 1, a
 *   point's index i_d = max(0, floorf((p_d - origin_d) / cell)) and its key
 *   ix + NX * (iy + NY * iz) (64 bit).  Every distinct key is a cell; its sums
 *   start at 0.0f and take the cell's points in ascending point index.
 *   out_xyz = sum * (float)(1.0 / (double)count), out_features = sum /
 *   (float)count.  Cells are output in ascending key.
 *   out_xyz [b,3,n], out_features [b,c,n] (NULL with c = 0): slot s < out_count
 *   is cell s, later slots hold 0; out_count [b]; cell_of [b,n]: the output
 *   slot of each input point, -1 past the valid count; cell_count [b,n]: points
 *   per slot, 0 past out_count; origin [b,3]; dims [b,3] = N_d (saturated at
 *   2^30 + 1); status [b]: 0 ok, 1 valid count outside [1, n], 2 a non-finite
 *   coordinate among the valid points, 3 some N_d > 2^20 or an origin that is
 *   not finite.  With a status other than 0: out_count 0, every slot 0,
 *   cell_of -1 (origin and dims 0 with status 1 / 2).  Every output element is
 *   written.  b, n, c >= 0 (n >= 1 when b > 0), b * n < 2^31; cell finite and
 *   > 0.  A bad cloud never fails the call and touches no other cloud.
 * Bit-identical from run to run (no float atomics: a stable sort orders every
 * cell's sum).  Runs on `stream`, no host sync; the workspace
 * (pcr_grid_subsample_workspace_size bytes: 40 + 4 c bytes per point, 1 KB per
 * 1024 points and 2 KB per cloud) is the caller's. */
size_t pcr_grid_subsample_workspace_size(int b, int n, int c);
pcr_status pcr_grid_subsample(const float *xyz, const float *features, const int *counts_in,
                              int b, int n, int c, float cell, float *out_xyz,
                              float *out_features, int *out_count, int *cell_of, int *cell_count,
                              float *origin, int *dims, int *status, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ------------------------------- FPFH descriptors --------------------------
 * Open3D's compute_fpfh_feature (ComputeFPFHFeature with
 * KDTreeSearchParamHybrid(radius, max_nn)), the training-free descriptor its
 * registration functions (utils/open3d_func.py:43-59) are normally paired
 * with, for b clouds (the scalar math is include/pcr_fpfh.h,
 * an fp32 restatement whose operation order is the contract).
 *   xyz [b,3,n], normals [b,3,n]; nbr_idx [b,k,n] and nbr_dist [b,k,n] exactly
 *   as pcr_knn_forward writes them for a cloud against itself (squared L2,
 *   ascending).  The op does not search.  Of the slots s < min(k, n), in
 *   ascending s, slot (j, d) is in N(i) when 0 <= j < n, j != i and 0 < d <=
 *   radius * radius (fp32; a NaN d fails); any other j is never an address.
 *   Every pair (i, j in N(i)) counts in three of 33 bins (pcr_fpfh_pair,
 *   pcr_fpfh_bins); spfh[i][c] = (float)count_c * (100.0f / (float)m) with m =
 *   |N(i)|, 0 when m = 0; acc_c = the sum over N(i) in ascending slot of
 *   spfh[j][c] / d from 0.0f; per group of 11 channels S = the sum of its acc
 *   in ascending channel from 0.0f; fpfh[i][c] = acc_c * (100.0f / S) +
 *   spfh[i][c] (acc_c + spfh[i][c] when S = 0).
 *   fpfh [b,33,n] (the layout pcr_mutual_nn_match_cm takes); spfh [b,33,n] and
 *   nbr_count [b,n] = m may be NULL.  Every output element is written.
 *   n >= 1, 1 <= k <= 128, radius finite and > 0, b * k * n < 2^31; b = 0
 *   returns PCR_OK.  A bad point (NaN coordinate or normal) never fails the
 *   call and touches only itself and the points that list it; no cloud touches
 *   another.
 * Bit-identical from run to run (integer bin counts, serial sums, no float
 * atomics).  Runs on `stream`; the workspace (pcr_fpfh_workspace_size bytes:
 * 164 bytes per point, each part rounded up to 256) is the caller's. */
size_t pcr_fpfh_workspace_size(int b, int n);
pcr_status pcr_fpfh(const float *xyz, const float *normals, const int *nbr_idx,
                    const float *nbr_dist, int b, int n, int k, float radius, float *fpfh,
                    float *spfh, int *nbr_count, void *workspace, size_t workspace_bytes,
                    void *stream);

/* ------------------------- hybrid (radius + max_nn) neighbour search -------
 * Open3D's KDTreeSearchParamHybrid(radius, max_nn) of b ragged clouds against
 * themselves: the search pcr_fpfh's neighbour sets are defined on (DESIGN.md
 * 4.8g; the scalar math is include/pcr_hybrid.h).
 *   xyz [b,3,n]; counts [b]: cloud q's valid points are its first counts[q]
 *   (clamped to [0, n]; NULL: all n).  d(i, j) = fmaf(tz, tz, fmaf(ty, ty, tx *
 *   tx)) with t = p_i - p_j in fp32, pcr_knn_forward's distance bit for bit; j
 *   is within the radius of i when d <= radius * radius (fp32; a NaN or
 *   infinite d fails).  The row of a valid query i lists the valid j within
 *   its radius (i itself included), ascending by (bits of d, j) -- ties go to
 *   the lower index -- cut to the first k (max_nn).
 *   nbr_dist [b,k,n] and nbr_idx [b,k,n], slot-major as pcr_fpfh reads them;
 *   unfilled slots hold (+inf, -1).  nbr_count [b,n]: the filled slots.
 *   within [b,n] (may be NULL): the points within the radius before the cut.
 *   A query at or past counts[q] has no filled slot and both counts 0, and so
 *   has a point with a non-finite coordinate, which is in no row either.
 *   Every output element is written.  n >= 1, 1 <= k <= 128, radius and
 *   radius * radius finite and > 0, b * k * n < 2^31; b = 0 returns PCR_OK.
 * The result is that rule for every input: the cell grid the kernels use
 * (side >= radius * (1 + 2^-8), at most 32 cells an axis, one cell where its
 * parameters cannot be formed) never changes it.  Bit-identical from run to
 * run (selection on the 64-bit key; integer atomics only).  Runs on `stream`,
 * no host sync; the workspace (pcr_hybrid_search_workspace_size bytes, a
 * function of b and n alone: 20 bytes per point, 8 per cell of a grid of g^3
 * cells, g the smallest with 2 g^3 >= n and at most 32, 2.1 KB per cloud) is
 * the caller's. */
size_t pcr_hybrid_search_workspace_size(int b, int n);
pcr_status pcr_hybrid_search(const float *xyz, const int *counts, int b, int n, int k,
                             float radius, float *nbr_dist, int *nbr_idx, int *nbr_count,
                             int *within, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------ LRF change_coords (8f f2) ----------
 * models/pvcnn_classify.py:153-184 (rot_invariant_preprocess ==
 * 'change_coords'), one cloud per workgroup, no host round trip.
 * Per cloud: nc = coords - mean (the fp64 mean reduction order is given in
 * oracle/pcr_oracle.c orc_lrf); base_x = the point of largest norm; base_y =
 * the next point in descending-norm rank with norm >= 1e-5 and
 * |<base_x, p/|p|>| < 0.9; Gram-Schmidt, base_z = x cross y; new_coords =
 * basis . nc.  Rank ties go to the lower index; a NaN norm ranks first (as in
 * torch.argsort, descending), so a cloud with a NaN or infinite coordinate
 * has status 1.
 *   coords [b,3,n] -> new_coords [b,3,n], basis [b,3,3] (rows x, y, z),
 *   picks [b,2] (base_x, base_y point indices), status [b]: 0 ok, 1 base_x
 *   norm <= 1e-5, 2 no base_y, 3 degenerate Gram-Schmidt.  These are the
 *   reference's asserts; the host shim raises on them. */
pcr_status pcr_lrf_change_coords(const float *coords, int b, int n, float *new_coords,
                                 float *basis, int *picks, int *status, void *stream);

/* --------------------------------- PointNet++ ops (8f f4) ----------------
 * sampling/sampling.cpp:6-58 gather_features_forward / _backward and
 * furthest_point_sampling_forward; interpolate/neighbor_interpolate.cpp:
 * 6-65 three_nearest_neighbors_interpolate_forward / _backward. */
/* features [b,c,n], indices [b,m] -> out [b,c,m] (indices outside [0,n)
 * read 0; the reference reads out of bounds there) */
pcr_status pcr_gather_features_forward(const float *features, const int *indices, int b, int c,
                                       int n, int m, float *out, void *stream);
/* grad_y [b,c,m] -> grad_x [b,c,n] (zeroed here, then scatter-added) */
pcr_status pcr_gather_features_backward(const float *grad_y, const int *indices, int b, int c,
                                        int n, int m, float *grad_x, void *stream);
/* coords [b,3,n] -> indices [b,m].  Tie order as the reference's
 * 512-thread reduction (pcr_fps_key).  workspace: pcr_fps_workspace_size. */
size_t pcr_fps_workspace_size(int b, int n);
pcr_status pcr_furthest_point_sampling(const float *coords, int b, int n, int m, int *indices,
                                       void *workspace, size_t workspace_bytes, void *stream);
/* points [b,3,n], centers [b,3,m], centers_features [b,c,m] ->
 * out [b,c,n], indices [b,3,n], weights [b,3,n] */
pcr_status pcr_three_nn_interpolate_forward(const float *points, const float *centers,
                                            const float *centers_features, int b, int c, int m,
                                            int n, float *out, int *indices, float *weights,
                                            void *stream);
/* grad_y [b,c,n] -> grad_x [b,c,m] (zeroed here, then scatter-added) */
pcr_status pcr_three_nn_interpolate_backward(const float *grad_y, const int *indices,
                                             const float *weights, int b, int c, int n, int m,
                                             float *grad_x, void *stream);

/* ------------------------------------------- normal estimation (8f f3) ----
 * utils/open3d_func.py:77-83 get_normals (Open3D estimate_normals with
 * KDTreeSearchParamRadius(radius) + orient_normals_towards_camera_location()
 * + normalize_normals()), batched on the GPU: points [b,3,n] -> normals
 * [b,3,n] (unit, facing the origin; (0,0,1) with < 3 neighbours),
 * counts [b,n] = neighbours within radius incl. the point (may be NULL).
 * Arithmetic: pcr_estimate_normal of include/pcr_math.h, in fp64. */
pcr_status pcr_estimate_normals(const float *points, int b, int n, double radius, float *normals,
                                int *counts, void *stream);
/* Normals from ready neighbour lists: Open3D's estimate_normals with
 * KDTreeSearchParamHybrid(radius, max_nn), the search being pcr_hybrid_search
 * (DESIGN.md 4.8h).  xyz [b,3,n]; nbr_idx [b,k,n] slot-major as
 * pcr_hybrid_search writes it, the point itself in its own row.  The
 * neighbours of point i are its slots s = 0 .. k-1 in ascending s whose index
 * j satisfies 0 <= j < n; any other value (-1, out of range) is skipped and
 * never used as an address.  The nine cumulants {sx, sy, sz, sxx, sxy, sxz,
 * syy, syz, szz} are fp64 sums from 0.0 in that order of fp64 products of the
 * widened coordinates, uncontracted; the normal is pcr_estimate_normal of
 * include/pcr_math.h on them: (0,0,1) with fewer than 3 neighbours, facing
 * the origin, unit, rounded to float.  normals [b,3,n]; nbr_count [b,n] (may
 * be NULL): the slots counted.  Every element is written; a point with an
 * empty row -- every pad of a ragged cloud -- gets (0,0,1) and 0.  A row that
 * names a non-finite point may give any normal for that point alone.
 * n >= 1, 1 <= k <= 128, b * k * n < 2^31; b = 0 returns PCR_OK.  No
 * workspace, no host sync; bit-identical from run to run. */
pcr_status pcr_normals_from_neighbors(const float *xyz, const int *nbr_idx, int b, int n, int k,
                                      float *normals, int *nbr_count, void *stream);

/* ----------------------------------------- on-disk point rows (8f f3) ----
 * datasets/modelnet40.py:30 np.loadtxt(<sample>.txt, delimiter=',') for the
 * ModelNet40 normal-resampled files ("x,y,z,nx,ny,nz" per line): every
 * value parsed as double, then rounded to float (= loadtxt + astype float32).
 * HOST memory, host code.  pcr_txt_shape counts rows/columns; pcr_read_xyzn_txt
 * fills a row-major [rows, cols] float buffer. */
pcr_status pcr_txt_shape(const char *path, long long *rows, int *cols);
pcr_status pcr_read_xyzn_txt(const char *path, float *out, long long rows, int cols);

/* ------------------------------------------------ native step runner ----
 * `steps` consecutive extractor steps (the pipelined schedule bench.py
 * measures), enqueued from native code: every launch and cross-stream event
 * of every step is issued here, so the host enqueue rate never limits the
 * step rate.  Forked from and joined back into `origin`.
 *
 * Step s of a call reads its clouds from, and writes every output into,
 * sets[(set0 + s) % nsets] -- a fresh batch per step, as the reference's
 * loaders hand one over per iteration (datasets/deepgmr_mn40.py:71-97,
 * train.py:138-153); nsets = 1 runs every step over one set of buffers.  The
 * workspaces are per queue, not per set.  With steps <= nsets every step of
 * a call writes its own set, so after the call (all streams joined back into
 * `origin`) the outputs of every step are readable on `origin`; the next
 * call forks from `origin` after whatever the caller enqueued there, so a
 * consumer enqueued between calls never races the next call's writes.  More
 * steps than sets in one call overwrite set q with step s + nsets.
 * desc_steps: [steps][b][c] per-step descriptors, or NULL (then each set's
 * desc).
 *   schedule 0: serial, two streams -- s_nbr: Morton sort, KNN selection,
 *               local PPF with knn_ws[0]; s_vox: prep + the fused grid /
 *               devox / descriptor kernel with vox_ws[0].
 *   (schedules 1-5, single-queue-per-stage variants measured in rounds 2-4,
 *   were removed: DESIGN.md 4.)
 *   schedule 6: two independent pipelines per chain and no cross-queue event
 *               inside the run: the voxel chain (prep, means / devox /
 *               descriptor, matching, grid stream) of step s on s_vox (even
 *               s) or `origin` (odd s) with vox_ws[s % 2], the KNN chain
 *               (sort, selection, local PPF) on s_nbr (even) or s_pre (odd)
 *               with knn_ws[s % 2], so every workspace is reused only on its
 *               own queue.  The odd voxel queue starts after step 0's means
 *               (one wait per call) so the two grid streams alternate rather
 *               than coincide.  Needs nsets >= 2 (consecutive steps write
 *               distinct sets); a ring of odd size that one call wraps orders
 *               each set's rewrite behind its previous step with per-set
 *               events (made on first use).
 *   schedule 7: as 6 with three voxel queues (s_vox, origin, s_pre with
 *               vox_ws[0..2]) and one KNN queue (s_nbr, knn_ws[0]); needs
 *               nsets >= 3, per-set events when the ring size is not a
 *               multiple of 3.  Schedules 6 / 7 with match_pairs: each voxel
 *               queue matches in its own part (half / third) of match_ws.
 *
 * `runner` holds the run's cross-stream events, created once by
 * pcr_runner_create on the current device and reused by every call (NULL:
 * transient events for this call only).  With timed_steps > 0 the runner
 * also brackets the grid-stream kernel (pcr_extractor_voxel_stream) of the
 * min(steps, timed_steps) steps in the middle of each run (pipeline full; fewer after
 * pcr_runner_set_timed) with timing events on its stream;
 * pcr_runner_grid_times waits for them and returns the per-step durations
 * (ms) of the last run -- the dominant kernel's in-step duration. */
typedef struct pcr_runner pcr_runner;
pcr_status pcr_runner_create(int timed_steps, pcr_runner **out);
void pcr_runner_destroy(pcr_runner *runner);
pcr_status pcr_runner_grid_times(pcr_runner *runner, float *ms, int cap, int *count);
/* steps timed by each later run (0..timed_steps of pcr_runner_create; the
 * default is all of them) */
pcr_status pcr_runner_set_timed(pcr_runner *runner, int timed_steps);
/* the clouds and outputs of one step */
typedef struct pcr_extractor_set {
  const float *xyz, *normals, *features;  /* [b,3,n], [b,3,n], [b,c,n] */
  int *knn_idx;                           /* [b,k,n] */
  float *knn_dist;                        /* [b,k,n] or NULL */
  float *local_ppf;                       /* [b,4,k,n] */
  float *norm_coords;                     /* [b,3,n] */
  int *ind, *cnt;                         /* [b,n], [b,r^3] */
  float *grid, *devox, *desc;             /* [b,c,r^3], [b,c,n], [b,c] */
  int *dinds;                             /* [b,8,n] */
  float *dwgts;                           /* [b,8,n] */
  int *corr12, *corr21, *idx1, *idx2, *match_count; /* match_pairs > 0: [P,n] / [P] */
} pcr_extractor_set;
/* what holds for every step of a run */
typedef struct pcr_extractor_args {
  int b, n, c, k, r, relative;
  void *knn_ws[2];                        /* pcr_knn_workspace_size(b, n, n) */
  size_t knn_ws_bytes;
  void *vox_ws[3];                        /* pcr_extractor_workspace_size(b, n, c, r) */
  size_t vox_ws_bytes;
  /* registration pairs (BASELINE c4, datasets/deepgmr_mn40.py:71-97,
   * 232-244): match_pairs = P > 0 with b == 2P makes every step also match
   * the devoxelised per-point features of cloud i (source) against cloud
   * P + i (target) by pcr_mutual_nn_match_cm, on the step's voxel queue
   * after its devox, into its set's corr12 ... match_count. */
  int match_pairs;
  void *match_ws;                         /* pcr_mutual_nn_workspace_size(P, n, n);
                                             schedules 6 / 7: two / three times
                                             that + 512 B (one part per voxel
                                             queue) */
  size_t match_ws_bytes;
  /* nsets >= 1 sets; step s of the call uses set (set0 + s) % nsets */
  int nsets, set0;
  const pcr_extractor_set *sets;
  /* nonzero: the spherical devox + descriptor stay in the means launch
   * (pcr_extractor_voxel_means_devox + pcr_extractor_voxel_stream) even where
   * the grid stream could evaluate them (pcr_extractor_stream_devox_ok); 0
   * (the default): they ride in the grid stream there */
  int devox_in_means;
} pcr_extractor_args;
pcr_status pcr_extractor_run(pcr_runner *runner, const pcr_extractor_args *args, int steps,
                             int schedule, float *desc_steps, void *origin, void *s_nbr,
                             void *s_pre, void *s_vox);

/* ------------------------------------------------------ self tests ------
 * Device evaluation of the shared bit-exact math (include/pcr_math.h) for
 * host-vs-device parity tests.  op: 0 acosf, 1 atanf, 2 sqrtf, 3 x/y,
 * 4 spherical index (x: [3,n] coords, y unused, out_i: index with r=aux). */
pcr_status pcr_selftest_math(int op, const float *x, const float *y, int n, int aux, float *out_f,
                             int *out_i, void *stream);
pcr_status pcr_selftest_math_d(int op, const double *x, const double *y, int n, double *out,
                               void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PCR_AMD_H */
