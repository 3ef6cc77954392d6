// voxelize.hpp -- what voxelize.hip (clouds of <= kMaxSortN points and the
// extractor's voxel stage) and voxelize_big.hip (larger clouds) share.
#pragma once

#include "common.hpp"

namespace pcr {

constexpr int kPrepThreads = kSortBlock;
constexpr int kMaxSortN = kSortBlock * kMaxE;

enum PrepMode { kSphCoords = 0, kSphNormalize = 1, kCube = 2 };

// voxelize_big.hip: the voxelization of clouds of more than kMaxSortN points
// (grid, ind, cnt as run_voxelize's), its workspace (c > 0: with room for the
// point-major feature copy) and pcr_spherical_normalize at that size
size_t vox_big_ws_size(int b, int n, int r, int c);
pcr_status run_voxelize_big(PrepMode mode, const float* features, const float* coords_f,
                            const int* coords_i, int b, int c, int n, int r, float* out, int* ind,
                            int* cnt, void* workspace, size_t ws_bytes, hipStream_t stream,
                            const char* name);
void launch_sph_normalize_big(const float* coords, int b, int n, float* norm_coords,
                              hipStream_t stream);

}  // namespace pcr
