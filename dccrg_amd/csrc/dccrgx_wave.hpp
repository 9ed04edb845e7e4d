// Wavefront helpers of the mesh build kernels; internal linkage, as when they
// stood in one file's unnamed namespace.
#pragma once

#include "dccrgx_mapping.hpp"

namespace dccrgx {
namespace {

constexpr int WAVE = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }

__device__ __forceinline__ uint64_t lanemask_lt() {
	const int l = lane_id();
	return l == 0 ? 0ull : (~0ull >> (64 - l));
}

__device__ __forceinline__ int wave_incl_scan(int v) {
	const int l = lane_id();
	for (int d = 1; d < WAVE; d <<= 1) {
		const int t = __shfl_up(v, d, WAVE);
		if (l >= d) v += t;
	}
	return v;
}

__device__ __forceinline__ int wave_sum(int v) {
	for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
	return v;
}

__device__ void cell_coords(const MapCtx& m, uint64_t id, uint64_t c[3], int& lvl) {
	lvl = map_indices(m, id, c[0], c[1], c[2]);
}

}  // namespace
}  // namespace dccrgx
