// The movers of fixed-size cell payloads: pack / place of the halo, the
// migration and the removed store (bytes [off, off + len) of the elements at
// a slot list) and the row gather that carries a field over a mesh rebuild.
// Whole 4-, 8- (and, for the gather, 16-) byte elements move typed, every
// other size and window byte by byte (tests/test_gpu_payload_bytes.py).
#include "dccrgx_internal.hpp"

namespace dccrgx {

namespace {

// pack / place: bytes [off, off + len) of the elements at `slots`
template <class T>
__global__ void pack_kernel(const T* __restrict__ f, const int32_t* __restrict__ slots, size_t n, T* __restrict__ out) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		out[i] = f[slots[i]];
}

template <class T>
__global__ void place_kernel(const T* __restrict__ in, const int32_t* __restrict__ slots, size_t n, T* __restrict__ f) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		f[slots[i]] = in[i];
}

__global__ void pack_bytes_kernel(const uint8_t* __restrict__ f, size_t elem, size_t off, size_t len,
                                  const int32_t* __restrict__ slots, size_t n, uint8_t* __restrict__ out) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n * len; i += size_t(gridDim.x) * blockDim.x) {
		const size_t k = i / len, b = i - k * len;
		out[i] = f[size_t(slots[k]) * elem + off + b];
	}
}

__global__ void place_bytes_kernel(const uint8_t* __restrict__ in, size_t elem, size_t off, size_t len,
                                   const int32_t* __restrict__ slots, size_t n, uint8_t* __restrict__ f) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n * len; i += size_t(gridDim.x) * blockDim.x) {
		const size_t k = i / len, b = i - k * len;
		f[size_t(slots[k]) * elem + off + b] = in[i];
	}
}

// out[s] = old[src[s]], zeros where src[s] < 0 (no source)
template <class T>
__global__ void gather_rows_kernel(const T* __restrict__ old, const int32_t* __restrict__ src, size_t n,
                                   T* __restrict__ out) {
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x)
		out[s] = src[s] >= 0 ? old[src[s]] : T{};
}

__global__ void gather_bytes_kernel(const uint8_t* __restrict__ old, const int32_t* __restrict__ src, size_t n,
                                    size_t elem, uint8_t* __restrict__ out) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n * elem; i += size_t(gridDim.x) * blockDim.x) {
		const size_t s = i / elem;
		out[i] = src[s] >= 0 ? old[size_t(src[s]) * elem + (i - s * elem)] : uint8_t(0);
	}
}

}  // namespace

void k_pack(const uint8_t* field, size_t elem, size_t off, size_t len, const int32_t* slots, size_t n, uint8_t* out,
            hipStream_t s) {
	if (!n || !len) return;
	if (off == 0 && len == elem && elem == 4)
		pack_kernel<uint32_t><<<grid_for(n, 256), 256, 0, s>>>((const uint32_t*)field, slots, n, (uint32_t*)out);
	else if (off == 0 && len == elem && elem == 8)
		pack_kernel<uint64_t><<<grid_for(n, 256), 256, 0, s>>>((const uint64_t*)field, slots, n, (uint64_t*)out);
	else
		pack_bytes_kernel<<<grid_for(n * len, 256), 256, 0, s>>>(field, elem, off, len, slots, n, out);
	HIP_CHECK(hipGetLastError());
}

void k_place(const uint8_t* in, size_t elem, size_t off, size_t len, const int32_t* slots, size_t n, uint8_t* field,
             hipStream_t s) {
	if (!n || !len) return;
	if (off == 0 && len == elem && elem == 4)
		place_kernel<uint32_t><<<grid_for(n, 256), 256, 0, s>>>((const uint32_t*)in, slots, n, (uint32_t*)field);
	else if (off == 0 && len == elem && elem == 8)
		place_kernel<uint64_t><<<grid_for(n, 256), 256, 0, s>>>((const uint64_t*)in, slots, n, (uint64_t*)field);
	else
		place_bytes_kernel<<<grid_for(n * len, 256), 256, 0, s>>>(in, elem, off, len, slots, n, field);
	HIP_CHECK(hipGetLastError());
}

void k_gather_rows(const uint8_t* old_data, const int32_t* src, size_t n, size_t elem, uint8_t* out, hipStream_t s) {
	if (!n || !elem) return;
	if (elem == 4)
		gather_rows_kernel<uint32_t><<<grid_for(n, 256), 256, 0, s>>>((const uint32_t*)old_data, src, n, (uint32_t*)out);
	else if (elem == 8)
		gather_rows_kernel<uint64_t><<<grid_for(n, 256), 256, 0, s>>>((const uint64_t*)old_data, src, n, (uint64_t*)out);
	else if (elem == 16)
		gather_rows_kernel<uint4><<<grid_for(n, 256), 256, 0, s>>>((const uint4*)old_data, src, n, (uint4*)out);
	else
		gather_bytes_kernel<<<grid_for(n * elem, 256), 256, 0, s>>>(old_data, src, n, elem, out);
	HIP_CHECK(hipGetLastError());
}

}  // namespace dccrgx
