// Generic device primitives (dccrgx_prims.hpp): fill, iota, sort, unique and
// scan, and hipcub / rocprim behind typed entry points.  The one source that
// includes hipcub, so each of its kernels is instantiated once.
#include <hipcub/hipcub.hpp>
#include <rocprim/device/device_merge.hpp>

#include "dccrgx_internal.hpp"

namespace dccrgx {

// ---- fill and iota ----------------------------------------------------------
namespace {
__global__ void fill_i32_kernel(int32_t* p, size_t n, int32_t v) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		p[i] = v;
}

__global__ void fill_u64_kernel(uint64_t* __restrict__ p, size_t n, uint64_t v) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) p[i] = v;
}

__global__ void iota_i32_from_kernel(int32_t* out, size_t n, int32_t first) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		out[i] = first + int32_t(i);
}

__global__ void iota_u64_kernel(uint64_t* out, uint64_t first, size_t n) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		out[i] = first + i;
}
}  // namespace

void k_fill_i32(int32_t* p, size_t n, int32_t v, hipStream_t s) { launch_per_item(fill_i32_kernel, n, s, p, n, v); }
void k_fill_u64(uint64_t* p, size_t n, uint64_t v, hipStream_t s) { launch_per_item(fill_u64_kernel, n, s, p, n, v); }
void k_iota_i32(int32_t* out, size_t n, int32_t first, hipStream_t s) {
	launch_per_item(iota_i32_from_kernel, n, s, out, n, first);
}
void k_iota_u64(uint64_t* out, uint64_t first, size_t n, hipStream_t s) {
	launch_per_item(iota_u64_kernel, n, s, out, first, n);
}

// ---- hipcub and rocprim by element type -----------------------------------------
template <class K>
TempOp cub_sort_keys(const K* in, K* out, size_t n, int end_bit, hipStream_t s) {
	return [=](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortKeys(t, b, in, out, n, 0, end_bit, s); };
}
template TempOp cub_sort_keys(const uint64_t*, uint64_t*, size_t, int, hipStream_t);
template TempOp cub_sort_keys(const uint32_t*, uint32_t*, size_t, int, hipStream_t);

template <class K, class V>
TempOp cub_sort_pairs(const K* kin, K* kout, const V* vin, V* vout, size_t n, int end_bit, hipStream_t s) {
	return [=](void* t, size_t& b) {
		return hipcub::DeviceRadixSort::SortPairs(t, b, kin, kout, vin, vout, n, 0, end_bit, s);
	};
}
template TempOp cub_sort_pairs(const uint64_t*, uint64_t*, const uint64_t*, uint64_t*, size_t, int, hipStream_t);
template TempOp cub_sort_pairs(const uint64_t*, uint64_t*, const uint32_t*, uint32_t*, size_t, int, hipStream_t);
template TempOp cub_sort_pairs(const uint64_t*, uint64_t*, const int32_t*, int32_t*, size_t, int, hipStream_t);
template TempOp cub_sort_pairs(const uint32_t*, uint32_t*, const uint64_t*, uint64_t*, size_t, int, hipStream_t);

template <class T>
TempOp cub_select_flagged(T* in, uint8_t* flags, T* out, unsigned long long* n_out, size_t n, hipStream_t s) {
	return [=](void* t, size_t& b) { return hipcub::DeviceSelect::Flagged(t, b, in, flags, out, n_out, n, s); };
}
template TempOp cub_select_flagged(uint64_t*, uint8_t*, uint64_t*, unsigned long long*, size_t, hipStream_t);
template TempOp cub_select_flagged(uint32_t*, uint8_t*, uint32_t*, unsigned long long*, size_t, hipStream_t);

TempOp cub_select_unique(uint64_t* in, uint64_t* out, unsigned long long* n_out, size_t n, hipStream_t s) {
	return [=](void* t, size_t& b) { return hipcub::DeviceSelect::Unique(t, b, in, out, n_out, n, s); };
}

TempOp cub_sum_by_key(uint64_t* kin, uint64_t* kout, uint64_t* vin, uint64_t* vout, unsigned long long* n_runs,
                      size_t n, hipStream_t s) {
	return [=](void* t, size_t& b) {
		return hipcub::DeviceReduce::ReduceByKey(t, b, kin, kout, vin, vout, n_runs, hipcub::Sum(), n, s);
	};
}

TempOp prim_merge_pairs(uint64_t* k1, uint64_t* k2, uint64_t* kout, uint64_t* v1, uint64_t* v2, uint64_t* vout,
                        size_t n1, size_t n2, hipStream_t s) {
	return [=](void* t, size_t& b) {
		return rocprim::merge(t, b, k1, k2, kout, v1, v2, vout, n1, n2, rocprim::less<uint64_t>(), s);
	};
}

// ---- sort and unique ------------------------------------------------------------
// a host list sorted (and deduplicated): by the device radix sort above a few
// thousand ids (std::sort of 200 K ids takes 5-15 ms on the host), else here
void host_sort_u64(std::vector<uint64_t>& v, bool unique, hipStream_t s) {
	// already in order (lists that arrive sorted: one rank's own, merged runs)
	if (unique ? std::adjacent_find(v.begin(), v.end(), std::greater_equal<uint64_t>()) == v.end()
	           : std::is_sorted(v.begin(), v.end()))
		return;
	if (v.size() < 8192) {
		std::sort(v.begin(), v.end());
		if (unique) v.erase(std::unique(v.begin(), v.end()), v.end());
		return;
	}
	DBuf<uint64_t> d;
	upload(d, v, s);
	const size_t n = unique ? sort_unique_u64(d.p, v.size(), s) : (sort_u64(d.p, v.size(), s), v.size());
	v = download(d.p, n, s);
}

void sort_u64(uint64_t* keys, size_t n, hipStream_t s, int end_bit) {
	if (n < 2) return;
	DBuf<uint64_t> tmp;
	tmp.alloc(n);
	with_temp(cub_sort_keys(keys, tmp.p, n, end_bit, s));
	// stream-ordered: every caller reads the keys on `s` (device consumers)
	// or through a download that drains it.  (Round 5 restored a sync here
	// after a Poisson transport failure; the cause was null-stream memsets
	// racing the compute stream, DESIGN.md section 6, not this function.)
	HIP_CHECK(hipMemcpyAsync(keys, tmp.p, n * 8, hipMemcpyDeviceToDevice, s));
}

size_t sort_unique_u64(uint64_t* keys, size_t n, hipStream_t s, int end_bit) {
	if (n == 0) return 0;
	DBuf<uint64_t> tmp;
	tmp.alloc(n);
	DevCounter nsel;
	nsel.word();
	with_temp(cub_sort_keys(keys, tmp.p, n, end_bit, s), cub_select_unique(tmp.p, keys, nsel.d.p, n, s));
	return nsel.read(s);
}

// ---- scans ------------------------------------------------------------------------
namespace {
struct PickU32 {
	size_t at[4];
	int k;
};
__global__ void pick_u32_kernel(const uint32_t* __restrict__ v, PickU32 p, uint32_t* __restrict__ out) {
	if (int(threadIdx.x) < p.k) out[threadIdx.x] = v[p.at[threadIdx.x]];
}

// scans n + 1 entries: out[n] = sum(in[0..n))
template <class T>
auto exclusive_sum(const T* in, T* out, size_t n, hipStream_t s) {
	return [=](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, in, out, n + 1, s); };
}
}  // namespace

uint32_t scan_exclusive_u32_at(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s, const size_t* at, int k,
                               uint32_t* vals) {
	DX_REQUIRE(k >= 0 && k <= 3, "internal error: too many scan positions");
	with_temp(exclusive_sum(in, out, n, s));
	// the total and the k positions in one read
	PickU32 p{{n, 0, 0, 0}, k + 1};
	for (int j = 0; j < k; j++) p.at[j + 1] = at[j];
	DBuf<uint32_t> picked;
	picked.alloc(4);
	pick_u32_kernel<<<1, 64, 0, s>>>(out, p, picked.p);
	HIP_CHECK(hipGetLastError());
	uint32_t h[4] = {0, 0, 0, 0};
	d2h_small(h, picked.p, sizeof(uint32_t) * size_t(k + 1), s);
	for (int j = 0; j < k; j++) vals[j] = h[j + 1];
	return h[0];
}

void scan_exclusive_u32_pair(const uint32_t* in1, uint32_t* out1, const uint32_t* in2, uint32_t* out2, size_t n,
                             hipStream_t s, size_t& t1, size_t& t2) {
	with_temp(exclusive_sum(in1, out1, n, s), exclusive_sum(in2, out2, n, s));
	DBuf<uint32_t> tot;
	tot.alloc(2);
	HIP_CHECK(hipMemcpyAsync(tot.p, out1 + n, 4, hipMemcpyDeviceToDevice, s));
	HIP_CHECK(hipMemcpyAsync(tot.p + 1, out2 + n, 4, hipMemcpyDeviceToDevice, s));
	uint32_t h[2] = {0, 0};
	d2h_small(h, tot.p, sizeof(h), s);
	t1 = h[0];
	t2 = h[1];
}

uint32_t scan_exclusive_u32(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s) {
	with_temp(exclusive_sum(in, out, n, s));
	uint32_t h = 0;
	d2h_small(&h, out + n, sizeof(h), s);
	return h;
}

uint64_t scan_exclusive_u64(const uint64_t* in, uint64_t* out, size_t n, hipStream_t s) {
	// in[n] is ignored
	with_temp(exclusive_sum(in, out, n, s));
	uint64_t h = 0;
	d2h_small(&h, out + n, sizeof(h), s);
	return h;
}

}  // namespace dccrgx
