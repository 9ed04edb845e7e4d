// Generic device primitives (device_prims.hip, the one source that includes
// hipcub) and the host idioms their callers share.  Included by
// dccrgx_internal.hpp once DBuf, upload, download and d2h_small are declared.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <functional>

namespace dccrgx {

// The two-call pattern of hipcub and rocprim.  Each op forwards (temp, bytes)
// to one primitive: all are asked for their size (temp == nullptr), one temp
// of the largest size, never empty, is allocated, and the ops run in order.
// A kernel between two primitives is an op that does nothing when temp is null.
using TempOp = std::function<hipError_t(void* temp, size_t& bytes)>;
template <class... Op>
inline void with_temp(Op&&... op) {
	size_t bytes[sizeof...(Op)] = {};
	size_t most = 1, i = 0;
	auto ask = [&](auto& f) { HIP_CHECK(f(nullptr, bytes[i])); most = std::max(most, bytes[i++]); };
	(ask(op), ...);
	DBuf<uint8_t> temp;
	temp.alloc(most);
	i = 0;
	auto run = [&](auto& f) { HIP_CHECK(f(static_cast<void*>(temp.p), bytes[i++])); };
	(run(op), ...);
}

// One 64-bit device word that kernels add to or a primitive writes its count
// to: zero() before the launch (allocates on first use), read() drains s.
struct DevCounter {
	DBuf<unsigned long long> d;
	// allocated, not zeroed: for a primitive that writes the count itself
	unsigned long long* word() {
		d.alloc(1);
		return d.p;
	}
	unsigned long long* zero(hipStream_t s) {
		d.alloc(1);
		HIP_CHECK(hipMemsetAsync(d.p, 0, sizeof(unsigned long long), s));
		return d.p;
	}
	size_t read(hipStream_t s) const {
		unsigned long long h = 0;
		d2h_small(&h, d.p, sizeof(h), s);
		return size_t(h);
	}
};

// a sorted host list on the device: the caller's copy when it has one, else
// uploaded into `own`
inline const uint64_t* given_or_upload(const uint64_t* given, const std::vector<uint64_t>& host, DBuf<uint64_t>& own,
                                       hipStream_t s) {
	if (given) return given;
	upload(own, host, s);
	return own.p;
}

void k_fill_i32(int32_t* p, size_t n, int32_t v, hipStream_t s);
void k_fill_u64(uint64_t* p, size_t n, uint64_t v, hipStream_t s);
void k_iota_i32(int32_t* out, size_t n, int32_t first, hipStream_t s);
void k_iota_u64(uint64_t* out, uint64_t first, size_t n, hipStream_t s);

size_t sort_unique_u64(uint64_t* keys, size_t n, hipStream_t s, int end_bit = 64);  // in place; keys < 2^end_bit
void sort_u64(uint64_t* keys, size_t n, hipStream_t s, int end_bit = 64);  // in place; keys < 2^end_bit
void host_sort_u64(std::vector<uint64_t>& v, bool unique, hipStream_t s);  // host list, device radix sort when large
// scans of n + 1 entries: out[n] = sum(in[0..n)), which is returned
uint32_t scan_exclusive_u32(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s);
uint64_t scan_exclusive_u64(const uint64_t* in, uint64_t* out, size_t n, hipStream_t s);
// two scans of n + 1 entries (the same temp storage size), both totals in one read
void scan_exclusive_u32_pair(const uint32_t* in1, uint32_t* out1, const uint32_t* in2, uint32_t* out2, size_t n,
                             hipStream_t s, size_t& t1, size_t& t2);
// the same, and out[at[j]] (j < k <= 3) into vals, all in one device read
uint32_t scan_exclusive_u32_at(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s, const size_t* at, int k,
                               uint32_t* vals);

// Ids that launch(out, counter, cap) appends to `cap` places (every id counted,
// those with a place written), sorted, unique and on the host.  A count above
// the capacity becomes the capacity of one more launch.  DCCRGX_APPEND_CAP,
// read at each call, replaces first_cap (tests force the second launch).
template <class Launch>
inline std::vector<uint64_t> collect_sorted_unique(size_t first_cap, int id_bits, hipStream_t s, Launch launch) {
	const char* ac = std::getenv("DCCRGX_APPEND_CAP");
	unsigned long long cap = ac && *ac ? std::strtoull(ac, nullptr, 10) : first_cap;
	for (;;) {
		DBuf<uint64_t> out;
		out.alloc(size_t(cap));
		DevCounter ctr;
		launch(out.p, ctr.zero(s), cap);
		HIP_CHECK(hipGetLastError());
		const size_t k = ctr.read(s);
		if (k > cap) {
			cap = k;
			continue;
		}
		const size_t u = sort_unique_u64(out.p, k, s, id_bits);
		return download(out.p, u, s);
	}
}

// hipcub and rocprim as ops for with_temp: radix sorts of the key bits
// [0, end_bit), select, run reduction, merge of two sorted runs
template <class K>
TempOp cub_sort_keys(const K* in, K* out, size_t n, int end_bit, hipStream_t s);
template <class K, class V>
TempOp cub_sort_pairs(const K* kin, K* kout, const V* vin, V* vout, size_t n, int end_bit, hipStream_t s);
template <class T>
TempOp cub_select_flagged(T* in, uint8_t* flags, T* out, unsigned long long* n_out, size_t n, hipStream_t s);
TempOp cub_select_unique(uint64_t* in, uint64_t* out, unsigned long long* n_out, size_t n, hipStream_t s);
TempOp cub_sum_by_key(uint64_t* kin, uint64_t* kout, uint64_t* vin, uint64_t* vout, unsigned long long* n_runs,
                      size_t n, hipStream_t s);
TempOp prim_merge_pairs(uint64_t* k1, uint64_t* k2, uint64_t* kout, uint64_t* v1, uint64_t* v2, uint64_t* vout,
                        size_t n1, size_t n2, hipStream_t s);

}  // namespace dccrgx
