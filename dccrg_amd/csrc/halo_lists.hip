// The halo lists of a rebuilt mesh (update_remote_neighbor_info
// dccrg.hpp:9096-9270, recalculate_neighbor_update_send_receive_lists
// 8590-8752): the remote entries of the neighbor rows, grouped by owner.
#include <algorithm>

#include "dccrgx_internal.hpp"

namespace dccrgx {

namespace {
// owned-elsewhere entries as keys owner * stride + id, or (owners != nullptr,
// ids too deep for such keys) as the id in keys[] and the owner in owners[]
__global__ void extract_remote_kernel(const uint64_t* ids, size_t n, DevMesh M, int rank, uint64_t stride,
                                      uint64_t* keys, uint32_t* owners, unsigned long long* counter) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t id = ids[i];
		if (id == error_cell) continue;
		const int32_t o = dm_owner(M, id);
		if (o < 0 || o == rank) continue;
		const unsigned long long at = atomicAdd(counter, 1ull);
		if (owners) {
			keys[at] = id;
			owners[at] = uint32_t(o);
		} else {
			keys[at] = uint64_t(o) * stride + id;
		}
	}
}

__global__ void extract_send_kernel(const uint64_t* nto_id, const uint32_t* nto_ptr, const uint64_t* slot_ids,
                                    size_t row0, size_t nrows, DevMesh M, int rank, uint64_t stride, uint64_t* keys,
                                    uint32_t* owners, unsigned long long* counter) {
	for (size_t r = blockIdx.x * size_t(blockDim.x) + threadIdx.x; r < nrows; r += size_t(gridDim.x) * blockDim.x) {
		const uint64_t self = slot_ids[row0 + r];
		for (uint32_t e = nto_ptr[r]; e < nto_ptr[r + 1]; e++) {
			const int32_t o = dm_owner(M, nto_id[e]);
			if (o < 0 || o == rank) continue;
			const unsigned long long at = atomicAdd(counter, 1ull);
			if (owners) {
				keys[at] = self;
				owners[at] = uint32_t(o);
			} else {
				keys[at] = uint64_t(o) * stride + self;
			}
		}
	}
}

// the remote ids of a neighbors_to list whose (owner, id) key is not among
// the sorted neighbors_of keys: cells that only this rank's cells' neighbors_to
// reach (the reference's remote neighbors_to-only copies)
__global__ void extract_extra_kernel(const uint64_t* ids, size_t n, DevMesh M, int rank, uint64_t stride,
                                     const uint64_t* of_keys, size_t n_of, uint64_t* out, unsigned long long* counter,
                                     const unsigned long long* n_of_dev = nullptr) {
	if (n_of_dev) n_of = size_t(*n_of_dev);
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t id = ids[i];
		if (id == error_cell) continue;
		const int32_t o = dm_owner(M, id);
		if (o < 0 || o == rank) continue;
		const uint64_t key = uint64_t(o) * stride + id;
		size_t lo = 0, hi = n_of;
		while (lo < hi) {
			const size_t mid = (lo + hi) >> 1;
			if (of_keys[mid] < key)
				lo = mid + 1;
			else
				hi = mid;
		}
		if (lo < n_of && of_keys[lo] == key) continue;
		out[atomicAdd(counter, 1ull)] = id;
	}
}

// 1 where a (owner, id) pair differs from the one before it
__global__ void pair_heads_kernel(const uint64_t* ids, const uint32_t* owners, size_t n, uint8_t* head) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		head[i] = (i == 0 || ids[i] != ids[i - 1] || owners[i] != owners[i - 1]) ? 1 : 0;
}
}  // namespace

// the n extracted entries grouped by owner, each group's ids ascending and
// unique: one 64-bit key sort, or for pairs a sort by id then a stable sort
// by owner and a select of the pair heads
static size_t group_by_owner(uint64_t* keys, uint32_t* owners, size_t n, uint64_t stride, int size,
                             std::map<int, std::vector<uint64_t>>& out, hipStream_t s) {
	out.clear();
	if (!n) return 0;
	if (!owners) {
		// keys = owner * stride + id < size * stride: only those bits sorted
		int bits = 1;
		const uint64_t top = uint64_t(size) * stride;
		while (bits < 64 && (top >> bits)) bits++;
		n = sort_unique_u64(keys, n, s, bits);
		for (uint64_t k : download(keys, n, s)) out[int(k / stride)].push_back(k % stride);
		return n;
	}
	DBuf<uint64_t> k2;
	DBuf<uint32_t> o2;
	k2.alloc(n);
	o2.alloc(n);
	int obits = 1;
	while (obits < 32 && (uint64_t(size) >> obits)) obits++;
	DBuf<uint8_t> head;
	head.alloc(n);
	DevCounter nsel;
	nsel.word();
	with_temp(cub_sort_pairs(keys, k2.p, owners, o2.p, n, 64, s),
	          cub_sort_pairs(o2.p, owners, k2.p, keys, n, obits, s),
	          [&](void* t, size_t&) {
		          if (!t) return hipSuccess;
		          pair_heads_kernel<<<grid_for(n, 256), 256, 0, s>>>(keys, owners, n, head.p);
		          return hipGetLastError();
	          },
	          cub_select_flagged(keys, head.p, k2.p, nsel.d.p, n, s),
	          cub_select_flagged(owners, head.p, o2.p, nsel.d.p, n, s));
	const size_t u = nsel.read(s);
	const std::vector<uint64_t> ids = download(k2.p, u, s);
	const std::vector<uint32_t> own = download(o2.p, u, s);
	for (size_t i = 0; i < u; i++) out[int(own[i])].push_back(ids[i]);
	return u;
}

void k_remote_by_owner(const uint64_t* ids, size_t n, const DevMesh& M, int rank, int size,
                       std::map<int, std::vector<uint64_t>>& out, hipStream_t s, DBuf<uint64_t>* keep, size_t* keep_n) {
	out.clear();
	if (keep_n) *keep_n = 0;
	if (!n) return;
	const uint64_t stride = M.last + 1;
	const bool pairs = uint64_t(size) > ~uint64_t(0) / stride;
	DBuf<uint64_t> keys;
	DBuf<uint32_t> owners;
	keys.alloc(n);
	if (pairs) owners.alloc(n);
	DevCounter ctr;
	launch_per_item(extract_remote_kernel, n, s, ids, n, M, rank, stride, keys.p, owners.p, ctr.zero(s));
	const size_t u = group_by_owner(keys.p, owners.p, ctr.read(s), stride, size, out, s);
	if (keep && !pairs) {
		keep->swap(keys);  // sorted unique (owner * stride + id) keys
		*keep_n = u;
	}
}

bool k_remote_extra(const uint64_t* ids, size_t n, const DevMesh& M, int rank, int size, const uint64_t* of_keys,
                    size_t n_of, std::vector<uint64_t>& out, hipStream_t s) {
	out.clear();
	const uint64_t stride = M.last + 1;
	if (uint64_t(size) > ~uint64_t(0) / stride) return false;  // keys would overflow: the caller's pair path
	if (!n) return true;
	DBuf<uint64_t> ex;
	ex.alloc(n);
	DevCounter ctr;
	launch_per_item(extract_extra_kernel, n, s, ids, n, M, rank, stride, of_keys, n_of, ex.p, ctr.zero(s),
	                nullptr);
	const size_t k = ctr.read(s);
	if (k) {
		out = download(ex.p, k, s);
		std::sort(out.begin(), out.end());
		out.erase(std::unique(out.begin(), out.end()), out.end());
	}
	return true;
}

void k_send_by_owner(const uint64_t* nto_id, const uint32_t* nto_ptr, size_t n_entries, const uint64_t* slot_ids,
                     size_t row0, size_t nrows, const DevMesh& M, int rank, int size,
                     std::map<int, std::vector<uint64_t>>& out, hipStream_t s) {
	out.clear();
	if (!nrows || !n_entries) return;
	const uint64_t stride = M.last + 1;
	const bool pairs = uint64_t(size) > ~uint64_t(0) / stride;
	DBuf<uint64_t> keys;
	DBuf<uint32_t> owners;
	keys.alloc(n_entries);
	if (pairs) owners.alloc(n_entries);
	DevCounter ctr;
	launch_per_item(extract_send_kernel, nrows, s, nto_id, nto_ptr, slot_ids, row0, nrows, M, rank, stride, keys.p,
	                owners.p, ctr.zero(s));
	group_by_owner(keys.p, owners.p, ctr.read(s), stride, size, out, s);
}

namespace {
// a sorted unique list padded with one sentinel group: drop it from the count
__global__ void drop_sentinel_kernel(const uint64_t* __restrict__ u, unsigned long long* __restrict__ cnt, uint64_t v) {
	if (threadIdx.x == 0 && *cnt > 0 && u[*cnt - 1] == v) *cnt -= 1;
}
__global__ void strip_owner_kernel(const uint64_t* __restrict__ keys, const unsigned long long* __restrict__ cnt,
                                   uint64_t stride, uint64_t* __restrict__ ids) {
	const size_t n = size_t(*cnt);
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		ids[i] = keys[i] % stride;
}
}  // namespace

// keys padded with sentinels to their capacity, sorted and made unique on
// the device, the count left on the device (no host read)
static void sort_unique_padded(DBuf<uint64_t>& keys, size_t cap, int bits, uint64_t sentinel, DBuf<uint64_t>& uniq,
                               unsigned long long* d_count, hipStream_t s) {
	DBuf<uint64_t> tmp;
	tmp.alloc(cap + 1);
	uniq.alloc(cap + 1);
	with_temp(cub_sort_keys(keys.p, tmp.p, cap, bits, s), cub_select_unique(tmp.p, uniq.p, d_count, cap, s));
	drop_sentinel_kernel<<<1, 64, 0, s>>>(uniq.p, d_count, sentinel);
	HIP_CHECK(hipGetLastError());
}

bool k_halo_lists(const uint64_t* of_id, size_t t_of, const uint64_t* to_id, const uint32_t* p_to, size_t t_to,
                  const uint64_t* slot_ids, size_t row0, size_t nrows, const DevMesh& M, int rank, int size,
                  HaloLists& out, hipStream_t s) {
	out.recv.clear();
	out.send.clear();
	out.extra.clear();
	out.n_recv = out.n_send = 0;
	const uint64_t stride = M.last + 1;
	if (uint64_t(size) > ~uint64_t(0) / stride) return false;  // keys would overflow: the pair path
	int bits = 1;
	const uint64_t top = uint64_t(size) * stride;
	while (bits < 64 && (top >> bits)) bits++;
	const uint64_t sentinel = bits >= 64 ? ~uint64_t(0) : (uint64_t(1) << bits) - 1;  // > every key
	DBuf<unsigned long long> cnt;  // 0 of keys, 1 to keys, 2 extra ids, 3 extract counter of, 4 of to
	cnt.alloc(5);
	HIP_CHECK(hipMemsetAsync(cnt.p, 0, 5 * sizeof(unsigned long long), s));
	DBuf<uint64_t> kof, kto;
	const size_t cof = std::max<size_t>(t_of, 1), cto = std::max<size_t>(t_to, 1);
	kof.alloc(cof + 1);
	kto.alloc(cto + 1);
	k_fill_u64(kof.p, cof, sentinel, s);
	k_fill_u64(kto.p, cto, sentinel, s);
	if (t_of)
		extract_remote_kernel<<<grid_for(t_of, 256), 256, 0, s>>>(of_id, t_of, M, rank, stride, kof.p, nullptr, cnt.p + 3);
	if (nrows && t_to)
		extract_send_kernel<<<grid_for(nrows, 256), 256, 0, s>>>(to_id, p_to, slot_ids, row0, nrows, M, rank, stride, kto.p,
		                                                         nullptr, cnt.p + 4);
	HIP_CHECK(hipGetLastError());
	// the extracted counts first: sorting the capacity (several times the
	// remote entries) costs more than this read
	unsigned long long ext[2] = {0, 0};
	d2h_small(ext, cnt.p + 3, sizeof(ext), s);
	if (ext[0]) sort_unique_padded(kof, size_t(ext[0]), bits, sentinel, out.recv_keys, cnt.p + 0, s);
	else out.recv_keys.alloc(1);
	if (ext[1]) sort_unique_padded(kto, size_t(ext[1]), bits, sentinel, out.send_keys, cnt.p + 1, s);
	else out.send_keys.alloc(1);
	// remote neighbors_to that are no neighbors_of (none for a symmetric hood)
	DBuf<uint64_t> ex;
	ex.alloc(cto + 1);
	if (t_to)
		extract_extra_kernel<<<grid_for(t_to, 256), 256, 0, s>>>(to_id, t_to, M, rank, stride, out.recv_keys.p, 0, ex.p,
		                                                         cnt.p + 2, cnt.p + 0);
	HIP_CHECK(hipGetLastError());
	unsigned long long h[3] = {0, 0, 0};
	d2h_small(h, cnt.p, sizeof(h), s);
	out.n_recv = size_t(h[0]);
	out.n_send = size_t(h[1]);
	// the three lists in one read
	const size_t b0 = 8 * size_t(h[0]), b1 = 8 * size_t(h[1]), b2 = 8 * size_t(h[2]);
	std::vector<uint64_t> all((b0 + b1 + b2) / 8);
	if (!all.empty()) {
		DBuf<uint8_t> stage;
		stage.alloc(b0 + b1 + b2);
		if (b0) HIP_CHECK(hipMemcpyAsync(stage.p, out.recv_keys.p, b0, hipMemcpyDeviceToDevice, s));
		if (b1) HIP_CHECK(hipMemcpyAsync(stage.p + b0, out.send_keys.p, b1, hipMemcpyDeviceToDevice, s));
		if (b2) HIP_CHECK(hipMemcpyAsync(stage.p + b0 + b1, ex.p, b2, hipMemcpyDeviceToDevice, s));
		d2h_small(all.data(), stage.p, b0 + b1 + b2, s);
	}
	for (size_t i = 0; i < size_t(h[0]); i++) out.recv[int(all[i] / stride)].push_back(all[i] % stride);
	for (size_t i = 0; i < size_t(h[1]); i++) out.send[int(all[h[0] + i] / stride)].push_back(all[h[0] + i] % stride);
	out.extra.assign(all.begin() + ptrdiff_t(h[0] + h[1]), all.end());
	std::sort(out.extra.begin(), out.extra.end());
	out.extra.erase(std::unique(out.extra.begin(), out.extra.end()), out.extra.end());
	// the lists' ids on the device in wire order (peer, then id): halo slot
	// ids and send cells without an upload
	out.recv_ids.alloc(size_t(h[0]) + 1);
	out.send_ids.alloc(size_t(h[1]) + 1);
	if (h[0]) launch_per_item(strip_owner_kernel, size_t(h[0]), s, out.recv_keys.p, cnt.p + 0, stride, out.recv_ids.p);
	if (h[1]) launch_per_item(strip_owner_kernel, size_t(h[1]), s, out.send_keys.p, cnt.p + 1, stride, out.send_ids.p);
	return true;
}

}  // namespace dccrgx
