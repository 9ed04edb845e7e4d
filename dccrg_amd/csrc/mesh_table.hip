// The rank's leaf knowledge on the device (dccrgx_mesh.hpp): the hash table
// and the range map of (id -> owner, slot), their inserts, clears and
// lookups, and the per-slot tables derived from lookups.
#include <algorithm>

#include "dccrgx_internal.hpp"

namespace dccrgx {

namespace {
// insert (id, owner, slot = -1); keys are unique
__global__ void hash_insert_kernel(HashEntry* tab, uint64_t mask, uint32_t shift, const uint64_t* ids,
                                   const int32_t* owners, int32_t owner_const, size_t n, size_t slot_upto) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t id = ids[i];
		uint64_t h = hash_home(id, shift);
		for (;;) {
			unsigned long long* kp = reinterpret_cast<unsigned long long*>(&tab[h].key);
			const unsigned long long prev = atomicCAS(kp, 0ull, (unsigned long long)id);
			if (prev == 0ull || prev == id) {
				tab[h].owner = owners ? owners[i] : owner_const;
				tab[h].slot = i < slot_upto ? int32_t(i) : -1;
				break;
			}
			h = (h + 1) & mask;
		}
	}
}

// per refinement level the smallest and largest id of a list (one atomic
// per block and bound, the block's bounds reduced in LDS first)
__global__ __launch_bounds__(256) void level_ranges_kernel(MapCtx m, const uint64_t* __restrict__ ids, size_t n,
                                                           unsigned long long* lo, unsigned long long* hi) {
	__shared__ unsigned long long slo[kRangeLevels], shi[kRangeLevels];
	if (threadIdx.x < kRangeLevels) {
		slo[threadIdx.x] = ~0ull;
		shi[threadIdx.x] = 0ull;
	}
	__syncthreads();
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t id = ids[i];
		const int L = map_level(m, id);
		if (L < 0 || L >= kRangeLevels) continue;
		atomicMin(&slo[L], (unsigned long long)id);
		atomicMax(&shi[L], (unsigned long long)id);
	}
	__syncthreads();
	if (threadIdx.x < kRangeLevels && shi[threadIdx.x]) {
		atomicMin(lo + threadIdx.x, slo[threadIdx.x]);
		atomicMax(hi + threadIdx.x, shi[threadIdx.x]);
	}
}
}  // namespace

void k_hash_insert(HashEntry* tab, uint64_t mask, uint32_t shift, const uint64_t* ids, const int32_t* owners,
                   int32_t owner_const, size_t n, hipStream_t s, size_t slot_upto) {
	launch_per_item(hash_insert_kernel, n, s, tab, mask, shift, ids, owners, owner_const, n, slot_upto);
}

bool k_level_ranges(const MapCtx& m, const uint64_t* ids, size_t n, uint64_t* lo, uint64_t* hi, hipStream_t s) {
	if (m.R >= kRangeLevels) return false;
	DBuf<unsigned long long> d;
	d.alloc(2 * kRangeLevels);
	std::vector<unsigned long long> h(2 * kRangeLevels);
	for (int L = 0; L < kRangeLevels; L++) {
		h[size_t(L)] = ~0ull;
		h[size_t(kRangeLevels + L)] = 0ull;
	}
	h2d(d.p, h.data(), h.size() * 8, s);
	if (n) {
		level_ranges_kernel<<<std::min<unsigned>(grid_for(n, 256), 2048), 256, 0, s>>>(m, ids, n, d.p,
		                                                                              d.p + kRangeLevels);
		HIP_CHECK(hipGetLastError());
	}
	d2h_small(h.data(), d.p, h.size() * 8, s);
	for (int L = 0; L < kRangeLevels; L++) {
		lo[L] = h[size_t(L)];
		hi[L] = h[size_t(kRangeLevels + L)];
	}
	return true;
}

namespace {
// every id of the list written by one thread: no atomics
__global__ void range_insert_kernel(int2* __restrict__ rmap, DevMesh M, const uint64_t* __restrict__ ids,
                                    const int32_t* __restrict__ owners, size_t n, size_t slot_upto) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const int64_t k = dm_range_index(M, ids[i]);
		if (k >= 0) rmap[k] = make_int2(owners ? owners[i] : -2, i < slot_upto ? int32_t(i) : -1);
	}
}

__global__ void range_clear_kernel(int2* __restrict__ rmap, DevMesh M, const uint64_t* __restrict__ ids, size_t n) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const int64_t k = dm_range_index(M, ids[i]);
		if (k >= 0) rmap[k] = make_int2(-1, -1);
	}
}
}  // namespace

void k_range_insert(int2* rmap, const DevMesh& M, const uint64_t* ids, const int32_t* owners, size_t n, size_t slot_upto,
                    hipStream_t s) {
	launch_per_item(range_insert_kernel, n, s, rmap, M, ids, owners, n, slot_upto);
}

void k_range_clear(int2* rmap, const DevMesh& M, const uint64_t* ids, size_t n, hipStream_t s) {
	launch_per_item(range_clear_kernel, n, s, rmap, M, ids, n);
}

namespace {
__global__ void hash_set_slots_kernel(DevMesh M, const uint64_t* slot_ids, size_t n, int32_t* err) {
	if (M.rmap) {
		int2* rmap = const_cast<int2*>(M.rmap);
		for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
			const int64_t k = dm_range_index(M, slot_ids[i]);
			if (k < 0 || rmap[k].x < 0) atomicExch(err, 1);
			else rmap[k].y = int32_t(i);
		}
		return;
	}
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t id = slot_ids[i];
		uint64_t h = hash_home(id, M.shift);
		HashEntry* tab = const_cast<HashEntry*>(M.tab);
		for (;;) {
			const uint64_t k = tab[h].key;
			if (k == id) {
				tab[h].slot = int32_t(i);
				break;
			}
			if (k == 0) {
				atomicExch(err, 1);
				break;
			}
			h = (h + 1) & M.mask;
		}
	}
}

__global__ void lookup_kernel(DevMesh M, const uint64_t* ids, size_t n, int32_t* owner, int32_t* slot) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t id = ids[i];
		if (owner) owner[i] = dm_owner(M, id);
		if (slot) slot[i] = dm_slot(M, id);
	}
}

__global__ void lookup_slots_kernel(const uint64_t* ids, size_t n, DevMesh M, int32_t* out, int32_t* err) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const int32_t s = dm_slot(M, ids[i]);
		out[i] = s;
		if (s < 0) atomicExch(err, 1);
	}
}
}  // namespace

void k_hash_set_slots(const DevMesh& M, const uint64_t* slot_ids, size_t n, int32_t* err, hipStream_t s) {
	launch_per_item(hash_set_slots_kernel, n, s, M, slot_ids, n, err);
}

void k_lookup(const DevMesh& M, const uint64_t* ids, size_t n, int32_t* owner, int32_t* slot, hipStream_t s) {
	launch_per_item(lookup_kernel, n, s, M, ids, n, owner, slot);
}

void k_lookup_slots(const uint64_t* ids, size_t n, const DevMesh& M, int32_t* out, int32_t* err_flag, hipStream_t s) {
	launch_per_item(lookup_slots_kernel, n, s, ids, n, M, out, err_flag);
}

void k_sorted_slot_index(const uint64_t* slot_ids, size_t n, std::vector<uint64_t>& ids, std::vector<int32_t>& slots,
                         hipStream_t s) {
	ids.clear();
	slots.clear();
	if (!n) return;
	DBuf<uint64_t> k2;
	DBuf<int32_t> v1, v2;
	k2.alloc(n);
	v1.alloc(n);
	v2.alloc(n);
	k_iota_i32(v1.p, n, 0, s);
	with_temp(cub_sort_pairs(slot_ids, k2.p, v1.p, v2.p, n, 64, s));
	ids = download(k2.p, n, s);
	slots = download(v2.p, n, s);
}

namespace {
// where each slot of a rebuilt mesh takes its payload from (rebuild step 6;
// the gathers write zeros where there is no source):
// the old local slot of the same cell, else (a new local cell absent from the
// old mesh: a refined cell's child) the old slot of its parent, else nothing
__global__ void carry_src_kernel(const uint64_t* __restrict__ slot_ids, size_t n_slots, size_t nl, MapCtx m,
                                 DevMesh oldM, size_t old_n_local, int32_t* __restrict__ src) {
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n_slots; s += size_t(gridDim.x) * blockDim.x) {
		const uint64_t id = slot_ids[s];
		const int32_t o = dm_slot(oldM, id);
		int32_t r = -1;
		if (o >= 0) {
			if (size_t(o) < old_n_local) r = o;
		} else if (s < nl) {
			const uint64_t p = map_parent(m, id);
			if (p != error_cell && p != id) r = dm_slot(oldM, p);
		}
		src[s] = r;
	}
}

// bits 0-4: the level; bits 5-7: the cell's octant in its parent (bit k set
// when its index along axis k is odd at its level; 0 at level 0), which is
// the corner test of adapter.hpp:84-102 without the cell's indices
__global__ void slot_levels_kernel(MapCtx m, const uint64_t* slot_ids, size_t n, uint8_t* lvl) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		uint64_t x, y, z;
		const int l = map_indices(m, slot_ids[i], x, y, z);
		const int sh = m.R - l;
		const unsigned oct = l ? unsigned(((x >> sh) & 1) | (((y >> sh) & 1) << 1) | (((z >> sh) & 1) << 2)) : 0u;
		lvl[i] = uint8_t(unsigned(l) | (oct << 5));
	}
}
}  // namespace

void k_carry_src(const uint64_t* slot_ids, size_t n_slots, size_t nl, const MapCtx& m, const DevMesh& oldM,
                 size_t old_n_local, int32_t* src, hipStream_t s) {
	launch_per_item(carry_src_kernel, n_slots, s, slot_ids, n_slots, nl, m, oldM, old_n_local, src);
}

void k_slot_levels(const MapCtx& m, const uint64_t* slot_ids, size_t n, uint8_t* lvl, hipStream_t s) {
	launch_per_item(slot_levels_kernel, n, s, m, slot_ids, n, lvl);
}

}  // namespace dccrgx
