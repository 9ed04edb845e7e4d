// The face table of the local rows (get_face_neighbors_of dccrg.hpp:2806-2933
// semantics) in fixed-width and CSR form, and the Morton order of the slots
// that lets it predict a same-size face neighbor's row.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "dccrgx_internal.hpp"
#include "dccrgx_wave.hpp"

namespace dccrgx {

namespace {

// The fixed-width face table (get_face_neighbors_of semantics), one thread
// per local slot: ell[6 r + d] = the slot of the single (same-size or
// coarser) face neighbor in direction d, -1 none, or -2 - f for the finer
// face f whose 4 slots are fine[4 f ..] in the reference's order.  Finer faces
// are numbered in (row, direction) order: face_table_kernel writes the
// directions with one neighbor and appends the finer ones' keys
// (row << 3 | d); after a sort of the keys face_fine_kernel probes those again.
// A single neighbor without a slot sets *err.
struct SlotExists {
	DevMesh M;
	mutable int32_t slot = -1;
	// DevExists's answer, and the slot of the cell it found
	__device__ __forceinline__ bool operator()(uint64_t id) const {
		slot = -1;
		if (id == 0 || id > M.last) return false;
		if (M.implicit) {
			if (id > M.bp.n0) return false;
			slot = dm_slot(M, id);
			return true;
		}
		int32_t o, sl;
		if (!dm_lookup(M, id, o, sl)) return false;
		slot = sl;
		return o >= 0;
	}
};

__device__ __forceinline__ uint64_t spread3(uint64_t v) {
	v &= 0x1FFFFFull;
	v = (v | (v << 32)) & 0x1F00000000FFFFull;
	v = (v | (v << 16)) & 0x1F0000FF0000FFull;
	v = (v | (v << 8)) & 0x100F00F00F00F00Full;
	v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
	v = (v | (v << 2)) & 0x1249249249249249ull;
	return v;
}

__device__ __forceinline__ uint64_t morton3(const uint64_t c[3]) {
	return spread3(c[0]) | (spread3(c[1]) << 1) | (spread3(c[2]) << 2);
}

// morton: the rows [0, nrows) are Morton-ordered runs [0, run1) and [run1,
// nrows) (k_morton_sort of rebuild step 2).  Then a same-size face neighbor
// is predicted at the row its Morton distance away - exact whenever every
// leaf between the two has that size - and taken when the row holds its id:
// a same-size leaf is the one face neighbor in that direction (no finer or
// coarser probe needed).  o6[dir] = -1 (no face neighbor), the predicted row,
// or kFaceMiss (the probes of face_dir decide).
constexpr int32_t kFaceMiss = -3;
__device__ __forceinline__ void face_predict(const MapCtx& m, const uint64_t* __restrict__ slot_ids, size_t r,
                                             size_t run1, size_t nrows, uint64_t id, const uint64_t c[3], int lvl,
                                             int32_t o6[6]) {
	int32_t h[6];
	uint64_t want[6], got[6];
	bool probe[6];
	const int sh = 3 * (m.R - lvl);
	const uint64_t len = uint64_t(1) << (m.R - lvl);
	const uint64_t key = morton3(c) >> sh;
	const int64_t lo = r < run1 ? 0 : int64_t(run1), hi = r < run1 ? int64_t(run1) : int64_t(nrows);
	// the neighbor's id and Morton key from this cell's: one step along d is
	// +-stride[d] in the id and a dilated +-1 in the key (no re-interleave,
	// no index -> id products); a periodic wrap takes the general form
	const uint64_t lx = m.len[0] << lvl, ly = m.len[1] << lvl;
	const uint64_t stride[3] = {1, lx, lx * ly};
#pragma unroll
	for (int dir = 0; dir < 6; dir++) {
		const int d = dir >> 1;
		uint64_t p[3];
		h[dir] = -1;
		want[dir] = ~uint64_t(0);
		probe[dir] = face_probe(m, c, lvl, dir, p);
		if (!probe[dir]) continue;
		p[d] &= ~(len - 1);  // the other two are c's, aligned
		const uint64_t M = uint64_t(0x1249249249249249ull) << d, u = uint64_t(1) << d;
		uint64_t nkey;
		if ((dir & 1) ? p[d] == c[d] + len : p[d] + len == c[d])
			nkey = (dir & 1) ? ((((key | ~M) + u) & M) | (key & ~M)) : ((((key & M) - u) & M) | (key & ~M));
		else
			nkey = morton3(p) >> sh;
		const int64_t q = int64_t(r) + (int64_t(nkey) - int64_t(key));
		if (q >= lo && q < hi) {
			h[dir] = int32_t(q);
			want[dir] = id + ((p[d] >> (m.R - lvl)) - (c[d] >> (m.R - lvl))) * stride[d];
		}
	}
	// the six row loads in flight together
#pragma unroll
	for (int dir = 0; dir < 6; dir++) got[dir] = h[dir] >= 0 ? slot_ids[h[dir]] : 0;
#pragma unroll
	for (int dir = 0; dir < 6; dir++)
		o6[dir] = !probe[dir] ? -1 : (h[dir] >= 0 && got[dir] == want[dir] ? h[dir] : kFaceMiss);
}

// One thread per row: the predictions, then face_dir's probes for the
// directions they leave open.  The loop runs whole waves (wave_reserve needs
// every lane).
// chunk_keys (non-null): a wave's 64 rows are one chunk (r / 64); its finer
// faces' keys go to chunk_keys[384 c ...] in (row, direction) order and
// their number to chunk_cnt[c], so a scan of the counts numbers every finer
// face in (row, direction) order - no sort of the keys
constexpr uint32_t kChunkKeys = 6 * 64;
__global__ void face_table_kernel(MapCtx m, DevMesh M, const uint64_t* slot_ids, size_t nrows, size_t run1,
                                  bool morton, int32_t* ell, unsigned long long* n_fine, uint32_t* fine_keys,
                                  size_t key_cap, int32_t* err, uint32_t* chunk_keys, uint32_t* chunk_cnt) {
	const SlotExists ex{M};
	const size_t stride = size_t(gridDim.x) * blockDim.x;
	for (size_t r = blockIdx.x * size_t(blockDim.x) + threadIdx.x; r - lane_id() < nrows; r += stride) {
		const bool live = r < nrows;
		int32_t o6[6];
		uint32_t kf = 0;  // finer faces
		if (live) {
			uint64_t c[3];
			int lvl;
			const uint64_t id = slot_ids[r];
			cell_coords(m, id, c, lvl);
			if (morton) face_predict(m, slot_ids, r, run1, nrows, id, c, lvl, o6);
#pragma unroll
			for (int dir = 0; dir < 6; dir++) {
				if (morton && o6[dir] != kFaceMiss) continue;
				uint64_t out[4];
				const int nf = face_dir(m, c, lvl, dir, ex, out);
				// a single neighbor was the last cell found (face_dir returns on it)
				if (nf == 1 && ex.slot < 0) atomicExch(err, 1);
				o6[dir] = nf == 0 ? -1 : (nf == 4 ? -2 : (ex.slot >= 0 ? ex.slot : -1));
				kf += nf == 4 ? 1u : 0u;
			}
			typedef int i2v __attribute__((ext_vector_type(2)));
			i2v* ev = reinterpret_cast<i2v*>(ell + 6 * r);
#pragma unroll
			for (int j = 0; j < 3; j++) ev[j] = i2v{o6[2 * j], o6[2 * j + 1]};
		}
		if (chunk_keys) {
			const int incl = wave_incl_scan(int(kf));
			const size_t c = (r - lane_id()) >> 6;
			if (lane_id() == WAVE - 1) chunk_cnt[c] = uint32_t(incl);
			uint32_t at = uint32_t(incl) - kf;
			if (live)
				for (int dir = 0; dir < 6; dir++)
					if (o6[dir] == -2) chunk_keys[kChunkKeys * c + at++] = (uint32_t(r) << 3) | uint32_t(dir);
			continue;
		}
		if (__ballot(kf != 0) == 0) continue;
		unsigned long long at = wave_reserve(n_fine, kf);
		if (live)
			for (int dir = 0; dir < 6; dir++)
				if (o6[dir] == -2) {
					if (at < key_cap) fine_keys[at] = (uint32_t(r) << 3) | uint32_t(dir);  // else counted only
					at++;
				}
	}
}

// the finer faces in key order: f = the key's position
__global__ void face_fine_kernel(MapCtx m, DevMesh M, const uint64_t* slot_ids, const uint32_t* fine_keys, size_t n,
                                 int32_t* ell, int32_t* fine, int32_t* err, const uint32_t* chunk_keys,
                                 const uint32_t* chunk_off, uint32_t n_chunks) {
	const DevExists ex{M};
	for (size_t f = blockIdx.x * size_t(blockDim.x) + threadIdx.x; f < n; f += size_t(gridDim.x) * blockDim.x) {
		uint32_t key;
		if (chunk_keys) {
			// the chunk holding finer face f: the last offset <= f
			uint32_t lo = 0, hi = n_chunks;
			while (hi - lo > 1) {
				const uint32_t mid = (lo + hi) >> 1;
				if (chunk_off[mid] <= uint32_t(f)) lo = mid;
				else hi = mid;
			}
			key = chunk_keys[size_t(kChunkKeys) * lo + (uint32_t(f) - chunk_off[lo])];
		} else {
			key = fine_keys[f];
		}
		const size_t r = size_t(key >> 3);
		const int dir = int(key & 7);
		uint64_t c[3];
		int lvl;
		cell_coords(m, slot_ids[r], c, lvl);
		uint64_t out[4];
		const int nf = face_dir(m, c, lvl, dir, ex, out);
		if (nf != 4) atomicExch(err, 1);
		int32_t sl[4];
#pragma unroll
		for (int i = 0; i < 4; i++) {
			sl[i] = i < nf ? dm_slot(M, out[i]) : -1;
			if (sl[i] < 0) atomicExch(err, 1);
		}
		reinterpret_cast<int4*>(fine)[f] = int4{sl[0], sl[1], sl[2], sl[3]};
		ell[6 * r + dir] = -2 - int32_t(f);
	}
}

}  // namespace

size_t k_face_table(const MapCtx& m, const DevMesh& M, const uint64_t* slot_ids, size_t nrows, size_t run1,
                    bool morton, int32_t* ell, DBuf<int32_t>& fine, int32_t* err, hipStream_t s) {
	DX_REQUIRE(nrows < (size_t(1) << 29), "too many local cells for the face keys");
	if (nrows && !(std::getenv("DCCRGX_FACE_KEYS") && std::strcmp(std::getenv("DCCRGX_FACE_KEYS"), "sort") == 0)) {
		// finer faces numbered by a scan of per-chunk counts (face_table_kernel)
		const size_t nch = (nrows + 63) / 64;
		DX_REQUIRE(nch * kChunkKeys < (size_t(1) << 32), "too many rows for the chunked face keys");
		DBuf<uint32_t> ckeys, ccnt, coff;
		ckeys.alloc(nch * kChunkKeys);
		ccnt.alloc(nch + 1);
		coff.alloc(nch + 1);
		launch_per_item(face_table_kernel, nrows, s, m, M, slot_ids, nrows, run1, morton && !M.implicit, ell,
		                nullptr, nullptr, 0, err, ckeys.p, ccnt.p);
		const size_t nf = scan_exclusive_u32(ccnt.p, coff.p, nch, s);
		fine.alloc(4 * nf + 4);
		if (!nf) return 0;
		launch_per_item(face_fine_kernel, nf, s, m, M, slot_ids, nullptr, nf, ell, fine.p, err, ckeys.p, coff.p,
		                uint32_t(nch));
		return nf;
	}
	DevCounter n_fine;
	n_fine.word();
	// finer faces: at most 6 per row, in practice a few percent of the rows;
	// keys row << 3 | direction, room for a quarter of the rows first (the
	// pass runs again with room for all of them if that was too little: it
	// rewrites every row of the table)
	DBuf<uint32_t> keys;
	const char* kc = std::getenv("DCCRGX_FACE_KEY_CAP");  // tests: a small first room forces the second pass
	size_t cap = kc && *kc ? size_t(std::strtoull(kc, nullptr, 10)) : nrows / 4 + 1024;
	size_t nf = 0;
	for (;;) {
		n_fine.zero(s);
		keys.alloc(cap);
		if (nrows)
			face_table_kernel<<<grid_for(nrows, 256), 256, 0, s>>>(m, M, slot_ids, nrows, run1, morton && !M.implicit,
			                                                       ell, n_fine.d.p, keys.p, cap, err, nullptr, nullptr);
		HIP_CHECK(hipGetLastError());
		nf = n_fine.read(s);
		if (nf <= cap) break;
		cap = nf;
	}
	fine.alloc(4 * nf + 4);
	if (!nf) return 0;
	int bits = 4;
	while (bits < 32 && (uint64_t(nrows) << 3) >> bits) bits++;
	if (nf > 1) {
		DBuf<uint32_t> sorted;
		sorted.alloc(nf);
		with_temp(cub_sort_keys(keys.p, sorted.p, nf, bits, s));
		keys.swap(sorted);
	}
	launch_per_item(face_fine_kernel, nf, s, m, M, slot_ids, keys.p, nf, ell, fine.p, err, nullptr, nullptr, 0);
	return nf;
}

namespace {
// the CSR form of the table (rows of slot * 8 + direction entries, a row's
// directions ascending, a finer face's four slots in table order): counts,
// then entries from the scan
__global__ void face_csr_count_kernel(const int32_t* ell, size_t nrows, uint32_t* cnt) {
	for (size_t r = blockIdx.x * size_t(blockDim.x) + threadIdx.x; r < nrows; r += size_t(gridDim.x) * blockDim.x) {
		uint32_t k = 0;
		for (int d = 0; d < 6; d++) {
			const int32_t e = ell[6 * r + d];
			k += e >= 0 ? 1u : (e <= -2 ? 4u : 0u);
		}
		cnt[r] = k;
	}
}

__global__ void face_csr_fill_kernel(const int32_t* ell, const int32_t* fine, size_t nrows, const uint32_t* ptr,
                                     int32_t* ent) {
	for (size_t r = blockIdx.x * size_t(blockDim.x) + threadIdx.x; r < nrows; r += size_t(gridDim.x) * blockDim.x) {
		uint32_t k = ptr[r];
		for (int d = 0; d < 6; d++) {
			const int32_t e = ell[6 * r + d];
			if (e >= 0) {
				ent[k++] = e * 8 + d;
			} else if (e <= -2) {
				const size_t f = size_t(-2 - e);
				for (int i = 0; i < 4; i++) ent[k++] = fine[4 * f + i] * 8 + d;
			}
		}
	}
}
}  // namespace

void k_face_csr(const int32_t* ell, const int32_t* fine, size_t nrows, DBuf<uint32_t>& ptr, DBuf<int32_t>& ent,
                hipStream_t s) {
	DBuf<uint32_t> cnt;
	cnt.alloc(nrows + 1);
	ptr.alloc(nrows + 1);
	if (nrows) launch_per_item(face_csr_count_kernel, nrows, s, ell, nrows, cnt.p);
	const size_t t = scan_exclusive_u32(cnt.p, ptr.p, nrows, s);
	ent.alloc(t + 1);
	if (nrows) launch_per_item(face_csr_fill_kernel, nrows, s, ell, fine, nrows, ptr.p, ent.p);
}

namespace {
__global__ void morton_keys_kernel(MapCtx m, const uint64_t* ids, size_t n, uint64_t* keys) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		uint64_t x, y, z;
		map_indices(m, ids[i], x, y, z);
		keys[i] = spread3(x) | (spread3(y) << 1) | (spread3(z) << 2);
	}
}
}  // namespace

// Reorder a run of cell ids along the Morton (z-order) curve of their min
// corners at finest-level resolution (leaves have distinct min corners).
void k_morton_sort(const MapCtx& m, uint64_t* ids, size_t n, hipStream_t s) {
	if (n < 2) return;
	DBuf<uint64_t> keys, keys2, ids2;
	keys.alloc(n);
	keys2.alloc(n);
	ids2.alloc(n);
	launch_per_item(morton_keys_kernel, n, s, m, ids, n, keys.p);
	// the keys' bits: 3 per level of the finest index (9 levels on a 512-wide
	// finest grid: 27 bits, 4 radix passes instead of 8)
	int b = 1;
	while (b < 21 && (uint64_t(1) << b) < std::max(m.glen[0], std::max(m.glen[1], m.glen[2]))) b++;
	const int end_bit = std::min(63, 3 * b);
	with_temp(cub_sort_pairs(keys.p, keys2.p, ids, ids2.p, n, end_bit, s));
	HIP_CHECK(hipMemcpyAsync(ids, ids2.p, n * 8, hipMemcpyDeviceToDevice, s));
	HIP_CHECK(hipStreamSynchronize(s));
}

// ids[0, run1) and ids[run1, n) each in Morton order -> ids in Morton order:
// one merge pass (rocprim::merge over the Morton keys) instead of a sort
void k_morton_merge2(const MapCtx& m, uint64_t* ids, size_t n, size_t run1, hipStream_t s) {
	if (run1 == 0 || run1 >= n) return;
	DBuf<uint64_t> keys, keys2, ids2;
	keys.alloc(n);
	keys2.alloc(n);
	ids2.alloc(n);
	launch_per_item(morton_keys_kernel, n, s, m, ids, n, keys.p);
	with_temp(prim_merge_pairs(keys.p, keys.p + run1, keys2.p, ids, ids + run1, ids2.p, run1, n - run1, s));
	HIP_CHECK(hipMemcpyAsync(ids, ids2.p, n * 8, hipMemcpyDeviceToDevice, s));
	HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace dccrgx
