// Device construction of the neighbor rows (replaces the reference's
// per-cell std::map walks: update_neighbors_ dccrg.hpp:9313-9458,
// find_neighbors_of 4339-4680, find_neighbors_to 4708-4861,
// update_remote_neighbor_info 8992-9095, update_cell_pointers 11314-11628,
// induce_refines 9591-9720): inner / outer flags, the neighbors_of and
// neighbors_to rows, the iterator lists, the neighbors a refine induces.
// One wavefront per cell; lanes own stencil items, and output positions come
// from a wave prefix scan or ballot + popcount: reference order, no atomics.
#include <cstdlib>

#include "dccrgx_internal.hpp"
#include "dccrgx_wave.hpp"

namespace dccrgx {

namespace {

constexpr int kMaxNtoLds = 8192;  // u64 entries of the neighbors_to dedupe (64 KB of LDS)

// --------------------------------------------------------------------------
// Pass 1: does a local cell have any remote neighbors_of / neighbors_to?
// (update_remote_neighbor_info 8992-9095).  One wave per cell.
__global__ void remote_flags_kernel(MapCtx m, const int32_t* hood, const int32_t* hood_to, int nh, DevMesh M, int rank,
                                    const uint64_t* cells, size_t n, uint32_t* flag) {
	const DevExists ex{M};
	const size_t waves = size_t(gridDim.x) * (blockDim.x / WAVE);
	for (size_t w = blockIdx.x * size_t(blockDim.x / WAVE) + threadIdx.x / WAVE; w < n; w += waves) {
		uint64_t c[3];
		int lvl;
		cell_coords(m, cells[w], c, lvl);
		bool remote = false;
		for (int k = lane_id(); k < nh; k += WAVE) {
			uint64_t w[3];
			const int kind = nof_item_case(m, c, lvl, hood + 3 * k, ex, w);
			for (int i = 0; i < item_count(kind); i++) {
				const int32_t ow = dm_owner(M, item_id(m, lvl, hood + 3 * k, kind, w, i, nullptr));
				if (ow >= 0 && ow != rank) remote = true;
			}
		}
		for (int k = lane_id(); k < 10 * nh; k += WAVE) {
			const uint64_t f = nto_candidate(m, c, lvl, hood_to, nh, k, ex);
			if (f != error_cell && dm_owner(M, f) != rank) remote = true;
		}
		const bool any = __any(remote);
		if (lane_id() == 0) flag[w] = any ? 1u : 0u;
	}
}

// The same classification with one thread per cell, for small hoods (the
// face hood: 6 neighbors_of items + 60 neighbors_to candidates per cell): a
// wave then holds 64 cells whose lookups are independent, where the wave per
// cell above issues its cell's 66 lookups as two dependent rounds and leaves
// 62 lanes idle in the second.  The walk stops at the first remote neighbor.
__global__ __launch_bounds__(256) void remote_flags_thread_kernel(MapCtx m, const int32_t* __restrict__ hood,
                                                                  const int32_t* __restrict__ hood_to, int nh,
                                                                  DevMesh M, int rank, const uint64_t* __restrict__ cells,
                                                                  size_t n, uint32_t* __restrict__ flag,
                                                                  const uint8_t* __restrict__ near, uint64_t near_lo,
                                                                  uint64_t near_n) {
	const DevExists ex{M};
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		if (near) {
			const uint64_t q = map_level0_parent(m, cells[i]) - near_lo;
			if (q < near_n && !near[q]) {
				flag[i] = 0u;
				continue;
			}
		}
		uint64_t c[3];
		int lvl;
		cell_coords(m, cells[i], c, lvl);
		bool remote = false;
		for (int k = 0; k < nh && !remote; k++) {
			uint64_t w[3];
			const int kind = nof_item_case(m, c, lvl, hood + 3 * k, ex, w);
			for (int j = 0; j < item_count(kind); j++) {
				const int32_t ow = dm_owner(M, item_id(m, lvl, hood + 3 * k, kind, w, j, nullptr));
				if (ow >= 0 && ow != rank) remote = true;
			}
		}
		for (int k = 0; k < 10 * nh && !remote; k++) {
			const uint64_t f = nto_candidate(m, c, lvl, hood_to, nh, k, ex);
			if (f != error_cell && dm_owner(M, f) != rank) remote = true;
		}
		flag[i] = remote ? 1u : 0u;
	}
}

}  // namespace

void k_remote_flags(const MapCtx& m, const int32_t* hood, const int32_t* hood_to, int nh, const DevMesh& M, int rank,
                    const uint64_t* cells, size_t n, uint32_t* flag, hipStream_t s, const uint8_t* near,
                    uint64_t near_lo, size_t near_n) {
	if (!n) return;
	static const char* env = std::getenv("DCCRGX_FLAGS_WAVE");  // A/B: the wave-per-cell form
	if ((nh <= 6 || near) && !(env && env[0] == '1'))
		remote_flags_thread_kernel<<<grid_for(n, 256), 256, 0, s>>>(m, hood, hood_to, nh, M, rank, cells, n, flag, near,
		                                                            near_lo, near_n);
	else
		remote_flags_kernel<<<grid_for(n, 4), 256, 0, s>>>(m, hood, hood_to, nh, M, rank, cells, n, flag);
	HIP_CHECK(hipGetLastError());
}

namespace {
// min / max level-0 parent of the ids: wave then block reduction, one
// atomic pair per block (per wave, 134 K pairs on one address cost 0.75 ms)
__global__ __launch_bounds__(256) void level0_span_kernel(MapCtx m, const uint64_t* __restrict__ ids, size_t n,
                                                          unsigned long long* mm) {
	__shared__ unsigned long long slo[256 / WAVE], shi[256 / WAVE];
	unsigned long long lo = ~0ull, hi = 0;
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const unsigned long long p = map_level0_parent(m, ids[i]);
		lo = p < lo ? p : lo;
		hi = p > hi ? p : hi;
	}
	for (int o = WAVE / 2; o > 0; o >>= 1) {
		const unsigned long long a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
		lo = a < lo ? a : lo;
		hi = b > hi ? b : hi;
	}
	if (lane_id() == 0) {
		slo[threadIdx.x / WAVE] = lo;
		shi[threadIdx.x / WAVE] = hi;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 256 / WAVE; w++) {
			lo = slo[w] < lo ? slo[w] : lo;
			hi = shi[w] > hi ? shi[w] : hi;
		}
		if (lo <= hi) {
			atomicMin(mm, lo);
			atomicMax(mm + 1, hi);
		}
	}
}

// mark the level-0 cells within r of every ghost leaf's level-0 parent
__global__ void level0_near_kernel(MapCtx m, MapCtx m0, const uint64_t* __restrict__ kid,
                                   const int32_t* __restrict__ kown, size_t n, int rank, int r, uint64_t lo,
                                   uint64_t span, uint8_t* __restrict__ near) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		if (kown[i] == rank) continue;
		uint64_t x, y, z;
		map_indices(m0, map_level0_parent(m, kid[i]), x, y, z);
		for (int dz = -r; dz <= r; dz++) {
			uint64_t wz;
			if (!map_wrap(m0, 2, int64_t(z) + dz, wz)) continue;
			for (int dy = -r; dy <= r; dy++) {
				uint64_t wy;
				if (!map_wrap(m0, 1, int64_t(y) + dy, wy)) continue;
				for (int dx = -r; dx <= r; dx++) {
					uint64_t wx;
					if (!map_wrap(m0, 0, int64_t(x) + dx, wx)) continue;
					const uint64_t q = map_from_indices(m0, wx, wy, wz, 0) - lo;
					if (q < span) near[q] = 1;
				}
			}
		}
	}
}
}  // namespace

bool k_level0_near(const MapCtx& m, const uint64_t* kid, const int32_t* kown, size_t n_known, int rank, int radius,
                   DBuf<uint8_t>& near, uint64_t& near_lo, hipStream_t s) {
	if (!n_known) return false;
	DBuf<unsigned long long> mm;
	mm.alloc(2);
	const unsigned long long init[2] = {~0ull, 0ull};
	h2d(mm.p, init, sizeof(init), s);
	level0_span_kernel<<<grid_for(n_known, 256, 1024), 256, 0, s>>>(m, kid, n_known, mm.p);
	HIP_CHECK(hipGetLastError());
	unsigned long long h[2] = {0, 0};
	d2h_small(h, mm.p, sizeof(h), s);
	if (h[0] > h[1]) return false;
	const uint64_t span = h[1] - h[0] + 1;
	if (span > 8 * uint64_t(n_known) + (uint64_t(1) << 24)) return false;
	near.alloc(size_t(span));
	HIP_CHECK(hipMemsetAsync(near.p, 0, size_t(span), s));
	MapCtx m0;
	const uint64_t len[3] = {m.len[0], m.len[1], m.len[2]};
	const int per[3] = {m.periodic[0], m.periodic[1], m.periodic[2]};
	map_init(m0, len, 0, per);
	launch_per_item(level0_near_kernel, n_known, s, m, m0, kid, kown, n_known, rank, radius, h[0], span, near.p);
	near_lo = h[0];
	return true;
}

namespace {
__global__ void assign_slots_kernel(const uint32_t* flag, const uint32_t* scan_outer, size_t n, size_t n_inner,
                                    const uint64_t* cells, uint64_t* slot_ids) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const size_t so = scan_outer[i];
		const size_t s = flag[i] ? n_inner + so : i - so;
		slot_ids[s] = cells[i];
	}
}

// --------------------------------------------------------------------------
// neighbors_to of one cell, sorted & deduplicated in LDS by the wave.
// Returns the unique count; when `out` is non-null, writes them ascending.
__device__ int nto_row(const MapCtx& m, const int32_t* hood_to, int nh, const DevExists& ex, const uint64_t c[3],
                       int lvl, uint64_t* lds, int cap, uint64_t* out) {
	int cnt = 0;
	const int seg_lo[3] = {0, nh, 9 * nh};
	const int seg_hi[3] = {nh, 9 * nh, 10 * nh};
	const bool seg_on[3] = {lvl > 0, lvl < m.R, true};
	for (int sgi = 0; sgi < 3; sgi++) {
		if (!seg_on[sgi]) continue;
		for (int k0 = seg_lo[sgi]; k0 < seg_hi[sgi]; k0 += WAVE) {
			const int k = k0 + lane_id();
			uint64_t f = error_cell;
			if (k < seg_hi[sgi]) f = nto_candidate(m, c, lvl, hood_to, nh, k, ex);
			const bool valid = f != error_cell;
			const uint64_t mask = __ballot(valid);
			const int pos = cnt + __popcll(mask & lanemask_lt());
			if (valid && pos < cap) lds[pos] = f;
			cnt += __popcll(mask);
		}
	}
	if (cnt > cap) cnt = cap;  // cap >= 10*nh (max_hood_items): never reached
	int P = 1;
	while (P < cnt) P <<= 1;
	for (int i = cnt + lane_id(); i < P; i += WAVE) lds[i] = ~0ull;
	__syncthreads();
	for (int k = 2; k <= P; k <<= 1) {
		for (int j = k >> 1; j > 0; j >>= 1) {
			for (int i = lane_id(); i < P; i += WAVE) {
				const int ixj = i ^ j;
				if (ixj > i) {
					const uint64_t a = lds[i], b = lds[ixj];
					const bool up = (i & k) == 0;
					if ((a > b) == up) {
						lds[i] = b;
						lds[ixj] = a;
					}
				}
			}
			__syncthreads();
		}
	}
	int base = 0;
	for (int i0 = 0; i0 < cnt; i0 += WAVE) {
		const int i = i0 + lane_id();
		const bool u = i < cnt && (i == 0 || lds[i] != lds[i - 1]);
		const uint64_t mask = __ballot(u);
		if (out && u) out[base + __popcll(mask & lanemask_lt())] = lds[i];
		base += __popcll(mask);
	}
	__syncthreads();
	return base;
}

// per-row counts in slot order (one wave = one block per row)
__global__ void count_rows_kernel(MapCtx m, const int32_t* hood, const int32_t* hood_to, int nh, DevMesh M,
                                  const uint64_t* slot_ids, size_t row0, size_t nrows, uint32_t* nof_cnt,
                                  uint32_t* nto_cnt, int cap) {
	extern __shared__ uint64_t lds[];
	const DevExists ex{M};
	for (size_t r = blockIdx.x; r < nrows; r += gridDim.x) {
		uint64_t c[3];
		int lvl;
		cell_coords(m, slot_ids[row0 + r], c, lvl);
		int n = 0;
		for (int k = lane_id(); k < nh; k += WAVE) {
			uint64_t w[3];
			n += item_count(nof_item_case(m, c, lvl, hood + 3 * k, ex, w));
		}
		n = wave_sum(n);
		const int t = nto_row(m, hood_to, nh, ex, c, lvl, lds, cap, nullptr);
		if (lane_id() == 0) {
			nof_cnt[r] = uint32_t(n);
			nto_cnt[r] = uint32_t(t);
		}
	}
}

// neighbors_of rows in stencil order (4339-4680 semantics, see dccrgx_neighbors.hpp)
__global__ void fill_nof_kernel(MapCtx m, const int32_t* hood, int nh, DevMesh M, const uint64_t* slot_ids, size_t row0,
                                size_t nrows, const uint32_t* ptr, uint64_t* ids, int32_t* offs) {
	const DevExists ex{M};
	const size_t waves = size_t(gridDim.x) * (blockDim.x / WAVE);
	for (size_t r = blockIdx.x * size_t(blockDim.x / WAVE) + threadIdx.x / WAVE; r < nrows; r += waves) {
		uint64_t c[3];
		int lvl;
		cell_coords(m, slot_ids[row0 + r], c, lvl);
		size_t base = ptr[r];
		for (int k0 = 0; k0 < nh; k0 += WAVE) {
			const int k = k0 + lane_id();
			uint64_t w[3] = {0, 0, 0};
			const int kind = k < nh ? nof_item_case(m, c, lvl, hood + 3 * k, ex, w) : 0;
			const int no = item_count(kind);
			const int incl = wave_incl_scan(no);
			const size_t pos = base + size_t(incl - no);
			for (int i = 0; i < no; i++) {
				int32_t off[3];
				ids[pos + i] = item_id(m, lvl, hood + 3 * k, kind, w, i, off);
				offs[3 * (pos + i) + 0] = off[0];
				offs[3 * (pos + i) + 1] = off[1];
				offs[3 * (pos + i) + 2] = off[2];
			}
			base += size_t(__shfl(incl, WAVE - 1, WAVE));
		}
	}
}

__global__ void fill_nto_kernel(MapCtx m, const int32_t* hood_to, int nh, DevMesh M, const uint64_t* slot_ids,
                                size_t row0, size_t nrows, const uint32_t* ptr, uint64_t* ids, int cap) {
	extern __shared__ uint64_t lds[];
	const DevExists ex{M};
	for (size_t r = blockIdx.x; r < nrows; r += gridDim.x) {
		uint64_t c[3];
		int lvl;
		cell_coords(m, slot_ids[row0 + r], c, lvl);
		nto_row(m, hood_to, nh, ex, c, lvl, lds, cap, ids + ptr[r]);
	}
}
}  // namespace

void k_assign_slots2(const uint32_t* flag, const uint32_t* scan_outer, size_t n, size_t n_inner, const uint64_t* cells,
                     uint64_t* slot_ids, hipStream_t s) {
	launch_per_item(assign_slots_kernel, n, s, flag, scan_outer, n, n_inner, cells, slot_ids);
}

int max_hood_items() { return kMaxNtoLds / 10; }

static int nto_cap(int nh) {
	int P = 1;
	while (P < 10 * nh) P <<= 1;
	DX_REQUIRE(P <= kMaxNtoLds, "neighborhood too large for the neighbors_to build");
	return P;
}

void k_count_rows(const MapCtx& m, const int32_t* hood, const int32_t* hood_to, int nh, const DevMesh& M,
                  const uint64_t* slot_ids, size_t row0, size_t nrows, uint32_t* nof_cnt, uint32_t* nto_cnt,
                  hipStream_t s) {
	if (!nrows) return;
	const int cap = nto_cap(nh);
	count_rows_kernel<<<grid_for(nrows, 1, 256u * 64u), WAVE, size_t(cap) * 8, s>>>(m, hood, hood_to, nh, M, slot_ids,
	                                                                                  row0, nrows, nof_cnt, nto_cnt, cap);
	HIP_CHECK(hipGetLastError());
}

void k_fill_neighbors_of(const MapCtx& m, const int32_t* hood, int nh, const DevMesh& M, const uint64_t* slot_ids,
                         size_t row0, size_t nrows, const uint32_t* ptr, uint64_t* ids, int32_t* offs, hipStream_t s) {
	if (!nrows) return;
	fill_nof_kernel<<<grid_for(nrows, 4), 256, 0, s>>>(m, hood, nh, M, slot_ids, row0, nrows, ptr, ids, offs);
	HIP_CHECK(hipGetLastError());
}

void k_fill_neighbors_to(const MapCtx& m, const int32_t* hood_to, int nh, const DevMesh& M, const uint64_t* slot_ids,
                         size_t row0, size_t nrows, const uint32_t* ptr, uint64_t* ids, hipStream_t s) {
	if (!nrows) return;
	const int cap = nto_cap(nh);
	fill_nto_kernel<<<grid_for(nrows, 1, 256u * 64u), WAVE, size_t(cap) * 8, s>>>(m, hood_to, nh, M, slot_ids, row0,
	                                                                                nrows, ptr, ids, cap);
	HIP_CHECK(hipGetLastError());
}

namespace {
// (id, offset) order of std::set<pair<uint64_t, array<int, 3>>>
__device__ __forceinline__ bool key_less(uint64_t ia, const int32_t* oa, uint64_t ib, const int32_t* ob) {
	if (ia != ib) return ia < ib;
	if (oa[0] != ob[0]) return oa[0] < ob[0];
	if (oa[1] != ob[1]) return oa[1] < ob[1];
	return oa[2] < ob[2];
}

// iterator neighbor range cell.neighbors_of (update_cell_pointers
// 11451-11500): the distinct (id, offset) pairs of the row, the ones whose id
// is not in the row's neighbors_to first ("only_of"), then the ones whose id
// is ("both"), each class in (id, offset) order.  One wave per row, one lane
// per entry; the loops over the row's other entries are wave-uniform, so
// every lane reads the same entry (one broadcast load).
// Pass 0 classifies every entry (0 repeat of an earlier pair, 1 only_of,
// 2 both) and counts the distinct pairs; pass 1 places each entry at its
// rank within its class.
__device__ __forceinline__ bool same_pair(const uint64_t* id, const int32_t* off, uint32_t i, uint32_t j) {
	return id[i] == id[j] && off[3 * i] == off[3 * j] && off[3 * i + 1] == off[3 * j + 1] &&
	       off[3 * i + 2] == off[3 * j + 2];
}

__global__ void iterator_class_kernel(const uint32_t* nof_ptr, const uint64_t* nof_id, const int32_t* nof_off,
                                      const uint32_t* nto_ptr, const uint64_t* nto_id, size_t nrows, uint8_t* cls,
                                      uint32_t* it_cnt) {
	const size_t waves = size_t(gridDim.x) * (blockDim.x / WAVE);
	for (size_t r = blockIdx.x * size_t(blockDim.x / WAVE) + threadIdx.x / WAVE; r < nrows; r += waves) {
		const uint32_t b = nof_ptr[r], e = nof_ptr[r + 1];
		const uint32_t tb = nto_ptr[r], te = nto_ptr[r + 1];
		uint32_t n_all = 0;
		for (uint32_t j0 = b; j0 < e; j0 += WAVE) {
			const uint32_t j = j0 + lane_id();
			uint8_t c = 0;
			if (j < e) {
				bool dup = false;
				for (uint32_t i = b; i < j && !dup; i++) dup = same_pair(nof_id, nof_off, i, j);
				if (!dup) {
					const uint64_t id = nof_id[j];
					uint32_t lo = tb, hi = te;
					while (lo < hi) {
						const uint32_t mid = (lo + hi) >> 1;
						if (nto_id[mid] < id) lo = mid + 1;
						else hi = mid;
					}
					c = (lo < te && nto_id[lo] == id) ? 2 : 1;
				}
				cls[j] = c;
			}
			n_all += uint32_t(__popcll(__ballot(c != 0)));
		}
		if (lane_id() == 0) it_cnt[r] = n_all;
	}
}

__global__ void iterator_fill_kernel(const uint32_t* nof_ptr, const uint64_t* nof_id, const int32_t* nof_off,
                                     const int32_t* nof_slot, const uint8_t* cls, size_t nrows, const uint32_t* it_ptr,
                                     int32_t* it_slot, int32_t* it_off) {
	const size_t waves = size_t(gridDim.x) * (blockDim.x / WAVE);
	for (size_t r = blockIdx.x * size_t(blockDim.x / WAVE) + threadIdx.x / WAVE; r < nrows; r += waves) {
		const uint32_t b = nof_ptr[r], e = nof_ptr[r + 1];
		uint32_t n_only = 0;
		for (uint32_t j0 = b; j0 < e; j0 += WAVE) {
			const uint32_t j = j0 + lane_id();
			n_only += uint32_t(__popcll(__ballot(j < e && cls[j] == 1)));
		}
		for (uint32_t j0 = b; j0 < e; j0 += WAVE) {
			const uint32_t j = j0 + lane_id();
			const uint8_t cj = j < e ? cls[j] : 0;
			uint32_t rank = 0;
			for (uint32_t i = b; i < e; i++)
				if (cj != 0 && cls[i] == cj && key_less(nof_id[i], nof_off + 3 * i, nof_id[j], nof_off + 3 * j)) rank++;
			if (cj == 0) continue;
			const uint32_t pos = it_ptr[r] + (cj == 2 ? n_only : 0u) + rank;
			it_slot[pos] = nof_slot[j];
			if (it_off) {
				it_off[3 * pos] = nof_off[3 * j];
				it_off[3 * pos + 1] = nof_off[3 * j + 1];
				it_off[3 * pos + 2] = nof_off[3 * j + 2];
			}
		}
	}
}
}  // namespace

void k_iterator_lists(const uint32_t* nof_ptr, const uint64_t* nof_id, const int32_t* nof_off,
                      const int32_t* nof_slot, const uint32_t* nto_ptr, const uint64_t* nto_id, size_t nrows,
                      uint8_t* cls, uint32_t* it_cnt, const uint32_t* it_ptr, int32_t* it_slot, int32_t* it_off,
                      int pass, hipStream_t s) {
	if (!nrows) return;
	if (pass == 0)
		iterator_class_kernel<<<grid_for(nrows, 4), 256, 0, s>>>(nof_ptr, nof_id, nof_off, nto_ptr, nto_id, nrows, cls,
		                                                         it_cnt);
	else
		iterator_fill_kernel<<<grid_for(nrows, 4), 256, 0, s>>>(nof_ptr, nof_id, nof_off, nof_slot, cls, nrows, it_ptr,
		                                                        it_slot, it_off);
	HIP_CHECK(hipGetLastError());
}

namespace {
// induce_refines (9591-9720): for a requested local cell r, every existing
// neighbors_of / neighbors_to entry coarser than r must be refined as well
// neighbors_of / neighbors_to of the local cells of req that are coarser
// (induce_refines 9591-9720) or, with finer != 0, finer (the dont_refine
// spread of override_refines 9991-10038) than the cell
__global__ void induced_kernel(MapCtx m, const int32_t* hood, const int32_t* hood_to, int nh, DevMesh M, int rank,
                               const uint64_t* req, size_t n, uint64_t* out, unsigned long long* counter,
                               unsigned long long cap, int finer) {
	const DevExists ex{M};
	const size_t waves = size_t(gridDim.x) * (blockDim.x / WAVE);
	for (size_t w = blockIdx.x * size_t(blockDim.x / WAVE) + threadIdx.x / WAVE; w < n; w += waves) {
		const uint64_t r = req[w];
		if (dm_owner(M, r) != rank) continue;  // wave-uniform
		uint64_t c[3];
		int lvl;
		cell_coords(m, r, c, lvl);
		auto emit = [&](uint64_t q) {
			if (q == error_cell || !ex(q)) return;
			const int ql = map_level(m, q);
			if (finer ? ql <= lvl : ql >= lvl) return;
			const unsigned long long pos = atomicAdd(counter, 1ull);
			if (pos < cap) out[pos] = q;
		};
		// nof_item's leaves from the item's case (no ItemOut in private memory)
		for (int k = lane_id(); k < nh; k += WAVE) {
			uint64_t w[3];
			const int kind = nof_item_case(m, c, lvl, hood + 3 * k, ex, w);
			for (int i = 0; i < item_count(kind); i++) emit(item_id(m, lvl, hood + 3 * k, kind, w, i, nullptr));
		}
		for (int k = lane_id(); k < 10 * nh; k += WAVE) emit(nto_candidate(m, c, lvl, hood_to, nh, k, ex));
	}
}
}  // namespace

std::vector<uint64_t> k_induced_refines(const MapCtx& m, const int32_t* hood, const int32_t* hood_to, int nh,
                                        const DevMesh& M, int rank, const std::vector<uint64_t>& req, hipStream_t s,
                                        bool finer, const uint64_t* dreq_given) {
	if (req.empty()) return {};
	DBuf<uint64_t> dreq_own;
	const uint64_t* dreq = given_or_upload(dreq_given, req, dreq_own, s);
	return collect_sorted_unique(req.size() * 16 + 1024, map_id_bits(m), s,
	                             [&](uint64_t* out, unsigned long long* ctr, unsigned long long cap) {
		                             induced_kernel<<<grid_for(req.size(), 4), 256, 0, s>>>(
		                                 m, hood, hood_to, nh, M, rank, dreq, req.size(), out, ctr, cap, finer ? 1 : 0);
	                             });
}

}  // namespace dccrgx
