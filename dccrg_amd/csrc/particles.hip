// Particles in cells (tests/particles/simple.cpp): a variable field of fp64
// records (K doubles each, doubles 0..2 the position) is pushed, wrapped
// through the periodic geometry, located (get_existing_cell(coordinate),
// dccrg.hpp:6316-6336) and re-binned into the cells' lists on the device.
//
// One __device__ function does the point location, a literal restatement of
// Cartesian_Geometry::get_real_coordinate / get_indices(coordinate)
// (dccrg_cartesian_geometry.hpp:521-607) and the finest-first probe of
// get_existing_cell(indices, 0, R) (dccrg.hpp:11275-11308); the batch query
// and the particle step both call it.  Under a stretched geometry
// (dccrgx_set_stretched_geometry) a second one restates
// Stretched_Cartesian_Geometry::get_real_coordinate / get_indices
// (dccrg_stretched_cartesian_geometry.hpp:504-607) with the reference's two
// linear scans replaced by a binary search and a corrected quotient that give
// the same indices; the Cartesian kernels are instantiated without it.
//
// The step (DESIGN.md "Particles"):
//   1. locate  - a thread per particle: source slot (search of the record
//                offsets, narrowed per block), x' = real(x + v dt) stored
//                back, destination slot, stay / mover flags, statistics;
//   2. two exclusive scans (stayers, movers) in one pass of temp storage;
//   3. movers compacted to (destination slot, rank of the source id | index)
//                keys and sorted by one stable radix sort;
//   4. arrivals per destination from the run boundaries of the sorted keys;
//   5. a scan of the new record counts;
//   6. scatter - stayers and movers into a fresh pool, swapped in.
// No atomic decides a position: a cell's records are its stayers in their
// previous order, then the arrivals ordered by (source cell id, index in the
// source cell).

#include <cmath>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "dccrgx_grid.hpp"
#include "dccrgx_philox.hpp"
#include "dccrgx_reduce.hpp"

// x + v dt, x +- L ceil(d / L) and (x - start) / l are separately rounded
// operations in the reference; hipcc fuses a * b + c by default
#pragma clang fp contract(off)

namespace dccrgx {

namespace {

// Cartesian geometry of the whole grid: start, end (get_end: start + double(
// length) * l0, formed on the host), the finest cell's length l0 / 2^R
struct PGeo {
	double start[3], end[3], cell[3];
	int per[3];
};

PGeo make_geo(const Grid& g) {
	PGeo G;
	for (int d = 0; d < 3; d++) {
		G.start[d] = g.start[d];
		const double span = double(g.len[d]) * g.l0[d];
		G.end[d] = g.start[d] + span;
		G.cell[d] = g.l0[d] / double(uint64_t(1) << g.R);
		G.per[d] = g.per[d];
	}
	return G;
}

// get_real_coordinate of one dimension (dccrg_cartesian_geometry.hpp:534-561)
__device__ __forceinline__ double real_coordinate(const PGeo& G, int d, double x) {
	const double start = G.start[d], end = G.end[d];
	if (x >= start && x <= end) return x;
	if (!G.per[d]) return __longlong_as_double(0x7ff8000000000000ll);
	const double L = end - start;
	if (x < start) {
		const double distance = start - x;
		const double q = distance / L;
		const double w = L * ceil(q);
		return x + w;
	}
	const double distance = x - end;
	const double q = distance / L;
	const double w = L * ceil(q);
	return x - w;
}

// dm_owner(M, id) >= 0 without the owner (an implicit mesh: no division)
__device__ __forceinline__ bool known_leaf(const DevMesh& M, uint64_t id) {
	if (id == error_cell || id > M.last) return false;
	if (M.implicit) return id <= M.bp.n0;
	int32_t o, s;
	return dm_lookup(M, id, o, s);
}

// the smallest leaf this process knows at x (error_cell: outside the grid,
// or nothing known there); get_indices wraps the coordinate once more, as
// the reference does
__device__ __forceinline__ uint64_t existing_cell_at(const MapCtx& m, const DevMesh& M, const PGeo& G,
                                                     const double x[3]) {
	uint64_t ind[3];
#pragma unroll
	for (int d = 0; d < 3; d++) {
		const double c = real_coordinate(G, d, x[d]);
		if (!(c >= G.start[d] && c <= G.end[d])) return error_cell;
		const double rel = c - G.start[d];
		const double q = rel / G.cell[d];
		ind[d] = uint64_t(floor(q));
		// a coordinate at the grid's end is inside for the wrap but indexes one
		// past the last cell (get_existing_cell(indices), dccrg.hpp:11280-11290)
		if (ind[d] >= m.glen[d]) return error_cell;
	}
	for (int lvl = m.R; lvl >= 0; lvl--) {
		const uint64_t id = map_from_indices(m, ind[0], ind[1], ind[2], lvl);
		if (known_leaf(M, id)) return id;
	}
	return error_cell;
}

// Stretched_Cartesian_Geometry (Grid::str): the packed level-0 boundaries of
// the three dimensions (dimension d at c + off[d], n[d] of them); g holds
// start = c[0], end = c[n - 1] and the periodicity, l0 = 2^R
struct SGeo {
	PGeo g;
	const double* c;
	uint32_t off[3], n[3];
	uint32_t total;
	double l0;
};

// the three coordinate lists are searched in LDS when together they are at
// most this many doubles (12 KiB: with the 4 KiB of record offsets a block of
// the locate kernel stays at 16 KiB, eight blocks a CU as before), else in
// global memory
constexpr uint32_t kCoordCache = 1536;

// get_indices of one dimension (dccrg_stretched_cartesian_geometry.hpp:575-602)
// for a coordinate inside [c[0], c[n - 1]].  The level-0 cell: the reference
// scans for the first boundary >= x and steps one back (a boundary belongs to
// the cell below it; x == c[0] to cell 0, the facade's host get_indices).  The
// offset inside it: the reference counts k up while c0 + k * li < x; the sum
// never decreases with k, so floor((x - c0) / li) corrected by that predicate
// is the same k.  li resolves at both ends of the cell (stretched_device
// checks it), so each loop runs a step or two.
__device__ __forceinline__ uint64_t stretched_index(const double* c, uint32_t n, double l0, double x) {
	uint32_t lo = 0, hi = n - 1;  // c[n - 1] >= x
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (c[mid] >= x)
			hi = mid;
		else
			lo = mid + 1;
	}
	const uint32_t i0 = lo == 0 ? 0 : lo - 1;
	const double c0 = c[i0];
	const double extent = c[i0 + 1] - c0;
	const double li = extent / l0;
	const double rel = x - c0;
	const double q = rel / li;
	uint64_t k = uint64_t(floor(q));
	while (true) {
		const double w = double(k) * li;
		if (!(c0 + w < x)) break;
		k++;
	}
	while (k > 0) {
		const double w = double(k - 1) * li;
		if (!(c0 + w >= x)) break;
		k--;
	}
	return uint64_t(i0) * uint64_t(l0) + (k == 0 ? 0 : k - 1);
}

// existing_cell_at under the stretched geometry; c: the packed coordinates
// (S.c, or a block's copy in LDS)
__device__ __forceinline__ uint64_t stretched_cell_at(const MapCtx& m, const DevMesh& M, const SGeo& S,
                                                      const double* c, const double x[3]) {
	uint64_t ind[3];
#pragma unroll
	for (int d = 0; d < 3; d++) {
		const double r = real_coordinate(S.g, d, x[d]);
		if (!(r >= S.g.start[d] && r <= S.g.end[d])) return error_cell;
		ind[d] = stretched_index(c + S.off[d], S.n[d], S.l0, r);
		// the reference's rounding quirk: a point at a level-0 cell's upper
		// boundary may index the next cell's first index, in the last cell one
		// past the grid (get_existing_cell(indices), dccrg.hpp:11280-11290)
		if (ind[d] >= m.glen[d]) return error_cell;
	}
	for (int lvl = m.R; lvl >= 0; lvl--) {
		const uint64_t id = map_from_indices(m, ind[0], ind[1], ind[2], lvl);
		if (known_leaf(M, id)) return id;
	}
	return error_cell;
}

// The point location of a kernel, Geo: PGeo (Cartesian) or SGeo (stretched).
// stage_geometry is the kernel's preamble: a block's copy of a stretched
// geometry's coordinates in LDS (the caller syncs before the first cell_at);
// false: they do not fit, or the geometry has none.  cell_at is the smallest
// known leaf at x under either geometry.
template <class Geo>
__device__ __forceinline__ bool stage_geometry(const Geo& G, const double*& s_c) {
	s_c = nullptr;
	if constexpr (std::is_same<Geo, SGeo>::value) {
		__shared__ double s_coords[kCoordCache];
		s_c = s_coords;
		if (G.total > kCoordCache) return false;
		for (uint32_t i = threadIdx.x; i < G.total; i += blockDim.x) s_coords[i] = G.c[i];
		return true;
	}
	return false;
}

__device__ __forceinline__ uint64_t cell_at(const MapCtx& m, const DevMesh& M, const PGeo& G, const double*, bool,
                                            const double x[3]) {
	return existing_cell_at(m, M, G, x);
}

__device__ __forceinline__ uint64_t cell_at(const MapCtx& m, const DevMesh& M, const SGeo& S, const double* s_c,
                                            bool cached, const double x[3]) {
	return cached ? stretched_cell_at(m, M, S, s_c, x) : stretched_cell_at(m, M, S, S.c, x);
}

template <class Geo>
__global__ void cells_at_kernel(const MapCtx m, const DevMesh M, const Geo G, const double* __restrict__ xyz, size_t n,
                                uint64_t* __restrict__ ids) {
	const double* s_c;
	const bool cached = stage_geometry(G, s_c);
	if (s_c) __syncthreads();  // (nothing is staged under PGeo)
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const double x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
		ids[i] = cell_at(m, M, G, s_c, cached, x);
	}
}

constexpr int kPB = 256;         // particles per block pass
constexpr int kOffCache = 1024;  // record offsets of a block's slots kept in LDS

// first index in [lo, hi) with a[i] > v
template <class T>
__device__ __forceinline__ size_t upper_bound_idx(const T* a, size_t lo, size_t hi, T v) {
	while (lo < hi) {
		const size_t mid = lo + (hi - lo) / 2;
		if (a[mid] > v)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}

// byte offsets -> record offsets; flag: an offset that is no whole record
__global__ void record_offsets_kernel(const uint64_t* __restrict__ voff, size_t n, uint64_t rec,
                                      uint32_t* __restrict__ ofirst, int32_t* __restrict__ flag) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t q = voff[i] / rec;
		if (q * rec != voff[i]) *flag = 1;
		ofirst[i] = uint32_t(q);
	}
}

// The record search (DESIGN.md "Passes of one step"): the slot of record p is
// the last one whose offset is <= p.  A side table narrows it per block pass,
// and the offsets between the pass's first and last slot are searched in LDS
// when they fit kOffCache, else in global memory.
//
// slot of the first record of every block pass (and, last entry, of the last
// record of all N).  A pass is kPB records, or (kDoubles) kPB doubles of records
// of K: i * kPB / K records lie before pass i (the step's and the gather's
// table pays for no division)
template <bool kDoubles>
__global__ void pass_slots_kernel(const uint32_t* __restrict__ off, size_t n_slots, size_t N, size_t passes, size_t K,
                                  uint32_t* __restrict__ pass_slot) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i <= passes; i += size_t(gridDim.x) * blockDim.x) {
		const size_t p = i == passes ? N - 1 : kDoubles ? (i * kPB) / K : i * kPB;
		pass_slot[i] = uint32_t(upper_bound_idx<uint32_t>(off, 0, n_slots + 1, uint32_t(p)) - 1);
	}
}

// K: 0 for passes of records
void launch_pass_slots(const uint32_t* off, size_t n_slots, size_t N, size_t passes, size_t K, DBuf<uint32_t>& pass_slot,
                       hipStream_t s) {
	pass_slot.alloc(passes + 1);
	if (K)
		pass_slots_kernel<true><<<grid_for(passes + 1, 256), 256, 0, s>>>(off, n_slots, N, passes, K, pass_slot.p);
	else
		pass_slots_kernel<false><<<grid_for(passes + 1, 256), 256, 0, s>>>(off, n_slots, N, passes, 1, pass_slot.p);
	HIP_CHECK(hipGetLastError());
}

// a block pass's window of the offsets, off[lo .. hi + 1]
struct OffsetWindow {
	const uint32_t *off, *s_off;  // all offsets; the block's copy of the window (if cached)
	size_t lo, hi;                // the slots of the pass's first and last record bound every search
	bool cached;

	__device__ __forceinline__ size_t slot(uint32_t p) const {
		return cached ? lo + upper_bound_idx<uint32_t>(s_off, 0, hi - lo + 2, p) - 1
		              : upper_bound_idx<uint32_t>(off, lo, hi + 2, p) - 1;
	}
	// off[s] of a slot of the window, read where the search read
	__device__ __forceinline__ uint32_t at(size_t s) const { return cached ? s_off[s - lo] : off[s]; }
};

// every thread of a block of kPB calls this once per pass (two barriers: the
// previous pass's searches end before the copy, the copy before this pass's)
__device__ __forceinline__ OffsetWindow stage_offsets(const uint32_t* off, const uint32_t* pass_slot, size_t pass,
                                                      uint32_t* s_off) {
	__syncthreads();
	OffsetWindow W{off, s_off, pass_slot[pass], pass_slot[pass + 1], false};
	const size_t span = W.hi - W.lo + 2;
	W.cached = span <= size_t(kOffCache);
	if (W.cached)
		for (size_t i = threadIdx.x; i < span; i += kPB) s_off[i] = off[W.lo + i];
	__syncthreads();
	return W;
}

// (the mapping, the mesh and the geometry are kernel parameters of their own:
// inside one struct their lane-uniform array reads put the struct in scratch)
struct PArgs {
	double* pool;
	const uint32_t* ofirst;      // n_slots + 1 record offsets
	const uint32_t* chunk_slot;  // chunks + 1 (pass_slots_kernel)
	size_t n_slots, n_local, N;
	int K;
	const uint64_t* slot_ids;
	const uint32_t *nof_ptr, *nto_ptr;
	const uint64_t *nof_id, *nto_id;
	const int32_t* nof_slot;
	double vel[3];
	int has_vel;
	double dt;
	int32_t *src, *dest;      // per particle: source slot, destination slot (-1: leaves the lists)
	uint32_t *stay, *mover;   // per particle flags (N + 1 entries, scanned)
	uint32_t* part;           // per block: moved, arrived, handed over, lost
};

__device__ __forceinline__ const PGeo& wrap_geo(const PGeo& G) { return G; }
__device__ __forceinline__ const PGeo& wrap_geo(const SGeo& S) { return S.g; }

template <class Geo>
__global__ __launch_bounds__(kPB) void particles_locate_kernel(const MapCtx m, const DevMesh M, const Geo G,
                                                                  const PArgs a) {
	__shared__ uint32_t s_off[kOffCache];
	__shared__ uint32_t s_cnt[4];
	const double* s_c;
	const bool coords_cached = stage_geometry(G, s_c);  // synced by the first pass below
	uint32_t n_moved = 0, n_arrived = 0, n_handed = 0, n_lost = 0;
	if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
	const size_t chunks = (a.N + kPB - 1) / kPB;
	for (size_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
		const size_t p0 = ch * kPB, p1 = p0 + kPB < a.N ? p0 + kPB : a.N;
		const OffsetWindow W = stage_offsets(a.ofirst, a.chunk_slot, ch, s_off);
		const size_t p = p0 + threadIdx.x;
		if (p >= p1) continue;
		const size_t s = W.slot(uint32_t(p));
		double* r = a.pool + p * size_t(a.K);
		double x[3];
#pragma unroll
		for (int d = 0; d < 3; d++) {
			const double v = a.has_vel ? a.vel[d] : r[3 + d];
			const double step = v * a.dt;
			const double moved = r[d] + step;
			x[d] = real_coordinate(wrap_geo(G), d, moved);
			r[d] = x[d];
		}
		const uint64_t dst = cell_at(m, M, G, s_c, coords_cached, x);
		const uint64_t own = a.slot_ids[s];
		const bool local = s < a.n_local;
		int32_t dest = -1;
		uint32_t stay = 0;
		if (local) {
			if (dst == own) {
				dest = int32_t(s);
				stay = 1;
			} else {
				bool found = false;  // not found: lost (error_cell, or not in neighbors_of)
				if (dst != error_cell) {
					const uint32_t e1 = a.nof_ptr[s + 1];
					for (uint32_t e = a.nof_ptr[s]; e < e1; e++) {
						if (a.nof_id[e] != dst) continue;
						const int32_t ds = a.nof_slot[e];
						found = true;
						if (ds >= 0 && size_t(ds) < a.n_local) {
							dest = ds;  // moved between local cells
							n_moved++;
						} else {
							n_handed++;  // handed over to the owner of a known remote cell
						}
						break;
					}
				}
				if (!found) n_lost++;
			}
		} else if (dst != error_cell && dst != own) {
			// a copy of a remote neighbor: its particle arrives when the copy is
			// in neighbors_to of a local destination
			const int32_t ds = dm_slot(M, dst);
			if (ds >= 0 && size_t(ds) < a.n_local) {
				for (uint32_t e = a.nto_ptr[ds]; e < a.nto_ptr[ds + 1]; e++) {
					if (a.nto_id[e] != own) continue;
					dest = ds;
					n_arrived++;
					break;
				}
			}
		}
		a.src[p] = int32_t(s);
		a.dest[p] = dest;
		a.stay[p] = stay;
		a.mover[p] = (dest >= 0 && !stay) ? 1u : 0u;
	}
	__syncthreads();
	if (n_moved) atomicAdd(&s_cnt[0], n_moved);
	if (n_arrived) atomicAdd(&s_cnt[1], n_arrived);
	if (n_handed) atomicAdd(&s_cnt[2], n_handed);
	if (n_lost) atomicAdd(&s_cnt[3], n_lost);
	__syncthreads();
	if (threadIdx.x < 4) a.part[4 * size_t(blockIdx.x) + threadIdx.x] = s_cnt[threadIdx.x];
}

__global__ void sum_parts_kernel(const uint32_t* __restrict__ part, size_t nb, uint64_t* __restrict__ out) {
	__shared__ unsigned long long s[4];
	if (threadIdx.x < 4) s[threadIdx.x] = 0;
	__syncthreads();
	unsigned long long c[4] = {0, 0, 0, 0};
	for (size_t i = threadIdx.x; i < nb; i += blockDim.x)
		for (int k = 0; k < 4; k++) c[k] += part[4 * i + k];
	for (int k = 0; k < 4; k++)
		if (c[k]) atomicAdd(&s[k], c[k]);
	__syncthreads();
	if (threadIdx.x < 4) out[threadIdx.x] = s[threadIdx.x];
}

__global__ void rank_by_id_kernel(const int32_t* __restrict__ order, size_t n, uint32_t* __restrict__ idrank) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		idrank[order[i]] = uint32_t(i);
}

// movers in particle order: key = destination slot << bits | rank of the
// source cell's id, value = the particle (a stable sort keeps the index order
// inside one source cell)
__global__ void mover_keys_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ dest,
                                  const uint32_t* __restrict__ mover, const uint32_t* __restrict__ mpos, size_t N,
                                  const uint32_t* __restrict__ idrank, int bits, uint64_t* __restrict__ keys,
                                  uint32_t* __restrict__ vals) {
	for (size_t p = blockIdx.x * size_t(blockDim.x) + threadIdx.x; p < N; p += size_t(gridDim.x) * blockDim.x) {
		if (!mover[p]) continue;
		const uint32_t k = mpos[p];
		keys[k] = (uint64_t(uint32_t(dest[p])) << bits) | idrank[src[p]];
		vals[k] = uint32_t(p);
	}
}

// first / one-past-last sorted mover of every destination slot
__global__ void arrival_runs_kernel(const uint64_t* __restrict__ keys, size_t M, int bits,
                                    uint32_t* __restrict__ arr_first, uint32_t* __restrict__ arr_end) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < M; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t ds = keys[i] >> bits;
		if (i == 0 || (keys[i - 1] >> bits) != ds) arr_first[ds] = uint32_t(i);
		if (i + 1 == M || (keys[i + 1] >> bits) != ds) arr_end[ds] = uint32_t(i + 1);
	}
}

// new record count of every slot: stayers + arrivals of a local cell, none of a remote copy
__global__ void new_counts_kernel(const uint32_t* __restrict__ ofirst, const uint32_t* __restrict__ stayrank,
                                  const uint32_t* __restrict__ arr_first, const uint32_t* __restrict__ arr_end,
                                  size_t n_slots, size_t n_local, uint32_t* __restrict__ staycnt,
                                  uint32_t* __restrict__ newcnt) {
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n_slots; s += size_t(gridDim.x) * blockDim.x) {
		uint32_t st = 0, nw = 0;
		if (s < n_local) {
			st = stayrank[ofirst[s + 1]] - stayrank[ofirst[s]];
			nw = st + (arr_end[s] - arr_first[s]);
		}
		staycnt[s] = st;
		newcnt[s] = nw;
	}
}

__global__ void byte_offsets_kernel(const uint32_t* __restrict__ nfirst, size_t n, uint64_t rec,
                                    uint64_t* __restrict__ noff) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		noff[i] = uint64_t(nfirst[i]) * rec;
}

__device__ __forceinline__ void copy_record(double* __restrict__ dst, const double* __restrict__ src, int K) {
	for (int k = 0; k < K; k++) dst[k] = src[k];
}

__global__ void scatter_stayers_kernel(const double* __restrict__ pool, double* __restrict__ out, int K, size_t N,
                                       const int32_t* __restrict__ src, const uint32_t* __restrict__ stay,
                                       const uint32_t* __restrict__ stayrank, const uint32_t* __restrict__ ofirst,
                                       const uint32_t* __restrict__ nfirst) {
	for (size_t p = blockIdx.x * size_t(blockDim.x) + threadIdx.x; p < N; p += size_t(gridDim.x) * blockDim.x) {
		if (!stay[p]) continue;
		const int32_t s = src[p];
		const size_t q = size_t(nfirst[s]) + (stayrank[p] - stayrank[ofirst[s]]);
		copy_record(out + q * size_t(K), pool + p * size_t(K), K);
	}
}

__global__ void scatter_movers_kernel(const double* __restrict__ pool, double* __restrict__ out, int K, size_t M,
                                      const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int bits,
                                      const uint32_t* __restrict__ nfirst, const uint32_t* __restrict__ staycnt,
                                      const uint32_t* __restrict__ arr_first) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < M; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t ds = keys[i] >> bits;
		const size_t q = size_t(nfirst[ds]) + staycnt[ds] + (uint32_t(i) - arr_first[ds]);
		copy_record(out + q * size_t(K), pool + size_t(vals[i]) * size_t(K), K);
	}
}

int bits_for(size_t n) {  // every value < n fits in this many bits (at least 1)
	int b = 1;
	while (b < 63 && (size_t(1) << b) < n) b++;
	return b;
}

// Cartesian, or stretched with its coordinates given (Grid::str); a geometry
// block that is only a grid file's bytes has no device geometry
void require_geometry(const Grid& g) {
	DX_REQUIRE(g.initialized, "not initialized");
	DX_REQUIRE(g.str.active || g.geo_block.empty(),
	           "the grid holds a stretched geometry block (Cartesian geometry only)");
}

SGeo make_sgeo(Grid& g) {
	SGeo S;
	S.c = stretched_device(g);
	uint32_t at = 0;
	for (int d = 0; d < 3; d++) {
		const auto& c = g.str.c[d];
		S.off[d] = at;
		S.n[d] = uint32_t(c.size());
		at += S.n[d];
		S.g.start[d] = c.front();
		S.g.end[d] = c.back();
		S.g.cell[d] = 0;
		S.g.per[d] = g.per[d];
	}
	S.total = at;
	S.l0 = double(uint64_t(1) << g.R);
	return S;
}

// What the particle calls share on the host.  A call names its field (the
// constructor), checks its own arguments, and then prepare()s: the checks on
// the grid, K, the shape and the geometry, in this order, the record offsets
// of every slot and the record counts (all zero and no offsets: no pool).
struct ParticleCall {
	Grid& g;
	Field& f;
	hipStream_t s;
	int K = 0;
	size_t N_all = 0;    // records of the pool, the remote copies' included
	size_t N_local = 0;  // records of the local cells, the pool's first (where asked for)
	DBuf<uint32_t> ofirst, chunk_slot;

	ParticleCall(Grid& g_, int fid) : g(g_), f(field(g_, fid)), s(g_.s_comp) {
		DX_REQUIRE(f.var, "particles need a variable-size field (this one is fixed-size)");
	}

	double* pool() const { return reinterpret_cast<double*>(f.data.p); }

	// lengths: the call reads cell lengths (CIC does anyway); local: N_local is wanted
	void prepare(int K_, int shape, bool lengths, bool local) {
		K = K_;
		DX_REQUIRE(g.initialized, "not initialized");
		DX_REQUIRE(K >= 3, "a particle record has at least 3 doubles (the position)");
		DX_REQUIRE(shape == 0 || shape == 1, "shape must be 0 (NGP) or 1 (CIC)");
		if (shape == 1) {
			DX_REQUIRE(g.hood_len >= 1, "CIC needs a neighborhood length of at least 1");
			DX_REQUIRE(!g.str.active, "CIC needs a Cartesian geometry (a stretched geometry is set)");
		}
		if (shape == 1 || lengths) require_geometry(g);
		const size_t ns = g.n_slots;
		if (!ns || !f.voff.p) return;
		const uint64_t rec = uint64_t(K) * sizeof(double);
		const uint64_t total = var_total(f, ns, s);
		DX_REQUIRE(total / rec < (uint64_t(1) << 31), "more than 2^31 particles on one process");
		// record offsets of the slots; every cell a whole number of records
		DBuf<int32_t> flag;
		ofirst.alloc(ns + 1);
		flag.alloc(1);
		HIP_CHECK(hipMemsetAsync(flag.p, 0, 4, s));
		launch_per_item(record_offsets_kernel, ns + 1, s, f.voff.p, ns + 1, rec, ofirst.p, flag.p);
		int32_t bad = 0;
		d2h_small(&bad, flag.p, 4, s);
		DX_REQUIRE(!bad, "a cell's payload is not a multiple of 8 * record_doubles bytes");
		N_all = size_t(total / rec);
		if (local && N_all && g.n_local) N_local = size_t(var_total(f, g.n_local, s) / rec);
	}

	// the side table of passes of kPB records over the first N (of n_slots slots)
	void chunk_slots(size_t n_slots, size_t N) {
		launch_pass_slots(ofirst.p, n_slots, N, (N + kPB - 1) / kPB, 0, chunk_slot, s);
	}

	// the call's kernels are queued: ofirst and chunk_slot go out of scope
	void finish() { HIP_CHECK(hipStreamSynchronize(s)); }
};

// -1 (q = 1), or a double of the record from first_allowed on and outside the
// three doubles that start at each of `taken`.  (K < 3 is prepare()'s to refuse.)
void require_weight_double(int K, int wd, int first_allowed, const char* past, std::initializer_list<int> taken = {}) {
	bool ok = wd >= first_allowed && wd < K;
	for (int t : taken) ok = ok && !(wd >= t && wd < t + 3);
	DX_REQUIRE(K < 3 || wd == -1 || ok,
	           std::string("weight_double must be -1 (q = 1) or a double of the record past the ") + past + " (" +
	               std::to_string(first_allowed) + " <= weight_double < record_doubles)");
}

}  // namespace

// the packed device copy of the coordinates, made at first use.  The finest
// cells must be resolvable at both ends of their level-0 cell (c + li != c):
// the point location's correction loops then end after a step or two.
const double* stretched_device(Grid& g) {
	Grid::Stretched& T = g.str;
	DX_REQUIRE(T.active, "no stretched geometry");
	DX_REQUIRE(g.initialized, "not initialized");
	if (T.dev_valid) return T.dev.p;
	std::vector<double> h;
	const double l0 = double(uint64_t(1) << g.R);
	for (int d = 0; d < 3; d++) {
		const auto& c = T.c[d];
		DX_REQUIRE(c.size() == g.len[d] + 1, "the grid's length changed after set_stretched_geometry");
		for (size_t i = 0; i + 1 < c.size(); i++) {
			const double li = (c[i + 1] - c[i]) / l0;
			DX_REQUIRE(li > 0 && c[i] + li > c[i] && c[i + 1] - li < c[i + 1],
			           "stretched geometry: the finest cells of dimension " + std::to_string(d) +
			               " are below the resolution of their coordinates");
		}
		h.insert(h.end(), c.begin(), c.end());
	}
	DX_REQUIRE(h.size() < (size_t(1) << 31), "stretched geometry: too many coordinates");
	T.dev.alloc(h.size());
	h2d(T.dev.p, h.data(), h.size() * sizeof(double), g.s_comp);
	HIP_CHECK(hipStreamSynchronize(g.s_comp));  // h is a local
	T.dev_valid = true;
	return T.dev.p;
}

StretchedView stretched_view(Grid& g) {
	StretchedView V;
	if (!g.str.active) return V;
	V.c = stretched_device(g);
	uint32_t at = 0;
	for (int d = 0; d < 3; d++) {
		V.off[d] = at;
		at += uint32_t(g.str.c[d].size());
	}
	return V;
}

void existing_cells_at(Grid& g, const double* xyz, size_t n, uint64_t* ids) {
	require_geometry(g);
	if (!n) return;
	DX_REQUIRE(xyz && ids, "null pointer");
	hipStream_t s = g.s_comp;
	DBuf<double> dx;
	DBuf<uint64_t> di;
	dx.alloc(3 * n);
	di.alloc(n);
	h2d(dx.p, xyz, 3 * n * sizeof(double), s);
	if (g.str.active)
		cells_at_kernel<SGeo><<<grid_for(n, 256), 256, 0, s>>>(g.m, g.dm(), make_sgeo(g), dx.p, n, di.p);
	else
		cells_at_kernel<PGeo><<<grid_for(n, 256), 256, 0, s>>>(g.m, g.dm(), make_geo(g), dx.p, n, di.p);
	HIP_CHECK(hipGetLastError());
	d2h_small(ids, di.p, n * sizeof(uint64_t), s);
}

void particles_step(Grid& g, int fid, int K, const double* velocity, double dt, uint64_t stats[5]) {
	require_geometry(g);
	ParticleCall P(g, fid);
	// (K before the call's own rules, as dccrgx_particles_reduce)
	DX_REQUIRE(K >= 3, "a particle record has at least 3 doubles (the position)");
	DX_REQUIRE(velocity || K >= 6, "per-particle velocities (velocity == NULL) need records of at least 6 doubles");
	DX_REQUIRE(stats, "null pointer");
	for (int k = 0; k < 5; k++) stats[k] = 0;
	P.prepare(K, 0, false, false);
	Field& f = P.f;
	hipStream_t s = P.s;
	const size_t ns = g.n_slots, nl = g.n_local, N = P.N_all;
	const uint64_t rec = uint64_t(K) * sizeof(double);
	const DBuf<uint32_t>& ofirst = P.ofirst;
	if (!N) return;
	ensure_csr(g);

	// 1. locate
	DBuf<int32_t> src, dest;
	DBuf<uint32_t> stay, mover, stayrank, mpos, part;
	src.alloc(N);
	dest.alloc(N);
	stay.alloc(N + 1);
	mover.alloc(N + 1);
	stayrank.alloc(N + 1);
	mpos.alloc(N + 1);
	const unsigned nb = grid_for(N, kPB, 8192);
	part.alloc(4 * size_t(nb));
	P.chunk_slots(ns, N);
	PArgs a{};
	a.pool = P.pool();
	a.ofirst = ofirst.p;
	a.chunk_slot = P.chunk_slot.p;
	a.n_slots = ns;
	a.n_local = nl;
	a.N = N;
	a.K = K;
	a.slot_ids = g.slot_ids.p;
	a.nof_ptr = g.nof_ptr.p;
	a.nto_ptr = g.nto_ptr.p;
	a.nof_id = g.nof_id.p;
	a.nto_id = g.nto_id.p;
	a.nof_slot = g.nof_slot.p;
	a.has_vel = velocity ? 1 : 0;
	for (int d = 0; d < 3; d++) a.vel[d] = velocity ? velocity[d] : 0.0;
	a.dt = dt;
	a.src = src.p;
	a.dest = dest.p;
	a.stay = stay.p;
	a.mover = mover.p;
	a.part = part.p;
	if (g.str.active)
		particles_locate_kernel<SGeo><<<nb, kPB, 0, s>>>(g.m, g.dm(), make_sgeo(g), a);
	else
		particles_locate_kernel<PGeo><<<nb, kPB, 0, s>>>(g.m, g.dm(), make_geo(g), a);
	HIP_CHECK(hipGetLastError());
	DBuf<uint64_t> dstats;
	dstats.alloc(4);
	sum_parts_kernel<<<1, 256, 0, s>>>(part.p, nb, dstats.p);
	HIP_CHECK(hipGetLastError());

	// 2. ranks of the stayers and of the movers
	size_t n_stay = 0, M = 0;
	scan_exclusive_u32_pair(stay.p, stayrank.p, mover.p, mpos.p, N, s, n_stay, M);

	// 3. movers sorted by (destination slot, source id), index order kept
	DBuf<uint32_t> arr_first, arr_end;
	arr_first.alloc(nl + 1);
	arr_end.alloc(nl + 1);
	HIP_CHECK(hipMemsetAsync(arr_first.p, 0, (nl + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(arr_end.p, 0, (nl + 1) * 4, s));
	DBuf<uint64_t> keys, keys2;
	DBuf<uint32_t> vals, vals2;
	const int bits = bits_for(ns);
	if (M) {
		// rank of every slot's id among the slots' ids
		DBuf<int32_t> iota, order;
		DBuf<uint64_t> sorted_ids;
		DBuf<uint32_t> idrank;
		iota.alloc(ns);
		order.alloc(ns);
		sorted_ids.alloc(ns);
		idrank.alloc(ns);
		k_iota_i32(iota.p, ns, 0, s);
		with_temp(cub_sort_pairs(g.slot_ids.p, sorted_ids.p, iota.p, order.p, ns, map_id_bits(g.m), s));
		launch_per_item(rank_by_id_kernel, ns, s, order.p, ns, idrank.p);
		keys.alloc(M);
		keys2.alloc(M);
		vals.alloc(M);
		vals2.alloc(M);
		launch_per_item(mover_keys_kernel, N, s, src.p, dest.p, mover.p, mpos.p, N, idrank.p, bits, keys.p, vals.p);
		const int end_bit = bits + bits_for(nl);
		with_temp(cub_sort_pairs(keys.p, keys2.p, vals.p, vals2.p, M, end_bit, s));
		// 4. arrivals per destination
		launch_per_item(arrival_runs_kernel, M, s, keys2.p, M, bits, arr_first.p, arr_end.p);
		HIP_CHECK(hipStreamSynchronize(s));  // the unsorted lists go out of scope
	}

	// 5. new sizes
	DBuf<uint32_t> staycnt, newcnt, nfirst;
	staycnt.alloc(ns + 1);
	newcnt.alloc(ns + 1);
	nfirst.alloc(ns + 1);
	launch_per_item(new_counts_kernel, ns, s, ofirst.p, stayrank.p, arr_first.p, arr_end.p, ns, nl, staycnt.p,
	                newcnt.p);
	const size_t Nn = scan_exclusive_u32(newcnt.p, nfirst.p, ns, s);
	DX_REQUIRE(Nn == n_stay + M, "particle counts do not add up");
	DBuf<uint64_t> noff;
	noff.alloc(ns + 1);
	launch_per_item(byte_offsets_kernel, ns + 1, s, nfirst.p, ns + 1, rec, noff.p);

	// 6. scatter into a fresh pool
	DBuf<uint8_t> nd;
	nd.alloc(size_t(Nn) * rec + 1);
	double* out = reinterpret_cast<double*>(nd.p);
	if (n_stay) {
		launch_per_item(scatter_stayers_kernel, N, s, a.pool, out, K, N, src.p, stay.p, stayrank.p, ofirst.p,
		                nfirst.p);
	}
	if (M) {
		launch_per_item(scatter_movers_kernel, M, s, a.pool, out, K, M, keys2.p, vals2.p, bits, nfirst.p,
		                staycnt.p, arr_first.p);
	}
	uint64_t h[4] = {0, 0, 0, 0};
	d2h_small(h, dstats.p, sizeof(h), s);  // drains s
	f.data.swap(nd);
	f.voff.swap(noff);
	field_written(f);
	stats[0] = n_stay;
	for (int k = 0; k < 4; k++) stats[1 + k] = h[k];
}

// ---------------------------------------------------------------------------
// Particles follow the mesh (DESIGN.md "Particles"): in stop_refining's
// rebuild a following field's records go where the reference's user code
// would put them from refined_cell_data (dccrg.hpp:10215-10219) and
// unrefined_cell_data (10387): a refined parent's to the child that
// get_existing_cell (6316-6336) names on the new mesh, the removed children's
// to their new parent.  The passes:
//   1. classify - a thread per old local cell: its new slot (stays), or
//                 refined (its first child is a local cell of the new mesh),
//                 or gone (merged into a parent: its bytes are in the removed
//                 store); the refined ones compacted into a list;
//   2. locate   - a wave per refined parent walks its records 64 at a time:
//                 the child (0..7, 8: none) of each into a byte per record,
//                 the per-child counts by ballots, the children's new sizes;
//   3. parents  - the removed store's cells grouped by parent (children in
//                 ascending id), a parent's new size the sum of theirs;
//   4. a scan of the new sizes;
//   5. scatter  - stayers cell by cell, the refined parents' records by
//                 (child, rank of the record among the child's: ballots and
//                 running counts), the removed children's after one another
//                 into a fresh pool, swapped in.
// No atomic decides a position: only the three statistics are added up.
namespace {

constexpr int kFB = 256;  // four waves, one refined parent each per pass

__global__ void follow_sizes_ok_kernel(const uint64_t* __restrict__ voff, size_t n, uint64_t rec,
                                       int32_t* __restrict__ flag) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t b = voff[i + 1] - voff[i];
		if ((b / rec) * rec != b) *flag = 1;
	}
}

// src: the old local cell of every new slot (-1 preset); refined: n_old + 1 flags
__global__ void follow_classify_kernel(const MapCtx m, const DevMesh newM, const uint64_t* __restrict__ old_ids,
                                       size_t n_old, size_t new_n_local, int32_t* __restrict__ src,
                                       uint32_t* __restrict__ refined) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i <= n_old; i += size_t(gridDim.x) * blockDim.x) {
		uint32_t r = 0;
		if (i < n_old) {
			const uint64_t id = old_ids[i];
			const int32_t ns = dm_slot(newM, id);
			if (ns >= 0) {
				src[ns] = int32_t(i);
			} else {
				const uint64_t c0 = map_child(m, id);
				if (c0 != id && c0 != error_cell) {
					const int32_t cs = dm_slot(newM, c0);
					r = cs >= 0 && size_t(cs) < new_n_local ? 1u : 0u;
				}
			}
		}
		refined[i] = r;
	}
}

__global__ void follow_compact_kernel(const uint32_t* __restrict__ refined, const uint32_t* __restrict__ rpos,
                                      size_t n_old, int32_t* __restrict__ plist) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n_old; i += size_t(gridDim.x) * blockDim.x)
		if (refined[i]) plist[rpos[i]] = int32_t(i);
}

__global__ void follow_stay_sizes_kernel(const int32_t* __restrict__ src, const uint64_t* __restrict__ ooff, size_t n,
                                         uint64_t* __restrict__ sizes) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i <= n; i += size_t(gridDim.x) * blockDim.x)
		sizes[i] = i < n && src[i] >= 0 ? ooff[src[i] + 1] - ooff[src[i]] : 0;
}

// (pointers and counts only: the mapping, the mesh and the geometry are kernel
// parameters of their own, see PArgs)
struct FArgs {
	const double* pool;          // the old pool
	const uint64_t* ooff;        // its byte offsets per old slot
	const uint64_t* old_ids;     // old local slots' ids
	const int32_t* plist;        // the refined old local slots
	size_t P;
	int K;
	size_t new_n_local;
	uint8_t* child;              // per old record: its child 0..7, 8: none
	int32_t* cslot;              // 8 per refined parent: the children's new slots
	uint64_t* sizes;             // per new slot: bytes
	unsigned long long* stats;   // to children, to parents, lost
};

template <class Geo>
__global__ __launch_bounds__(kFB) void follow_locate_kernel(const MapCtx m, const DevMesh M, const Geo G,
                                                              const FArgs a) {
	const double* s_c;
	const bool coords_cached = stage_geometry(G, s_c);
	// the two counts of a block are added up in LDS, one global atomic per
	// block and count (one per child of every parent, all on one address,
	// cost 19 ms at 262 144 parents where the whole carry now takes 0.7 ms)
	__shared__ unsigned long long s_cnt[2];
	if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	uint32_t n_placed = 0, n_lost = 0;
	const uint32_t lane = threadIdx.x & 63u;
	const size_t waves = size_t(gridDim.x) * (kFB >> 6);
	const uint64_t rec = uint64_t(a.K) * sizeof(double);
	for (size_t j = blockIdx.x * size_t(kFB >> 6) + (threadIdx.x >> 6); j < a.P; j += waves) {
		const size_t os = size_t(a.plist[j]);
		uint64_t ch[8];
		map_all_children(m, a.old_ids[os], ch);
		const size_t first = size_t(a.ooff[os] / rec), n = size_t((a.ooff[os + 1] - a.ooff[os]) / rec);
		uint32_t mine = 0;  // lane k < 8: records of child k; lane 8: of none
		for (size_t r0 = 0; r0 < n; r0 += 64) {
			const bool valid = r0 + lane < n;
			uint32_t c = 9;
			if (valid) {
				const double* r = a.pool + (first + r0 + lane) * size_t(a.K);
				const double x[3] = {r[0], r[1], r[2]};
				const uint64_t leaf = cell_at(m, M, G, s_c, coords_cached, x);
				c = 8;
#pragma unroll
				for (int k = 0; k < 8; k++)
					if (leaf == ch[k] && leaf != error_cell) c = uint32_t(k);
				a.child[first + r0 + lane] = uint8_t(c);
			}
#pragma unroll
			for (uint32_t k = 0; k < 9; k++) {
				const unsigned long long b = __ballot(c == k);
				if (lane == k) mine += uint32_t(__popcll(b));
			}
		}
		if (lane < 8) {
			const int32_t cs = dm_slot(M, ch[lane]);
			// (the classify pass saw the first child local; every child of a
			// refined local cell is created on its process)
			const bool ok = cs >= 0 && size_t(cs) < a.new_n_local;
			a.cslot[8 * j + lane] = ok ? cs : -1;
			if (ok) {
				a.sizes[cs] = uint64_t(mine) * rec;
				n_placed += mine;
			} else {
				n_lost += mine;
			}
		} else if (lane == 8) {
			n_lost += mine;
		}
	}
	if (n_placed) atomicAdd(&s_cnt[0], (unsigned long long)n_placed);
	if (n_lost) atomicAdd(&s_cnt[1], (unsigned long long)n_lost);
	__syncthreads();
	if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&a.stats[threadIdx.x == 0 ? 0 : 2], s_cnt[threadIdx.x]);
}

// a refined parent's records into its children, each child's in the parent's order
__global__ __launch_bounds__(kFB) void follow_scatter_children_kernel(const FArgs a, const uint64_t* __restrict__ noff,
                                                                        double* __restrict__ out) {
	const uint32_t lane = threadIdx.x & 63u;
	const size_t waves = size_t(gridDim.x) * (kFB >> 6);
	const uint64_t rec = uint64_t(a.K) * sizeof(double);
	const unsigned long long below = (1ull << lane) - 1ull;
	for (size_t j = blockIdx.x * size_t(kFB >> 6) + (threadIdx.x >> 6); j < a.P; j += waves) {
		const size_t os = size_t(a.plist[j]);
		const size_t first = size_t(a.ooff[os] / rec), n = size_t((a.ooff[os + 1] - a.ooff[os]) / rec);
		// per child (the same in every lane, indexed by unrolled constants
		// only): the record index of its first record in the new pool (~0: no
		// slot) and its records placed so far
		uint64_t start[8];
		uint32_t base[8];
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const int32_t sl = a.cslot[8 * j + k];
			start[k] = sl >= 0 ? noff[sl] / rec : ~uint64_t(0);
			base[k] = 0;
		}
		for (size_t r0 = 0; r0 < n; r0 += 64) {
			const bool valid = r0 + lane < n;
			const uint32_t c = valid ? a.child[first + r0 + lane] : 9u;
			uint64_t q = 0;
			bool place = false;
#pragma unroll
			for (uint32_t k = 0; k < 8; k++) {
				const unsigned long long b = __ballot(c == k);
				if (c == k && start[k] != ~uint64_t(0)) {
					q = start[k] + base[k] + uint32_t(__popcll(b & below));
					place = true;
				}
				base[k] += uint32_t(__popcll(b));
			}
			if (place) copy_record(out + q * size_t(a.K), a.pool + (first + r0 + lane) * size_t(a.K), a.K);
		}
	}
}

// a wave per new slot that keeps its old cell's records
__global__ void follow_copy_stays_kernel(const double* __restrict__ pool, const uint64_t* __restrict__ ooff,
                                         const int32_t* __restrict__ src, double* __restrict__ out,
                                         const uint64_t* __restrict__ noff, size_t n) {
	const uint32_t lane = threadIdx.x & 63u;
	const size_t waves = size_t(gridDim.x) * (blockDim.x >> 6);
	for (size_t i = blockIdx.x * size_t(blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += waves) {
		if (src[i] < 0) continue;
		const double* from = pool + ooff[src[i]] / 8;
		double* to = out + noff[i] / 8;
		const uint64_t len = (noff[i + 1] - noff[i]) / 8;
		for (uint64_t k = lane; k < len; k += 64) to[k] = from[k];
	}
}

__global__ void removed_parent_ids_kernel(const MapCtx m, const uint64_t* __restrict__ rm, size_t n,
                                          uint64_t* __restrict__ par) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		par[i] = map_parent(m, rm[i]);
}

// the removed store's cell i belongs to row `lo` of the sorted parents, at
// its place among the eight children (map_all_children order = ascending id)
__global__ void follow_rows_kernel(const MapCtx m, const uint64_t* __restrict__ rm, size_t n,
                                   const uint64_t* __restrict__ parents, size_t np, int32_t* __restrict__ cidx) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		uint64_t x, y, z;
		const int l = map_indices(m, rm[i], x, y, z);
		if (l <= 0) continue;
		const uint64_t p = map_parent(m, rm[i]);
		const size_t lo = upper_bound_idx<uint64_t>(parents, 0, np, p - 1);  // first parents[lo] >= p
		if (lo >= np || parents[lo] != p) continue;
		const uint64_t o = uint64_t(1) << (m.R - l);  // the child's length in indices
		const int k = int((x / o) & 1u) | int(((y / o) & 1u) << 1) | int(((z / o) & 1u) << 2);
		cidx[8 * lo + size_t(k)] = int32_t(i);
	}
}

__global__ void follow_parent_sizes_kernel(const int32_t* __restrict__ cidx, const int32_t* __restrict__ pslot,
                                           size_t np, size_t new_n_local, const uint64_t* __restrict__ rm_off,
                                           uint64_t rec, uint64_t* __restrict__ sizes,
                                           unsigned long long* __restrict__ stats) {
	__shared__ unsigned long long s_cnt;
	if (threadIdx.x == 0) s_cnt = 0;
	__syncthreads();
	unsigned long long n_records = 0;
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < np; i += size_t(gridDim.x) * blockDim.x) {
		if (pslot[i] < 0 || size_t(pslot[i]) >= new_n_local) continue;
		uint64_t b = 0;
		for (int k = 0; k < 8; k++) {
			const int32_t c = cidx[8 * i + k];
			if (c >= 0) b += rm_off[c + 1] - rm_off[c];
		}
		sizes[pslot[i]] = b;
		n_records += b / rec;
	}
	if (n_records) atomicAdd(&s_cnt, n_records);
	__syncthreads();
	if (threadIdx.x == 0 && s_cnt) atomicAdd(&stats[1], s_cnt);
}

// a wave per (parent, child): the child's removed bytes after its smaller siblings'
__global__ void follow_copy_parents_kernel(const int32_t* __restrict__ cidx, const int32_t* __restrict__ pslot,
                                           size_t np, size_t new_n_local, const uint64_t* __restrict__ rm_off,
                                           const double* __restrict__ removed, const uint64_t* __restrict__ noff,
                                           double* __restrict__ out) {
	const uint32_t lane = threadIdx.x & 63u;
	const size_t waves = size_t(gridDim.x) * (blockDim.x >> 6);
	for (size_t w = blockIdx.x * size_t(blockDim.x >> 6) + (threadIdx.x >> 6); w < 8 * np; w += waves) {
		const size_t i = w / 8;
		const int k = int(w % 8);
		const int32_t c = cidx[w];
		if (c < 0 || pslot[i] < 0 || size_t(pslot[i]) >= new_n_local) continue;
		uint64_t before = 0;
		for (int q = 0; q < k; q++) {
			const int32_t e = cidx[8 * i + q];
			if (e >= 0) before += rm_off[e + 1] - rm_off[e];
		}
		const double* from = removed + rm_off[c] / 8;
		double* to = out + (noff[pslot[i]] + before) / 8;
		const uint64_t len = (rm_off[c + 1] - rm_off[c]) / 8;
		for (uint64_t t = lane; t < len; t += 64) to[t] = from[t];
	}
}

unsigned follow_wave_grid(size_t n) { return grid_for(n, kFB >> 6, 8192); }

}  // namespace

void particles_follow_set(Grid& g, int fid, int K) {
	Field& f = field(g, fid);
	DX_REQUIRE(f.var, "particles need a variable-size field (this one is fixed-size)");
	DX_REQUIRE(K == 0 || K >= 3, "a particle record has at least 3 doubles (the position)");
	f.follow_K = K;
	for (uint64_t& v : f.adapt_stats) v = 0;
}

bool particles_follow_check(Grid& g, const Field& f) {
	require_geometry(g);
	if (!g.n_local || !f.voff.p) return true;
	hipStream_t s = g.s_comp;
	DBuf<int32_t> flag;
	flag.alloc(1);
	HIP_CHECK(hipMemsetAsync(flag.p, 0, 4, s));
	launch_per_item(follow_sizes_ok_kernel, g.n_local, s, f.voff.p, g.n_local,
	                uint64_t(f.follow_K) * sizeof(double), flag.p);
	int32_t bad = 0;
	d2h_small(&bad, flag.p, 4, s);
	return !bad;
}

void particles_follow_rebuild(Grid& g, Field& f, const uint64_t* old_ids, size_t n_old, const DevMesh& newM,
                              size_t ns, size_t nl, hipStream_t s) {
	const int K = f.follow_K;
	const uint64_t rec = uint64_t(K) * sizeof(double);
	const bool had = n_old && f.voff.p;
	DBuf<unsigned long long> dstats;
	dstats.alloc(3);
	HIP_CHECK(hipMemsetAsync(dstats.p, 0, 3 * sizeof(unsigned long long), s));

	// 1. classify
	DBuf<int32_t> src, plist;
	DBuf<uint32_t> refined, rpos;
	src.alloc(ns + 1);
	k_fill_i32(src.p, ns + 1, -1, s);
	size_t P = 0;
	if (had) {
		refined.alloc(n_old + 1);
		rpos.alloc(n_old + 1);
		launch_per_item(follow_classify_kernel, n_old + 1, s, g.m, newM, old_ids, n_old, nl, src.p, refined.p);
		P = scan_exclusive_u32(refined.p, rpos.p, n_old, s);
	}
	DBuf<uint64_t> sizes, noff;
	sizes.alloc(ns + 1);
	noff.alloc(ns + 1);
	if (had) {
		launch_per_item(follow_stay_sizes_kernel, ns + 1, s, src.p, f.voff.p, ns, sizes.p);
	} else {
		HIP_CHECK(hipMemsetAsync(sizes.p, 0, (ns + 1) * 8, s));
	}

	// 2. locate the refined parents' records on the new mesh
	FArgs a{};
	DBuf<uint8_t> child;
	DBuf<int32_t> cslot;
	if (P) {
		const uint64_t total = var_total(f, n_old, s);  // the old pool's local part ends at voff[n_old]
		plist.alloc(P);
		launch_per_item(follow_compact_kernel, n_old, s, refined.p, rpos.p, n_old, plist.p);
		child.alloc(size_t(total / rec) + 1);
		cslot.alloc(8 * P);
		a.pool = reinterpret_cast<const double*>(f.data.p);
		a.ooff = f.voff.p;
		a.old_ids = old_ids;
		a.plist = plist.p;
		a.P = P;
		a.K = K;
		a.new_n_local = nl;
		a.child = child.p;
		a.cslot = cslot.p;
		a.sizes = sizes.p;
		a.stats = dstats.p;
		if (total) {
			if (g.str.active)
				follow_locate_kernel<SGeo><<<follow_wave_grid(P), kFB, 0, s>>>(g.m, newM, make_sgeo(g), a);
			else
				follow_locate_kernel<PGeo><<<follow_wave_grid(P), kFB, 0, s>>>(g.m, newM, make_geo(g), a);
			HIP_CHECK(hipGetLastError());
		} else {
			P = 0;  // nothing to place: the children keep size 0
		}
	}

	// 3. the merged families' parents take the removed store's records
	const size_t n_rm = f.rm_off.p ? g.removed_ids.size() : 0;
	DBuf<uint64_t> up, par;
	DBuf<int32_t> cidx, pslot, err;
	size_t np = 0;
	const uint64_t* rm_dev = nullptr;
	if (n_rm) {
		rm_dev = g.removed_ids.dev();
		if (!rm_dev) {
			upload(up, g.removed_ids.host(s), s);
			rm_dev = up.p;
		}
		par.alloc(n_rm);
		launch_per_item(removed_parent_ids_kernel, n_rm, s, g.m, rm_dev, n_rm, par.p);
		np = sort_unique_u64(par.p, n_rm, s, map_id_bits(g.m));
		cidx.alloc(8 * np);
		pslot.alloc(np);
		err.alloc(1);
		HIP_CHECK(hipMemsetAsync(cidx.p, 0xff, 8 * np * sizeof(int32_t), s));
		HIP_CHECK(hipMemsetAsync(err.p, 0, 4, s));
		launch_per_item(follow_rows_kernel, n_rm, s, g.m, rm_dev, n_rm, par.p, np, cidx.p);
		k_lookup_slots(par.p, np, newM, pslot.p, err.p, s);  // (a parent without a slot: -1, skipped)
		follow_parent_sizes_kernel<<<grid_for(np, 256), 256, 0, s>>>(cidx.p, pslot.p, np, nl, f.rm_off.p, rec, sizes.p,
		                                                             dstats.p);
		HIP_CHECK(hipGetLastError());
	}

	// 4. new offsets, 5. scatter into a fresh pool
	const uint64_t total = scan_exclusive_u64(sizes.p, noff.p, ns, s);
	DBuf<uint8_t> nd;
	nd.alloc(total + 1);
	double* out = reinterpret_cast<double*>(nd.p);
	if (total && had && f.data.p) {
		follow_copy_stays_kernel<<<follow_wave_grid(ns), kFB, 0, s>>>(reinterpret_cast<const double*>(f.data.p),
		                                                              f.voff.p, src.p, out, noff.p, ns);
		HIP_CHECK(hipGetLastError());
	}
	if (total && P) {
		follow_scatter_children_kernel<<<follow_wave_grid(P), kFB, 0, s>>>(a, noff.p, out);
		HIP_CHECK(hipGetLastError());
	}
	if (total && np && f.removed.p) {
		follow_copy_parents_kernel<<<follow_wave_grid(8 * np), kFB, 0, s>>>(
		    cidx.p, pslot.p, np, nl, f.rm_off.p, reinterpret_cast<const double*>(f.removed.p), noff.p, out);
		HIP_CHECK(hipGetLastError());
	}
	unsigned long long h[3] = {0, 0, 0};
	d2h_small(h, dstats.p, sizeof(h), s);  // drains s: the temporaries end here
	f.data.swap(nd);
	f.voff.swap(noff);
	for (int k = 0; k < 3; k++) f.adapt_stats[k] = h[k];
}

// ---------------------------------------------------------------------------
// Particles <-> cell fields (DESIGN.md "Particles"): a record p held by leaf s
// gives leaf c the share W(p, c).  Shape 0 (NGP): 1 for c == s.  Shape 1 (CIC
// over leaves, Cartesian geometry): the cloud is a box the size of s centred
// on the position clamped into s, W the fraction of its volume inside c (the
// periodic images of c included), so the receivers are s and the distinct
// leaves of neighbors_of(s), and every s with W(p, c) > 0 is in
// neighbors_of(c).  Every product, quotient and sum below is one IEEE
// operation in the order of dccrgx.h, so a model forms bitwise equal terms;
// only the order of a sum is the kernel's own.
//   deposit - a wave per receiving local cell c: its own records 64 at a time,
//             then the distinct non-empty leaves of its iterator row (sorted by
//             id: repeats are adjacent) four at a time, 16 lanes each; the
//             lanes' partial sums meet in a fixed shuffle tree and lane 0
//             stores.  No atomic decides a sum: two calls give equal bits.
//   gather  - a thread per record of a local cell (source slot found as in the
//             locate pass): the sum over s and the distinct leaves of its row,
//             up to four fields per pass, stored into the record.
namespace {

struct CellBox {
	double lo[3], L[3], hi[3];
};

// geometry_fill_kernel's low and length of a Cartesian cell.  Its two
// quotients have powers of two as divisors, 1 / 2^level and along / 2^R: the
// first is formed from its exponent, the second is the product with 1 / 2^R,
// both the same bits as the divisions (an fp64 division costs this pass about
// as much as the rest of a weight's dimension)
__device__ __forceinline__ void cell_box(const MapCtx& m, const WGeo& G, uint64_t id, CellBox& B) {
	uint64_t ind[3] = {0, 0, 0};
	const int lvl = map_indices(m, id, ind[0], ind[1], ind[2]);
	const double sf = __longlong_as_double((1023ll - (lvl < 0 ? 0 : lvl)) << 52);
#pragma unroll
	for (int d = 0; d < 3; d++) {
		const double along = double(ind[d]) * G.l0[d];
		const double rel = along * G.inv_fine;
		B.lo[d] = G.start[d] + rel;
		B.L[d] = G.l0[d] * sf;
		B.hi[d] = B.lo[d] + B.L[d];
	}
}

// (cell_volume, (lx * ly) * lz with geometry_fill_kernel's lengths, stands in
// dccrgx_internal.hpp beside WGeo: dccrgx_field_reduce's by_volume uses it too)

__device__ __forceinline__ double overlap_1d(double a, double b, double lo, double hi) {
	const double top = fmin(b, hi);
	const double bottom = fmax(a, lo);
	const double o = top - bottom;
	return fmax(0.0, o);
}

// W(p, c) of a record at x held by the cell S, for the receiving cell C
__device__ __forceinline__ double cic_weight(const WGeo& G, const CellBox& S, const CellBox& C, const double x[3]) {
	double o[3];
#pragma unroll
	for (int d = 0; d < 3; d++) {
		const double xc = fmin(fmax(x[d], S.lo[d]), S.hi[d]);
		const double half = S.L[d] / 2;
		const double a = xc - half;
		const double b = xc + half;
		o[d] = overlap_1d(a, b, C.lo[d], C.hi[d]);
		if (G.per[d]) {
			const double down = -G.period[d], up = G.period[d];
			const double om = overlap_1d(a, b, C.lo[d] + down, C.hi[d] + down);
			const double op = overlap_1d(a, b, C.lo[d] + up, C.hi[d] + up);
			const double lower = om + o[d];
			o[d] = lower + op;
		}
	}
	// no overlap in one dimension: the product of the fractions is +0
	if (o[0] == 0.0 || o[1] == 0.0 || o[2] == 0.0) return 0.0;
	const double fx = o[0] / S.L[0], fy = o[1] / S.L[1], fz = o[2] / S.L[2];
	const double fxy = fx * fy;
	return fxy * fz;
}

WGeo make_wgeo(Grid& g, bool lengths_only) {
	WGeo G{};
	for (int d = 0; d < 3; d++) {
		G.start[d] = g.start[d];
		G.l0[d] = g.l0[d];
		G.period[d] = double(g.len[d]) * g.l0[d];
		G.per[d] = g.per[d];
	}
	G.inv_fine = 1.0 / double(uint64_t(1) << g.R);
	G.c = nullptr;
	if (lengths_only && g.str.active) {
		const StretchedView V = stretched_view(g);
		G.c = V.c;
		for (int d = 0; d < 3; d++) G.off[d] = V.off[d];
	}
	return G;
}

constexpr int kDB = 256;    // four waves, one receiving cell each per pass
constexpr int kDGroup = 16;  // lanes that share one source leaf

struct DArgs {
	const double* pool;
	const uint32_t* ofirst;  // n_slots + 1 record offsets
	const uint64_t* slot_ids;
	const uint32_t* it_ptr;
	const int32_t* it_slot;
	size_t n_local;
	int K, wd, per_volume;  // wd: the record's double that is q (-1: q = 1)
	double* out;
};

// The walk of one receiving local cell c (id cid) by its wave: the cell's own
// records 64 at a time, then (CIC) the distinct non-empty leaves of its row
// four at a time, 16 lanes each.  Every (record, receiver) pair reaches
// acc.add(rec, q, w) once, q the weight double and w = W(p, c); what the
// lanes' sums become is the kernel's.
template <int SHAPE, class Acc>
__device__ __forceinline__ void deposit_walk(const MapCtx& m, const WGeo& G, const DArgs& a, size_t c, uint64_t cid,
                                             uint32_t lane, Acc& acc) {
	const uint32_t grp = lane / kDGroup, gl = lane % kDGroup;
	CellBox C{};
	if (SHAPE == 1) cell_box(m, G, cid, C);
	// the cell's own records
	for (uint32_t r = a.ofirst[c] + lane, r1 = a.ofirst[c + 1]; r < r1; r += 64) {
		const double* rec = a.pool + size_t(r) * size_t(a.K);
		const double q = a.wd < 0 ? 1.0 : rec[a.wd];
		double w = 1.0;
		if (SHAPE == 1) {
			const double x[3] = {rec[0], rec[1], rec[2]};
			w = cic_weight(G, C, C, x);
		}
		acc.add(rec, q, w);
	}
	if (SHAPE == 1) {
		const uint32_t b = a.it_ptr[c], e = a.it_ptr[c + 1];
		for (uint32_t j0 = b; j0 < e; j0 += 64) {
			const uint32_t j = j0 + lane;
			int32_t s = 0;
			bool take = false;
			if (j < e) {
				s = a.it_slot[j];
				take = s >= 0 && size_t(s) != c && (j == b || a.it_slot[j - 1] != s) &&
				       a.ofirst[s + 1] != a.ofirst[s];
			}
			// the sources of this part of the row, four at a time: group k
			// takes the (k + 1)-th lane left in `rem`
			unsigned long long rem = __ballot(take);
			while (rem) {
				unsigned long long mine = rem;
				for (uint32_t k = 0; k < grp; k++) mine &= mine - 1;
				const int from = mine ? __ffsll(mine) - 1 : 0;
				const int32_t sg = __shfl(s, from);
				if (mine) {
					CellBox S;
					cell_box(m, G, a.slot_ids[sg], S);
					for (uint32_t r = a.ofirst[sg] + gl, r1 = a.ofirst[sg + 1]; r < r1; r += kDGroup) {
						const double* rec = a.pool + size_t(r) * size_t(a.K);
						const double q = a.wd < 0 ? 1.0 : rec[a.wd];
						const double x[3] = {rec[0], rec[1], rec[2]};
						const double w = cic_weight(G, S, C, x);
						acc.add(rec, q, w);
					}
				}
				for (int k = 0; k < 64 / kDGroup; k++) rem &= rem - 1;
			}
		}
	}
}

// the deposit's accumulator: one sum of q W
struct DepositSum {
	double sum = 0.0;
	__device__ __forceinline__ void add(const double*, double q, double w) {
		const double term = q * w;
		sum = sum + term;
	}
};

// (at least six waves per SIMD: the CIC form fits 80 VGPRs without scratch,
// and its chains of dependent fp64 operations want the waves: 8.85 -> 7.5 ms
// on the bench's grid against the four waves of 106 VGPRs)
template <int SHAPE>
__global__ __launch_bounds__(kDB) __attribute__((amdgpu_waves_per_eu(6))) void particles_deposit_kernel(const MapCtx m, const WGeo G, const DArgs a) {
	const uint32_t lane = threadIdx.x & 63u;
	const size_t waves = size_t(gridDim.x) * (kDB >> 6);
	for (size_t c = blockIdx.x * size_t(kDB >> 6) + (threadIdx.x >> 6); c < a.n_local; c += waves) {
		const uint64_t cid = a.slot_ids[c];
		DepositSum acc;
		deposit_walk<SHAPE>(m, G, a, c, cid, lane, acc);
		double sum = acc.sum;
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			const double other = __shfl_down(sum, o);
			sum = sum + other;
		}
		if (lane == 0) {
			if (a.per_volume) sum = sum / cell_volume(m, G, cid);
			a.out[c] = sum;
		}
	}
}

// Several moments of the records in one walk (dccrgx_particles_deposit_moments):
// the deposit's walk (deposit_walk) and its shuffle tree, with W(p, c)
// formed once per (record, receiver) and fed to M accumulators.  A call with
// more moments than kMW runs several passes, full ones first.  (DESIGN.md
// "Moments in one deposit pass" has the resource report and the measurements
// the width was chosen from.)
#ifndef DCCRGX_MOMENTS_WIDTH
#define DCCRGX_MOMENTS_WIDTH 5
#endif
constexpr int kMW = DCCRGX_MOMENTS_WIDTH;  // moments per pass (the define is for A/B builds of a narrower width)
static_assert(kMW >= 1 && kMW <= 5, "six accumulators and more spill to scratch even at four waves per SIMD");
// waves per SIMD asked of the compiler: up to three accumulators fit the
// deposit's 80 VGPRs, four need 96 (five waves), five 123 (four waves: ten
// moments in two passes measured 25.2 ms against 29.6 ms in passes of 4, 4
// and 2); none uses scratch
constexpr int moments_waves(int M) { return M <= 3 ? 6 : M == 4 ? 5 : 4; }

// (a kernel parameter of its own, read with unrolled constant indices only:
// the factor indices and the outputs stay in SGPRs, see PArgs)
struct MArgs {
	int fu[kMW], fv[kMW];  // m_j = (q * record[fu[j]]) * record[fv[j]]; -1: 1.0
	double* out[kMW];
};

template <int M>
__device__ __forceinline__ void moments_add(const double* rec, double q, double w, const MArgs& f, double (&sum)[M]) {
#pragma unroll
	for (int j = 0; j < M; j++) {
		// (a factor of -1 costs no load, and the product with 1.0 is kept:
		// loading double 0 instead and dropping it, or branching round the
		// product, both measured slower)
		const double u = f.fu[j] < 0 ? 1.0 : rec[f.fu[j]];
		const double v = f.fv[j] < 0 ? 1.0 : rec[f.fv[j]];
		const double qu = q * u;
		const double mj = qu * v;
		const double term = mj * w;
		sum[j] = sum[j] + term;
	}
}

// the moments' accumulator: the M sums of a pass
template <int M>
struct MomentSums {
	const MArgs& f;
	double sum[M] = {};
	__device__ __forceinline__ void add(const double* rec, double q, double w) { moments_add<M>(rec, q, w, f, sum); }
};

template <int SHAPE, int M>
__global__ __launch_bounds__(kDB) __attribute__((amdgpu_waves_per_eu(moments_waves(M)))) void particles_moments_kernel(
    const MapCtx m, const WGeo G, const DArgs a, const MArgs f) {
	const uint32_t lane = threadIdx.x & 63u;
	const size_t waves = size_t(gridDim.x) * (kDB >> 6);
	for (size_t c = blockIdx.x * size_t(kDB >> 6) + (threadIdx.x >> 6); c < a.n_local; c += waves) {
		const uint64_t cid = a.slot_ids[c];
		MomentSums<M> acc{f};
		deposit_walk<SHAPE>(m, G, a, c, cid, lane, acc);
		double(&sum)[M] = acc.sum;
#pragma unroll
		for (int j = 0; j < M; j++) {
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				const double other = __shfl_down(sum[j], o);
				sum[j] = sum[j] + other;
			}
		}
		if (lane == 0) {
			const double V = a.per_volume ? cell_volume(m, G, cid) : 1.0;
#pragma unroll
			for (int j = 0; j < M; j++) f.out[j][c] = a.per_volume ? sum[j] / V : sum[j];
		}
	}
}

constexpr int kGF = 4;  // cell fields per gather pass

struct GArgs {
	double* pool;
	const uint32_t* ofirst;      // n_local + 1 record offsets
	const uint32_t* chunk_slot;  // chunks + 1 (pass_slots_kernel)
	size_t N;                    // records of the local cells
	int K, first, nf;            // nf fields into doubles first ..
	const uint64_t* slot_ids;
	const uint32_t* it_ptr;
	const int32_t* it_slot;
	const double *f0, *f1, *f2, *f3;
};

template <int SHAPE>
__global__ __launch_bounds__(kPB) void particles_gather_kernel(const MapCtx m, const WGeo G, const GArgs a) {
	__shared__ uint32_t s_off[kOffCache];
	const double* const F[kGF] = {a.f0, a.f1, a.f2, a.f3};
	const size_t chunks = (a.N + kPB - 1) / kPB;
	for (size_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
		const size_t p0 = ch * kPB, p1 = p0 + kPB < a.N ? p0 + kPB : a.N;
		const OffsetWindow W = stage_offsets(a.ofirst, a.chunk_slot, ch, s_off);
		const size_t p = p0 + threadIdx.x;
		if (p >= p1) continue;
		const size_t s = W.slot(uint32_t(p));
		double* r = a.pool + p * size_t(a.K);
		double acc[kGF];
		if (SHAPE == 0) {
#pragma unroll
			for (int j = 0; j < kGF; j++) acc[j] = j < a.nf ? F[j][s] : 0.0;
		} else {
			const double x[3] = {r[0], r[1], r[2]};
			CellBox S;
			cell_box(m, G, a.slot_ids[s], S);
			const double w0 = cic_weight(G, S, S, x);
#pragma unroll
			for (int j = 0; j < kGF; j++) acc[j] = j < a.nf ? w0 * F[j][s] : 0.0;
			int32_t prev = -1;
			for (uint32_t e = a.it_ptr[s], e1 = a.it_ptr[s + 1]; e < e1; e++) {
				const int32_t c = a.it_slot[e];
				if (c == prev) continue;
				prev = c;
				if (c < 0 || size_t(c) == s) continue;
				CellBox C;
				cell_box(m, G, a.slot_ids[c], C);
				const double w = cic_weight(G, S, C, x);
				if (!(w > 0.0)) continue;
#pragma unroll
				for (int j = 0; j < kGF; j++) {
					if (j < a.nf) {
						const double term = w * F[j][c];
						acc[j] = acc[j] + term;
					}
				}
			}
		}
#pragma unroll
		for (int j = 0; j < kGF; j++)
			if (j < a.nf) r[a.first + j] = acc[j];
	}
}

// v += (factor q) E for the first N records of the pool (the local cells'):
// the product rounded, then the sum.  The update does not depend on the
// holding cell, so no slot is looked up.
__global__ __launch_bounds__(kPB) void particles_accelerate_kernel(double* __restrict__ pool, size_t N, int K, int first,
                                                                   int wd, double factor) {
	for (size_t p = blockIdx.x * size_t(kPB) + threadIdx.x; p < N; p += size_t(gridDim.x) * kPB) {
		double* r = pool + p * size_t(K);
		const double k = wd >= 0 ? factor * r[wd] : factor;
		const double e0 = r[first], e1 = r[first + 1], e2 = r[first + 2];
		const double v0 = r[3], v1 = r[4], v2 = r[5];
		const double t0 = k * e0, t1 = k * e1, t2 = k * e2;
		r[3] = v0 + t0;
		r[4] = v1 + t1;
		r[5] = v2 + t2;
	}
}

// the Boris kick of dccrgx.h for the first N records of the pool: half the
// electric kick, the rotation about B, the other half; every operation
// rounded on its own (fp contract is off in this file)
__global__ __launch_bounds__(kPB) void particles_boris_kernel(double* __restrict__ pool, size_t N, int K, int ef, int bf,
                                                              int wd, double factor) {
	for (size_t p = blockIdx.x * size_t(kPB) + threadIdx.x; p < N; p += size_t(gridDim.x) * kPB) {
		double* r = pool + p * size_t(K);
		const double h = wd >= 0 ? factor * r[wd] : factor;
		const double e0 = r[ef], e1 = r[ef + 1], e2 = r[ef + 2];
		const double b0 = r[bf], b1 = r[bf + 1], b2 = r[bf + 2];
		const double v0 = r[3], v1 = r[4], v2 = r[5];
		const double he0 = h * e0, he1 = h * e1, he2 = h * e2;
		const double m0 = v0 + he0, m1 = v1 + he1, m2 = v2 + he2;
		const double t0 = h * b0, t1 = h * b1, t2 = h * b2;
		const double t00 = t0 * t0, t11 = t1 * t1, t22 = t2 * t2;
		const double t01 = t00 + t11;
		const double tt = t01 + t22;
		const double den = 1.0 + tt;
		const double d0 = 2.0 * t0, d1 = 2.0 * t1, d2 = 2.0 * t2;
		const double s0 = d0 / den, s1 = d1 / den, s2 = d2 / den;
		// c = vm x t
		const double c0a = m1 * t2, c0b = m2 * t1;
		const double c1a = m2 * t0, c1b = m0 * t2;
		const double c2a = m0 * t1, c2b = m1 * t0;
		const double c0 = c0a - c0b, c1 = c1a - c1b, c2 = c2a - c2b;
		const double p0 = m0 + c0, p1 = m1 + c1, p2 = m2 + c2;
		// d = vp x s
		const double g0a = p1 * s2, g0b = p2 * s1;
		const double g1a = p2 * s0, g1b = p0 * s2;
		const double g2a = p0 * s1, g2b = p1 * s0;
		const double g0 = g0a - g0b, g1 = g1a - g1b, g2 = g2a - g2b;
		const double q0 = m0 + g0, q1 = m1 + g1, q2 = m2 + g2;
		r[3] = q0 + he0;
		r[4] = q1 + he1;
		r[5] = q2 + he2;
	}
}

// dccrgx_particles_reduce, first stage: a thread per record of the first N of
// the pool (the local cells'), as particles_accelerate_kernel walks them.
// Only the doubles the terms name are read (D.d, each once per record, eight
// loads in flight), staged in the thread's LDS column; 128 threads, so that
// 33 values a record fit 64 KB.  Block b's partials go to part[b * kRedTerms ..].
constexpr int kRP = 128;

struct RedDoubles {
	int d[kRedValues];
};

__global__ __launch_bounds__(kRP) void particles_reduce_kernel(const double* __restrict__ pool, size_t N, int K,
                                                               const RedArgs T, const RedDoubles D,
                                                               double* __restrict__ part) {
	extern __shared__ double red_sh[];
	double acc[kRedTerms];
	red_init(T, acc);
	const int col = int(threadIdx.x);
	for (size_t p = blockIdx.x * size_t(kRP) + threadIdx.x; p < N; p += size_t(gridDim.x) * kRP) {
		const double* r = pool + p * size_t(K);
		for (int f0 = 0; f0 < T.nv; f0 += 8) {
			double v[8];
#pragma unroll
			for (int k = 0; k < 8; k++)
				if (f0 + k < T.nv) v[k] = r[D.d[f0 + k]];
#pragma unroll
			for (int k = 0; k < 8; k++)
				if (f0 + k < T.nv) red_sh[(f0 + k) * kRP + col] = v[k];
		}
		red_accumulate(T, red_sh, kRP, col, 1.0, acc);
	}
	const double r = red_block<kRP>(T, red_sh, acc);
	if (int(threadIdx.x) < T.n) part[size_t(blockIdx.x) * kRedTerms + threadIdx.x] = r;
}

Field& fp64_cell_field(Grid& g, int fid, const char* what) {
	Field& F = fixed_field(g, fid);
	DX_REQUIRE(F.elem == 8, std::string(what) + " must be a fixed-size field of 8-byte elements (fp64)");
	return F;
}

// the walk's arguments of a prepared call with records (ensure_csr: the rows)
DArgs make_dargs(const ParticleCall& P, int weight_double, int per_volume, double* out) {
	ensure_csr(P.g);
	DArgs a{};
	a.pool = P.pool();
	a.ofirst = P.ofirst.p;
	a.slot_ids = P.g.slot_ids.p;
	a.it_ptr = P.g.it_ptr.p;
	a.it_slot = P.g.it_slot.p;
	a.n_local = P.g.n_local;
	a.K = P.K;
	a.wd = weight_double;
	a.per_volume = per_volume ? 1 : 0;
	a.out = out;
	return a;
}

}  // namespace

void particles_deposit(Grid& g, int fid, int K, int shape, int weight_double, int out_fid, int per_volume) {
	ParticleCall P(g, fid);
	Field& out = fp64_cell_field(g, out_fid, "the deposit's output");
	require_weight_double(K, weight_double, 3, "position");
	P.prepare(K, shape, per_volume != 0, false);
	const size_t nl = g.n_local;
	field_written(out);
	if (!nl) return;
	double* o = reinterpret_cast<double*>(out.data.p);
	if (!P.N_all) {  // every sum is empty
		HIP_CHECK(hipMemsetAsync(o, 0, nl * sizeof(double), P.s));
		return;
	}
	const DArgs a = make_dargs(P, weight_double, per_volume, o);
	const WGeo G = make_wgeo(g, per_volume != 0);
	const unsigned nb = grid_for(nl, kDB >> 6, 1u << 20);
	if (shape == 1)
		particles_deposit_kernel<1><<<nb, kDB, 0, P.s>>>(g.m, G, a);
	else
		particles_deposit_kernel<0><<<nb, kDB, 0, P.s>>>(g.m, G, a);
	HIP_CHECK(hipGetLastError());
	P.finish();
}

namespace {

// one pass of exactly `width` moments (1 .. kMW): a missing instantiation is an error
template <int M>
void moments_launch(int width, int shape, unsigned nb, hipStream_t s, const MapCtx& m, const WGeo& G, const DArgs& a,
                    const MArgs& f) {
	if (width == M) {
		if (shape == 1)
			particles_moments_kernel<1, M><<<nb, kDB, 0, s>>>(m, G, a, f);
		else
			particles_moments_kernel<0, M><<<nb, kDB, 0, s>>>(m, G, a, f);
		return;
	}
	if constexpr (M > 1)
		moments_launch<M - 1>(width, shape, nb, s, m, G, a, f);
	else
		DX_REQUIRE(false, "no moments kernel of this width");
}

}  // namespace

void particles_deposit_moments(Grid& g, int fid, int K, int shape, int weight_double, const int* factors,
                               const int* out_fids, int n, int per_volume) {
	ParticleCall P(g, fid);
	DX_REQUIRE(n >= 1 && n <= 16, "the number of moments must be 1 .. 16");
	DX_REQUIRE(factors && out_fids, "null pointer");
	std::vector<double*> outs;
	for (int j = 0; j < n; j++) {
		Field& o = fp64_cell_field(g, out_fids[j], "a moment's output");
		for (int i = 0; i < j; i++)
			DX_REQUIRE(out_fids[i] != out_fids[j], "two moments share an output field");
		outs.push_back(reinterpret_cast<double*>(o.data.p));
	}
	require_weight_double(K, weight_double, 3, "position");
	for (int j = 0; j < 2 * n; j++)
		DX_REQUIRE(factors[j] == -1 || (factors[j] >= 3 && factors[j] < K) || K < 3,
		           "a moment factor must be -1 (1.0) or a double of the record past the position (3 <= factor < "
		           "record_doubles)");
	P.prepare(K, shape, per_volume != 0, false);
	const size_t nl = g.n_local;
	hipStream_t s = P.s;
	for (int j = 0; j < n; j++) field_written(fixed_field(g, out_fids[j]));
	if (!nl) return;
	if (!P.N_all) {  // every sum is empty
		for (int j = 0; j < n; j++) HIP_CHECK(hipMemsetAsync(outs[size_t(j)], 0, nl * sizeof(double), s));
		return;
	}
	const DArgs a = make_dargs(P, weight_double, per_volume, nullptr);
	const WGeo G = make_wgeo(g, per_volume != 0);
	const unsigned nb = grid_for(nl, kDB >> 6, 1u << 20);
	for (int j0 = 0; j0 < n; j0 += kMW) {
		const int width = n - j0 < kMW ? n - j0 : kMW;
		MArgs ma{};
		for (int j = 0; j < kMW; j++) {
			const bool on = j < width;
			ma.fu[j] = on ? factors[2 * (j0 + j)] : -1;
			ma.fv[j] = on ? factors[2 * (j0 + j) + 1] : -1;
			ma.out[j] = on ? outs[size_t(j0 + j)] : nullptr;
		}
		moments_launch<kMW>(width, shape, nb, s, g.m, G, a, ma);
		HIP_CHECK(hipGetLastError());
	}
	P.finish();
}

void particles_gather(Grid& g, int fid, int K, int shape, const int* cell_fields, int n, int first_double) {
	ParticleCall P(g, fid);
	DX_REQUIRE(n >= 1 && cell_fields, "gather needs at least one cell field");
	std::vector<const double*> F;
	for (int j = 0; j < n; j++)
		F.push_back(reinterpret_cast<const double*>(fp64_cell_field(g, cell_fields[j], "a gathered cell field").data.p));
	DX_REQUIRE(K < 3 || (first_double >= 3 && first_double + n <= K),
	           "the gathered doubles must lie in the record past the position (3 <= first_double, first_double + n <= "
	           "record_doubles)");
	P.prepare(K, shape, false, true);
	const size_t N = P.N_local;
	hipStream_t s = P.s;
	if (!N) return;
	ensure_csr(g);
	P.chunk_slots(g.n_local, N);
	GArgs a{};
	a.pool = P.pool();
	a.ofirst = P.ofirst.p;
	a.chunk_slot = P.chunk_slot.p;
	a.N = N;
	a.K = K;
	a.slot_ids = g.slot_ids.p;
	a.it_ptr = g.it_ptr.p;
	a.it_slot = g.it_slot.p;
	const WGeo G = make_wgeo(g, false);
	const unsigned nb = grid_for(N, kPB, 1u << 20);
	for (int j0 = 0; j0 < n; j0 += kGF) {
		a.first = first_double + j0;
		a.nf = n - j0 < kGF ? n - j0 : kGF;
		const double* p[kGF] = {nullptr, nullptr, nullptr, nullptr};
		for (int j = 0; j < a.nf; j++) p[j] = F[size_t(j0 + j)];
		a.f0 = p[0];
		a.f1 = p[1];
		a.f2 = p[2];
		a.f3 = p[3];
		if (shape == 1)
			particles_gather_kernel<1><<<nb, kPB, 0, s>>>(g.m, G, a);
		else
			particles_gather_kernel<0><<<nb, kPB, 0, s>>>(g.m, G, a);
		HIP_CHECK(hipGetLastError());
	}
	field_written(P.f);
	P.finish();
}

void particles_accelerate(Grid& g, int fid, int K, int first_double, int weight_double, double factor) {
	ParticleCall P(g, fid);
	DX_REQUIRE(K < 3 || (first_double >= 6 && first_double + 3 <= K),
	           "the field's three doubles must lie in the record past the velocity (6 <= first_double, first_double + 3 "
	           "<= record_doubles)");
	require_weight_double(K, weight_double, 6, "velocity and outside the field's three", {first_double});
	P.prepare(K, 0, false, true);
	const size_t N = P.N_local;
	if (!N) return;
	particles_accelerate_kernel<<<grid_for(N, kPB, 1u << 20), kPB, 0, P.s>>>(P.pool(), N, K, first_double, weight_double,
	                                                                         factor);
	HIP_CHECK(hipGetLastError());
	field_written(P.f);
	P.finish();
}

void particles_boris(Grid& g, int fid, int K, int e_first, int b_first, int weight_double, double factor) {
	ParticleCall P(g, fid);
	DX_REQUIRE(K < 3 || (e_first >= 6 && e_first + 3 <= K),
	           "E's three doubles must lie in the record past the velocity (6 <= e_first, e_first + 3 <= "
	           "record_doubles)");
	DX_REQUIRE(K < 3 || (b_first >= 6 && b_first + 3 <= K),
	           "B's three doubles must lie in the record past the velocity (6 <= b_first, b_first + 3 <= "
	           "record_doubles)");
	DX_REQUIRE(K < 3 || b_first >= e_first + 3 || e_first >= b_first + 3,
	           "E's and B's doubles overlap (e_first and b_first must be at least 3 apart)");
	require_weight_double(K, weight_double, 6, "velocity and outside E's and B's three", {e_first, b_first});
	P.prepare(K, 0, false, true);
	const size_t N = P.N_local;
	if (!N) return;
	particles_boris_kernel<<<grid_for(N, kPB, 1u << 20), kPB, 0, P.s>>>(P.pool(), N, K, e_first, b_first, weight_double,
	                                                                    factor);
	HIP_CHECK(hipGetLastError());
	field_written(P.f);
	P.finish();
}

// up to 16 reductions over the records of the local cells, the results in
// device memory d_out, queued on the compute stream.  The checks of the
// cells' byte counts and the number of local records (which sizes the grid)
// are read back first, as in every particle call; from there on nothing
// waits on the host.
void particles_reduce(Grid& g, int fid, int K, int weight_double, const int* terms, int n, int collective,
                      double* d_out) {
	ParticleCall P(g, fid);
	DX_REQUIRE(n >= 1 && n <= kRedTerms, "the number of terms must be 1 .. 16");
	DX_REQUIRE(terms && d_out, "null pointer");
	DX_REQUIRE(K >= 3, "a particle record has at least 3 doubles (the position)");
	require_weight_double(K, weight_double, 3, "position");
	RedArgs T;
	RedDoubles D{};
	T.n = n;
	auto staged = [&](int d) {  // the column of the record's double d
		if (d == -1) return kRedOne;
		for (int i = 0; i < T.nv; i++)
			if (D.d[i] == d) return i;
		D.d[T.nv] = d;
		return T.nv++;
	};
	int cops[kRedTerms];
	for (int j = 0; j < n; j++) {
		const int op = terms[3 * j], u = terms[3 * j + 1], v = terms[3 * j + 2];
		DX_REQUIRE(op >= DCCRGX_REDUCE_SUM && op <= DCCRGX_REDUCE_MAX_ABS, "unknown reduction (DCCRGX_REDUCE_*)");
		DX_REQUIRE((u == -1 || (u >= 3 && u < K)) && (v == -1 || (v >= 3 && v < K)),
		           "a term's factor must be -1 (1.0) or a double of the record past the position (3 <= factor < "
		           "record_doubles)");
		T.op[j] = int8_t(op);
		T.x0[j] = int8_t(staged(weight_double));
		T.x1[j] = int8_t(staged(u));
		T.x2[j] = int8_t(staged(v));
		cops[j] = red_combine_op(op);
	}
	if (collective && g.size > 1) comm_require(g, "a collective reduction");
	P.prepare(K, 0, false, true);
	const size_t N = P.N_local;
	hipStream_t s = P.s;
	const unsigned nb = N ? grid_for(N, kRP, 4096) : 0;
	k_time_begin(g);
	if (nb) {
		g.red_part.reserve(size_t(nb) * kRedTerms);
		const size_t lds = std::max(size_t(T.nv) * kRP, size_t(kRedTerms) * (kRP / 64)) * sizeof(double);
		particles_reduce_kernel<<<nb, kRP, lds, s>>>(P.pool(), N, K, T, D, g.red_part.p);
		HIP_CHECK(hipGetLastError());
	}
	k_reduce_fold(T, g.red_part.p, nb, d_out, s);
	k_time_end(g);
	if (collective) comm_allreduce_f64_ops_dev(g, d_out, d_out, n, cops, s);
}

// where dccrgx_field_reduce's by_volume takes V_c from: cell_volume, as the
// deposit's per_volume (and its rule for a stretched block without
// coordinates); on a Cartesian geometry the level's volume, the same bits
RedVolume reduce_volume(Grid& g, bool by_volume) {
	RedVolume V;
	if (!by_volume) return V;
	require_geometry(g);
	V.G = make_wgeo(g, true);
	V.slot_ids = g.slot_ids.p;
	if (g.str.active) {
		V.mode = 2;
		return V;
	}
	V.mode = 1;
	const double a = g.l0[0] * g.l0[1];
	V.vol0 = a * g.l0[2];
	if (g.R > 0) {
		ensure_face(g);  // the level byte of every slot
		V.slot_lvl = g.slot_lvl.p;
	}
	return V;
}

// ---------------------------------------------------------------------------
// Particles are created on the device (dccrgx_particles_create; DESIGN.md
// "Particles").  Every value is a function of (seed, cell id, index among the
// cell's new records, double): Philox4x32-10 keyed by the seed with that
// counter, so neither the slot, the launch nor the other processes matter.
//   1. counts   - a thread per slot: the new byte size (old + 8 K n_c of a
//                 local cell, old of a remote copy), the two refusals;
//   2. a scan of the sizes and the re-lay of varfield.hip, old records in
//                 front, the new region left unwritten;
//   3. generate - a thread per *double* of the new records: a wave stores 512
//                 contiguous bytes wherever it lies inside one cell.  The
//                 cell comes from the new records' offsets by the locate
//                 kernel's narrowed search.  No atomic, no exchange: doubles
//                 0 and 1 each compute block 0.
namespace {

constexpr int kCB = 256;  // doubles per block pass
static_assert(kCB == kPB, "stage_offsets copies with a block of kPB threads");

struct CRecipe {
	const double *fa, *fb;  // cell fields scaling a and b (nullptr: none)
	double a, b;
	int kind;  // 0 constant, 1 uniform, 2 normal
};

// geometry_fill_kernel's geometry: Cartesian start and l0, or the packed
// coordinates of the stretched one
struct CGeo {
	double start[3], l0[3];
	const double* c;
	uint32_t off[3];
};

struct CArgs {
	double* pool;
	const uint64_t* noff;        // byte offsets of the new layout
	const uint32_t* nfirst;      // n_local + 1: first new record of every local slot, all new records numbered through
	const uint32_t* tile_slot;   // tiles + 1 (pass_slots_kernel)
	const uint64_t* slot_ids;
	const CRecipe* recipe;       // K entries
	size_t Nd;                   // doubles to write: new records * K
	uint32_t K, k0, k1;
};

// err[0]: the lowest local slot whose count is refused (~0: none); err[1]: a
// local cell's bytes are no whole records
__global__ void create_counts_kernel(const uint64_t* __restrict__ voff, const uint64_t* __restrict__ slot_ids,
                                     size_t n_slots, size_t n_local, uint64_t rec, const double* __restrict__ F,
                                     double count, int round_random, uint32_t k0, uint32_t k1,
                                     uint64_t* __restrict__ sizes, uint32_t* __restrict__ err) {
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s <= n_slots; s += size_t(gridDim.x) * blockDim.x) {
		if (s == n_slots) {
			sizes[s] = 0;
			continue;
		}
		const uint64_t old = voff[s + 1] - voff[s];
		uint64_t add = 0;
		if (s < n_local) {
			if ((old / rec) * rec != old) err[1] = 1;
			double v = F ? count * F[s] : count;
			if (!(v >= 0.0) || v >= 2147483648.0) {
				atomicMin(&err[0], uint32_t(s));
			} else {
				if (round_random) {
					const uint64_t id = slot_ids[s];
					uint32_t w[4];
					philox4x32_10(uint32_t(id), uint32_t(id >> 32), 0xFFFFFFFFu, 0xFFFFFFFFu, k0, k1, w);
					const double u = philox_uniform(w[0], w[1]);
					v = v + u;
				}
				add = uint64_t(floor(v)) * rec;
			}
		}
		sizes[s] = old + add;
	}
}

// the new records in front of every slot: the bytes the new layout put before
// it less the bytes the old one did
__global__ void create_first_kernel(const uint64_t* __restrict__ noff, const uint64_t* __restrict__ ooff, size_t n,
                                    uint64_t rec, uint32_t* __restrict__ nfirst) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		nfirst[i] = uint32_t((noff[i] - ooff[i]) / rec);
}

// the next double towards -inf of a finite value
__device__ __forceinline__ double pred(double h) {
	long long b = __double_as_longlong(h);
	if (h > 0.0)
		b--;
	else if (h < 0.0)
		b++;
	else
		b = (long long)0x8000000000000001ull;
	return __longlong_as_double(b);
}

// 2^-k, exact
__device__ __forceinline__ double pow2_neg(int k) { return __longlong_as_double((1023ll - k) << 52); }

// center and length of dimension d of the cell id: geometry_fill_kernel's
// expressions.  Its quotients have powers of two as divisors; they are the
// products with the exact reciprocals here, the same bits (cell_box)
__device__ __forceinline__ void create_center_length(const MapCtx& m, const CGeo& G, uint64_t id, uint32_t d,
                                                     double& center, double& L) {
	uint64_t i0 = 0, i1 = 0, i2 = 0;
	const int lvl = map_indices(m, id, i0, i1, i2);
	const uint64_t ind = d == 0 ? i0 : d == 1 ? i1 : i2;
	const double inv_lvl = pow2_neg(lvl < 0 ? 0 : lvl), inv_fine = pow2_neg(m.R);
	if (G.c) {
		const uint32_t off = d == 0 ? G.off[0] : d == 1 ? G.off[1] : G.off[2];
		const uint64_t c_i = ind >> m.R;
		const double c0 = G.c[off + c_i];
		const double extent = G.c[off + c_i + 1] - c0;
		L = extent * inv_lvl;
		const double length_of_index = extent * inv_fine;
		const double in_cell = length_of_index * double(ind - (c_i << m.R));
		const double low = c0 + in_cell;
		center = low + L / 2;
	} else {
		const double start = d == 0 ? G.start[0] : d == 1 ? G.start[1] : G.start[2];
		const double l0 = d == 0 ? G.l0[0] : d == 1 ? G.l0[1] : G.l0[2];
		L = l0 * inv_lvl;
		const double along = double(ind) * l0;
		const double rel = along * inv_fine;
		const double low = start + rel;
		center = low + L / 2;
	}
}

// Every double is A + B * z, one product and one sum: a position with
// A = center, B = L, z = u - 0.5 (then clamped), a recipe's with A = base,
// B = spread, z = the uniform or the normal.  The lanes of a wave hold
// different doubles of a record, so the kernel keeps what they share in one
// path - one Philox block for every lane that needs one, one product and sum
// - and branches only for the geometry and for the normal's log, sqrt and cos.
__global__ __launch_bounds__(kCB) void particles_create_kernel(const MapCtx m, const CGeo G, const CArgs a) {
	__shared__ uint32_t s_off[kOffCache];
	const size_t tiles = (a.Nd + kCB - 1) / kCB;
	for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
		const size_t d0 = t * kCB;
		const size_t r0 = d0 / a.K;  // the same in every lane
		const uint32_t j0 = uint32_t(d0 - r0 * a.K);
		const OffsetWindow W = stage_offsets(a.nfirst, a.tile_slot, t, s_off);
		if (d0 + threadIdx.x >= a.Nd) continue;
		const uint32_t within = j0 + threadIdx.x;
		const uint32_t dr = within / a.K;
		const uint32_t j = within - dr * a.K;
		const uint32_t r = uint32_t(r0) + dr;
		const size_t c = W.slot(r);
		const uint32_t f0 = W.at(c), f1 = W.at(c + 1);
		const uint32_t i = r - f0;
		// the cell's new records end where its bytes end
		double* dst = a.pool + (a.noff[c + 1] / 8 - size_t(f1 - f0) * a.K) + size_t(i) * a.K + j;
		const uint64_t id = a.slot_ids[c];
		const bool pos = j < 3;
		int kind = 1;
		double A, B = 0.0;
		if (pos) {
			create_center_length(m, G, id, j, A, B);
		} else {
			const CRecipe R = a.recipe[j];
			kind = R.kind;
			A = R.fa ? R.a * R.fa[c] : R.a;
			if (kind != 0) B = R.fb ? R.b * R.fb[c] : R.b;
		}
		double val = A;  // a constant
		if (kind != 0) {
			uint32_t w[4];
			philox4x32_10(uint32_t(id), uint32_t(id >> 32), i, pos ? (j < 2 ? 0u : 1u) : j, a.k0, a.k1, w);
			const double first = philox_uniform(w[0], w[1]), second = philox_uniform(w[2], w[3]);
			double z;
			if (pos) {
				const double u = j == 1 ? second : first;
				z = u - 0.5;
			} else if (kind == 2) {
				const double q = 1.0 - first;
				const double lg = log(q);
				const double tt = -2.0 * lg;
				const double rad = sqrt(tt);
				const double theta = 6.283185307179586 * second;
				const double cs = cos(theta);
				z = rad * cs;
			} else {
				z = first;
			}
			const double bz = B * z;
			val = A + bz;
			if (pos) {
				const double half = B / 2;
				const double low = A - half;
				const double high = A + half;
				val = fmin(fmax(val, low), pred(high));
			}
		}
		*dst = val;
	}
}

}  // namespace

void particles_create(Grid& g, int fid, int K, int count_field, double count, int round_random, const int* recipe_i,
                      const double* recipe_d, uint64_t seed, uint64_t* created) {
	DX_REQUIRE(created, "null pointer");
	*created = 0;
	Field& f = field(g, fid);
	DX_REQUIRE(f.var, "particles need a variable-size field (this one is fixed-size)");
	DX_REQUIRE(K >= 3, "a particle record has at least 3 doubles (the position)");
	DX_REQUIRE(round_random == 0 || round_random == 1, "round_random must be 0 (floor) or 1 (random rounding)");
	DX_REQUIRE(std::isfinite(count), "count must be finite");
	DX_REQUIRE(K == 3 || (recipe_i && recipe_d), "null pointer");
	const double* F = nullptr;
	if (count_field != -1) F = reinterpret_cast<const double*>(fp64_cell_field(g, count_field, "count_field").data.p);
	std::vector<CRecipe> rc(static_cast<size_t>(K));
	for (int j = 0; j < K; j++) {
		CRecipe& R = rc[size_t(j)];
		R = CRecipe{nullptr, nullptr, 0.0, 0.0, 0};
		if (j < 3) continue;  // the position: its entries are ignored
		R.kind = recipe_i[3 * j];
		DX_REQUIRE(R.kind >= 0 && R.kind <= 2,
		           "recipe kind of double " + std::to_string(j) + " must be 0 (constant), 1 (uniform) or 2 (normal)");
		const int bf = recipe_i[3 * j + 1], sf = recipe_i[3 * j + 2];
		if (bf != -1) R.fa = reinterpret_cast<const double*>(fp64_cell_field(g, bf, "a recipe's base_field").data.p);
		if (sf != -1) R.fb = reinterpret_cast<const double*>(fp64_cell_field(g, sf, "a recipe's spread_field").data.p);
		R.a = recipe_d[2 * j];
		R.b = recipe_d[2 * j + 1];
	}
	require_geometry(g);
	hipStream_t s = g.s_comp;
	const size_t ns = g.n_slots, nl = g.n_local;
	if (!ns || !nl) return;
	if (!f.voff.p) var_reset(f, ns, s);
	const uint64_t rec = uint64_t(K) * sizeof(double);
	const uint32_t k0 = uint32_t(seed), k1 = uint32_t(seed >> 32);

	// 1. the new sizes and the refusals
	DBuf<uint64_t> sizes, noff;
	DBuf<uint32_t> err;
	sizes.alloc(ns + 1);
	noff.alloc(ns + 1);
	err.alloc(2);
	const uint32_t err0[2] = {0xFFFFFFFFu, 0u};
	h2d(err.p, err0, sizeof(err0), s);
	launch_per_item(create_counts_kernel, ns + 1, s, f.voff.p, g.slot_ids.p, ns, nl, rec, F, count, round_random,
	                k0, k1, sizes.p, err.p);
	uint32_t herr[2] = {0, 0};
	d2h_small(herr, err.p, sizeof(herr), s);
	DX_REQUIRE(!herr[1], "a cell's payload is not a multiple of 8 * record_doubles bytes");
	if (herr[0] != 0xFFFFFFFFu) {
		uint64_t id = 0;
		d2h_small(&id, g.slot_ids.p + herr[0], sizeof(id), s);
		DX_REQUIRE(false, "the count of cell " + std::to_string(id) + " is NaN, negative or at least 2^31");
	}

	// 2. the new layout, the old records in front
	const uint64_t old_total = var_total(f, ns, s);
	const uint64_t total = scan_exclusive_u64(sizes.p, noff.p, ns, s);
	const uint64_t N = (total - old_total) / rec;
	if (!N) return;
	DX_REQUIRE(total / rec < (uint64_t(1) << 31), "more than 2^31 particles on one process");
	var_relay(f, ns, noff, total, false, s);  // noff: the previous offsets from here on

	// 3. generate
	DBuf<uint32_t> nfirst, tile_slot;
	DBuf<CRecipe> drc;
	nfirst.alloc(nl + 1);
	launch_per_item(create_first_kernel, nl + 1, s, f.voff.p, noff.p, nl + 1, rec, nfirst.p);
	const size_t Nd = size_t(N) * size_t(K);
	const size_t tiles = (Nd + kCB - 1) / kCB;
	launch_pass_slots(nfirst.p, nl, size_t(N), tiles, size_t(K), tile_slot, s);
	drc.alloc(size_t(K));
	h2d(drc.p, rc.data(), size_t(K) * sizeof(CRecipe), s);
	CGeo G{};
	if (g.str.active) {
		const StretchedView V = stretched_view(g);
		G.c = V.c;
		for (int d = 0; d < 3; d++) G.off[d] = V.off[d];
	} else {
		for (int d = 0; d < 3; d++) {
			G.start[d] = g.start[d];
			G.l0[d] = g.l0[d];
		}
	}
	CArgs a{};
	a.pool = reinterpret_cast<double*>(f.data.p);
	a.noff = f.voff.p;
	a.nfirst = nfirst.p;
	a.tile_slot = tile_slot.p;
	a.slot_ids = g.slot_ids.p;
	a.recipe = drc.p;
	a.Nd = Nd;
	a.K = uint32_t(K);
	a.k0 = k0;
	a.k1 = k1;
	k_time_begin(g);
	particles_create_kernel<<<grid_for(tiles, 1, 1u << 16), kCB, 0, s>>>(g.m, G, a);
	HIP_CHECK(hipGetLastError());
	k_time_end(g);
	field_written(f);
	HIP_CHECK(hipStreamSynchronize(s));  // the offsets and the recipe go out of scope
	*created = N;
}

// ---------------------------------------------------------------------------
// Particles are removed on the device (dccrgx_particles_remove; DESIGN.md
// "Particles").  The local cells' records are the pool's first N and a cell's
// kept records keep their order, so the compacted local part is the stable
// compaction of those N records as one list: the kept records before record r
// are also the kept records before it in its cell plus those of the cells in
// front.  Record r lies in chunk r >> 6.
//   1. decide  - a thread per record (the step's record search names its
//                cell): mask, tests, chance, the rescale in place.  A wave's
//                ballot of the kept is the chunk's 64 bits, its popcount the
//                chunk's count; the verdicts are counted from ballots in the
//                wave's registers, one partial a wave of the grid;
//   2. a scan of the chunk counts: kept before r = scanned[r >> 6] +
//                popcount(bits[r >> 6] below bit r & 63), removed before r =
//                r - that.  Nothing removed: the call ends here;
//   3. tally   - a wave per local cell that loses a record: the lanes stride
//                its records, a butterfly adds the lanes, lane 0 writes;
//   4. offsets - a thread per slot: kept before the cell's first record times
//                the record size; a remote copy moves up by the removed bytes;
//                into_field's cells grow by what their cell loses (varfield's
//                re-lay puts their own records in front);
//   5. copy    - a thread per double of the N records, passes of kCB doubles:
//                a kept double to its rank in the fresh pool, a removed one
//                (into_field) behind the destination cell's own records, its
//                cell from the record search.  The remote copies' bytes
//                follow as one device copy, and the pool is swapped in.
namespace {

constexpr int kRT = 8;      // tests of one call
constexpr int kRTally = 4;  // tallies of one call

struct RTest {
	double lo, hi;
	int j, mode;  // the tested double; 0 keep inside, 1 drop inside
};

struct RArgs {
	double* pool;
	const uint32_t* ofirst;      // n_local + 1 record offsets of the local slots
	const uint32_t* chunk_slot;  // passes + 1 (pass_slots_kernel)
	const uint64_t* slot_ids;
	const double* M;             // the mask (nullptr: none)
	const double* F;             // prob_field (nullptr: none)
	const RTest* tests;
	uint64_t* kbits;             // per chunk: the kept
	uint32_t* kcnt;              // per chunk: their number
	uint32_t* part;              // per wave of the grid: removed by mask, by a test, by chance; rescaled
	size_t N;
	double prob;
	uint32_t K, k0, k1;
	int n_tests, chance;
	int wd;  // the double the kept are rescaled in (-1: none)
};

__global__ __launch_bounds__(kPB) void particles_remove_decide_kernel(const RArgs a) {
	__shared__ uint32_t s_off[kOffCache];
	const size_t passes = (a.N + kPB - 1) / kPB;
	uint32_t n1 = 0, n2 = 0, n3 = 0, ns = 0;  // the wave's counts (one atomic a wave and pass on one word took
	                                          // 6.9 of (a)'s 7.4 ms in particles_bench --remove)
	for (size_t t = blockIdx.x; t < passes; t += gridDim.x) {
		const size_t p = t * kPB + threadIdx.x;
		const OffsetWindow W = stage_offsets(a.ofirst, a.chunk_slot, t, s_off);
		int verdict = -1;  // no record
		bool scaled = false;
		if (p < a.N) {
			const size_t c = W.slot(uint32_t(p));
			double* rec = a.pool + p * a.K;
			verdict = 0;
			if (a.M && a.M[c] != 0.0) verdict = 1;
			for (int k = 0; k < a.n_tests && verdict == 0; k++) {
				const RTest T = a.tests[k];
				const double x = rec[T.j];
				const bool in = T.lo <= x && x < T.hi;
				if (in == (T.mode == 1)) verdict = 2;
			}
			if (a.chance && verdict == 0) {
				const double pc = a.F ? a.prob * a.F[c] : a.prob;
				const uint64_t id = a.slot_ids[c];
				uint32_t w[4];
				philox4x32_10(uint32_t(id), uint32_t(id >> 32), uint32_t(p) - W.at(c), 0xFFFFFFFEu, a.k0, a.k1, w);
				const double u = philox_uniform(w[0], w[1]);
				if (u < pc) {
					verdict = 3;
				} else if (a.wd >= 0 && pc > 0.0 && pc < 1.0) {
					const double rest = 1.0 - pc;
					rec[a.wd] = rec[a.wd] / rest;
					scaled = true;
				}
			}
		}
		const uint64_t kb = __ballot(verdict == 0);
		const uint64_t b1 = __ballot(verdict == 1), b2 = __ballot(verdict == 2), b3 = __ballot(verdict == 3);
		const uint64_t bs = __ballot(scaled);
		if ((threadIdx.x & 63u) == 0) {
			const size_t ch = t * (kPB >> 6) + (threadIdx.x >> 6);
			a.kbits[ch] = kb;
			a.kcnt[ch] = uint32_t(__popcll(kb));
		}
		n1 += uint32_t(__popcll(b1));
		n2 += uint32_t(__popcll(b2));
		n3 += uint32_t(__popcll(b3));
		ns += uint32_t(__popcll(bs));
	}
	if ((threadIdx.x & 63u) == 0) {
		uint32_t* part = a.part + 4 * (size_t(blockIdx.x) * (kPB >> 6) + (threadIdx.x >> 6));
		part[0] = n1;
		part[1] = n2;
		part[2] = n3;
		part[3] = ns;
	}
}

// the kept records in front of record r (r <= N: the chunk arrays have an
// entry past the last record's)
__device__ __forceinline__ uint32_t kept_before(const uint64_t* __restrict__ kbits, const uint32_t* __restrict__ kbase,
                                                uint32_t r) {
	const uint32_t b = r & 63u;
	return kbase[r >> 6] + uint32_t(__popcll(kbits[r >> 6] & ((1ull << b) - 1ull)));
}

// (read with unrolled constant indices only, see MArgs)
struct TArgs {
	int fu[kRTally], fv[kRTally];  // m_j = (q * record[fu[j]]) * record[fv[j]]; -1: 1.0
	double* out[kRTally];
	int n;
};

__global__ __launch_bounds__(kPB) void particles_remove_tally_kernel(const double* __restrict__ pool,
                                                                     const uint32_t* __restrict__ ofirst,
                                                                     const uint64_t* __restrict__ kbits,
                                                                     const uint32_t* __restrict__ kbase, size_t n_local,
                                                                     uint32_t K, int wd, const TArgs f) {
	const uint32_t lane = threadIdx.x & 63u;
	const size_t waves = size_t(gridDim.x) * (kPB >> 6);
	for (size_t c = blockIdx.x * size_t(kPB >> 6) + (threadIdx.x >> 6); c < n_local; c += waves) {
		const uint32_t r0 = ofirst[c], r1 = ofirst[c + 1];
		if (r1 - r0 == kept_before(kbits, kbase, r1) - kept_before(kbits, kbase, r0)) continue;  // the cell loses none
		double sum[kRTally] = {};
		for (uint32_t r = r0 + lane; r < r1; r += 64) {
			if ((kbits[r >> 6] >> (r & 63u)) & 1ull) continue;
			const double* rec = pool + size_t(r) * K;
			const double q = wd < 0 ? 1.0 : rec[wd];
#pragma unroll
			for (int j = 0; j < kRTally; j++) {
				if (j >= f.n) continue;
				const double u = f.fu[j] < 0 ? 1.0 : rec[f.fu[j]];
				const double v = f.fv[j] < 0 ? 1.0 : rec[f.fv[j]];
				const double qu = q * u;
				const double mj = qu * v;
				sum[j] = sum[j] + mj;
			}
		}
#pragma unroll
		for (int j = 0; j < kRTally; j++) {
			if (j >= f.n) continue;
			for (int o = 32; o > 0; o >>= 1) sum[j] = sum[j] + __shfl_xor(sum[j], o, 64);
			if (lane == 0) f.out[j][c] = f.out[j][c] + sum[j];
		}
	}
}

// the byte offsets after the call: var_field's (noff) and into_field's (inoff,
// nullptr: none)
__global__ void remove_offsets_kernel(const uint64_t* __restrict__ voff, const uint64_t* __restrict__ ivoff,
                                      const uint32_t* __restrict__ ofirst, const uint32_t* __restrict__ iofirst,
                                      const uint64_t* __restrict__ kbits, const uint32_t* __restrict__ kbase,
                                      size_t n_slots, size_t n_local, uint64_t rec, uint64_t removed,
                                      uint64_t* __restrict__ noff, uint64_t* __restrict__ inoff) {
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s <= n_slots; s += size_t(gridDim.x) * blockDim.x) {
		if (s <= n_local) {
			const uint32_t kr = kept_before(kbits, kbase, ofirst[s]);
			noff[s] = uint64_t(kr) * rec;
			if (inoff) inoff[s] = (uint64_t(iofirst[s]) + (ofirst[s] - kr)) * rec;
		} else {
			noff[s] = voff[s] - removed * rec;
			if (inoff) inoff[s] = ivoff[s] + removed * rec;
		}
	}
}

struct XArgs {
	const double* src;
	double *dst, *into;         // the fresh pool; into_field's re-laid pool
	const uint64_t* kbits;
	const uint32_t* kbase;
	const uint32_t* ofirst;     // n_local + 1, the source's record offsets
	const uint32_t* iofirst;    // n_local + 1, into_field's before the call
	const uint32_t* tile_slot;  // tiles + 1 (pass_slots_kernel)
	size_t Nd;                  // doubles of the local records
	uint32_t K;
};

// The removed records of cell c follow its own in into_field: there the new
// first record of c is iofirst[c] + (removed before ofirst[c]), so removed
// record r goes to iofirst[c + 1] + (removed before r).
template <bool kInto>
__global__ __launch_bounds__(kCB) void particles_remove_copy_kernel(const XArgs a) {
	__shared__ uint32_t s_off[kInto ? kOffCache : 1];
	const size_t tiles = (a.Nd + kCB - 1) / kCB;
	for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
		const size_t d0 = t * kCB;
		const size_t r0 = d0 / a.K;  // the same in every lane
		const uint32_t j0 = uint32_t(d0 - r0 * a.K);
		OffsetWindow W{};
		if constexpr (kInto) W = stage_offsets(a.ofirst, a.tile_slot, t, s_off);
		const size_t d = d0 + threadIdx.x;
		if (d >= a.Nd) continue;
		const uint32_t within = j0 + threadIdx.x;
		const uint32_t dr = within / a.K;
		const uint32_t j = within - dr * a.K;
		const uint32_t r = uint32_t(r0) + dr;
		const uint32_t kr = kept_before(a.kbits, a.kbase, r);
		if ((a.kbits[r >> 6] >> (r & 63u)) & 1ull) {
			a.dst[size_t(kr) * a.K + j] = a.src[d];
		} else if constexpr (kInto) {
			const size_t c = W.slot(r);
			a.into[(size_t(a.iofirst[c + 1]) + (r - kr)) * a.K + j] = a.src[d];
		}
	}
}

}  // namespace

void particles_remove(Grid& g, int fid, int K, const int* test_i, const double* test_d, int n_tests, int mask_fid,
                      int prob_fid, double prob, uint64_t seed, int rescale, int weight_double,
                      const int* tally_factors, const int* tally_fids, int n_tally, int into_fid, uint64_t stats[4]) {
	DX_REQUIRE(stats, "null pointer");
	DX_REQUIRE(g.initialized, "not initialized");
	Field& f = field(g, fid);
	DX_REQUIRE(f.var, "particles need a variable-size field (this one is fixed-size)");
	DX_REQUIRE(K >= 3, "a particle record has at least 3 doubles (the position)");
	DX_REQUIRE(n_tests >= 0 && n_tests <= kRT, "the number of tests must be 0 .. 8");
	DX_REQUIRE(!n_tests || (test_i && test_d), "null pointer");
	std::vector<RTest> tests(size_t(n_tests) + 1);  // (never empty: uploaded as it is)
	for (int t = 0; t < n_tests; t++) {
		RTest& T = tests[size_t(t)];
		T = RTest{test_d[2 * t], test_d[2 * t + 1], test_i[2 * t], test_i[2 * t + 1]};
		DX_REQUIRE(T.j >= 0 && T.j < K, "test " + std::to_string(t) + " names a double outside 0 .. record_doubles - 1");
		DX_REQUIRE(T.mode == 0 || T.mode == 1, "a test's mode must be 0 (keep inside) or 1 (drop inside)");
		DX_REQUIRE(!std::isnan(T.lo) && !std::isnan(T.hi), "a test's bound is NaN");
	}
	const double *M = nullptr, *F = nullptr;
	if (mask_fid != -1) M = reinterpret_cast<const double*>(fp64_cell_field(g, mask_fid, "mask_field").data.p);
	if (prob_fid != -1) F = reinterpret_cast<const double*>(fp64_cell_field(g, prob_fid, "prob_field").data.p);
	DX_REQUIRE(std::isfinite(prob), "prob must be finite");
	require_weight_double(K, weight_double, 3, "position");
	DX_REQUIRE(!rescale || weight_double != -1, "rescale needs a weight_double");
	DX_REQUIRE(n_tally >= 0 && n_tally <= kRTally, "the number of tallies must be 0 .. 4");
	DX_REQUIRE(!n_tally || (tally_factors && tally_fids), "null pointer");
	TArgs ta{};
	ta.n = n_tally;
	for (int j = 0; j < kRTally; j++) {
		ta.fu[j] = ta.fv[j] = -1;
		ta.out[j] = nullptr;
		if (j >= n_tally) continue;
		ta.fu[j] = tally_factors[2 * j];
		ta.fv[j] = tally_factors[2 * j + 1];
		for (int v : {ta.fu[j], ta.fv[j]})
			DX_REQUIRE(v == -1 || (v >= 3 && v < K),
			           "a tally factor must be -1 (1.0) or a double of the record past the position (3 <= factor < "
			           "record_doubles)");
		ta.out[j] = reinterpret_cast<double*>(fp64_cell_field(g, tally_fids[j], "a tally field").data.p);
		for (int i = 0; i < j; i++) DX_REQUIRE(tally_fids[i] != tally_fids[j], "two tallies share a field");
		DX_REQUIRE(tally_fids[j] != mask_fid && tally_fids[j] != prob_fid,
		           "a tally field is also the mask_field or the prob_field");
	}
	Field* fi = nullptr;
	if (into_fid != -1) {
		DX_REQUIRE(into_fid != fid, "into_field is the var_field itself");
		fi = &field(g, into_fid);
		DX_REQUIRE(fi->var, "into_field must be a variable-size field (this one is fixed-size)");
	}
	hipStream_t s = g.s_comp;
	const size_t ns = g.n_slots, nl = g.n_local;
	const uint64_t rec = uint64_t(K) * sizeof(double);
	const uint64_t limit = uint64_t(1) << 31;

	// the record offsets of the local slots; every local cell whole records
	DBuf<int32_t> flag;
	flag.alloc(1);
	auto local_records = [&](const Field& x, DBuf<uint32_t>& of) -> uint64_t {
		of.alloc(nl + 1);
		if (!x.voff.p) {
			HIP_CHECK(hipMemsetAsync(of.p, 0, (nl + 1) * sizeof(uint32_t), s));
			return 0;
		}
		const uint64_t n = var_total(x, nl, s) / rec;
		DX_REQUIRE(n < limit, "more than 2^31 particles on one process");
		HIP_CHECK(hipMemsetAsync(flag.p, 0, 4, s));
		launch_per_item(record_offsets_kernel, nl + 1, s, x.voff.p, nl + 1, rec, of.p, flag.p);
		int32_t bad = 0;
		d2h_small(&bad, flag.p, 4, s);
		DX_REQUIRE(!bad, "a cell's payload is not a multiple of 8 * record_doubles bytes");
		return n;
	};
	DBuf<uint32_t> ofirst, iofirst;
	uint64_t N = 0;
	if (ns && nl) {
		N = local_records(f, ofirst);
		if (fi) local_records(*fi, iofirst);
	}
	if (!N) {
		for (int k = 0; k < 4; k++) stats[k] = 0;
		return;
	}
	const uint64_t into_bytes = fi && fi->voff.p ? var_total(*fi, ns, s) : 0, into_all = into_bytes / rec;

	// 1. decide, 2. scan.  The rescale writes in place, so where into_field
	// could overflow the verdicts are counted once without it
	const size_t passes = (size_t(N) + kPB - 1) / kPB, chunks = passes * (kPB >> 6);
	DBuf<uint32_t> chunk_slot, kcnt, kbase;
	DBuf<uint64_t> kbits;
	DBuf<RTest> dtests;
	DBuf<uint32_t> part;
	DBuf<uint64_t> count;
	launch_pass_slots(ofirst.p, nl, size_t(N), passes, 0, chunk_slot, s);
	kbits.alloc(chunks + 1);
	kcnt.alloc(chunks + 1);
	kbase.alloc(chunks + 1);
	const unsigned nb = grid_for(passes, 1, 4096);
	part.alloc(size_t(nb) * (kPB >> 6) * 4);
	count.alloc(4);
	dtests.alloc(tests.size());
	h2d(dtests.p, tests.data(), tests.size() * sizeof(RTest), s);
	HIP_CHECK(hipMemsetAsync(kbits.p + chunks, 0, sizeof(uint64_t), s));
	RArgs a{};
	a.pool = reinterpret_cast<double*>(f.data.p);
	a.ofirst = ofirst.p;
	a.chunk_slot = chunk_slot.p;
	a.slot_ids = g.slot_ids.p;
	a.M = M;
	a.F = F;
	a.tests = dtests.p;
	a.kbits = kbits.p;
	a.kcnt = kcnt.p;
	a.part = part.p;
	a.N = size_t(N);
	a.prob = prob;
	a.K = uint32_t(K);
	a.k0 = uint32_t(seed);
	a.k1 = uint32_t(seed >> 32);
	a.n_tests = n_tests;
	a.chance = (prob_fid != -1 || prob != 0.0) ? 1 : 0;
	uint64_t hc[4] = {0, 0, 0, 0};
	uint64_t kept = 0;
	auto decide = [&](bool write) {
		a.wd = write && rescale ? weight_double : -1;
		k_time_begin(g);
		particles_remove_decide_kernel<<<nb, kPB, 0, s>>>(a);
		HIP_CHECK(hipGetLastError());
		k_time_end(g);
		sum_parts_kernel<<<1, 256, 0, s>>>(part.p, size_t(nb) * (kPB >> 6), count.p);
		HIP_CHECK(hipGetLastError());
		kept = scan_exclusive_u32(kcnt.p, kbase.p, chunks, s);
		d2h_small(hc, count.p, sizeof(hc), s);
	};
	const bool may_overflow = fi && into_all + N >= limit;
	decide(!may_overflow);
	const uint64_t removed = N - kept;
	if (may_overflow) {
		DX_REQUIRE(into_all + removed < limit, "more than 2^31 - 1 records in into_field afterwards");
		if (rescale) decide(true);
	}
	stats[0] = kept;
	for (int k = 0; k < 3; k++) stats[k + 1] = hc[k];
	if (!removed) {
		if (hc[3]) field_written(f);
		return;
	}

	// 3. the tallies, from the pool as it stands
	if (n_tally) {
		k_time_begin(g);
		particles_remove_tally_kernel<<<grid_for(nl, kPB >> 6, 1u << 20), kPB, 0, s>>>(a.pool, ofirst.p, kbits.p,
		                                                                               kbase.p, nl, a.K, weight_double, ta);
		HIP_CHECK(hipGetLastError());
		k_time_end(g);
		for (int j = 0; j < n_tally; j++) field_written(fixed_field(g, tally_fids[j]));
	}

	// 4. the new layouts
	DBuf<uint64_t> noff, inoff;
	noff.alloc(ns + 1);
	if (fi) {
		inoff.alloc(ns + 1);
		if (!fi->voff.p) var_reset(*fi, ns, s);
	}
	launch_per_item(remove_offsets_kernel, ns + 1, s, f.voff.p, fi ? fi->voff.p : nullptr, ofirst.p, iofirst.p, kbits.p,
	                kbase.p, ns, nl, rec, removed, noff.p, fi ? inoff.p : nullptr);
	const uint64_t old_total = var_total(f, ns, s), local_bytes = N * rec;
	const uint64_t total = old_total - removed * rec;
	DBuf<uint8_t> nd;
	nd.alloc(total + 1);
	if (fi) var_relay(*fi, ns, inoff, into_bytes + removed * rec, false, s);

	// 5. the copy; the remote copies' bytes behind the local part
	XArgs x{};
	x.src = a.pool;
	x.dst = reinterpret_cast<double*>(nd.p);
	x.into = fi ? reinterpret_cast<double*>(fi->data.p) : nullptr;
	x.kbits = kbits.p;
	x.kbase = kbase.p;
	x.ofirst = ofirst.p;
	x.iofirst = iofirst.p;
	x.Nd = size_t(N) * size_t(K);
	x.K = uint32_t(K);
	const size_t tiles = (x.Nd + kCB - 1) / kCB;
	DBuf<uint32_t> tile_slot;
	if (fi) {
		launch_pass_slots(ofirst.p, nl, size_t(N), tiles, size_t(K), tile_slot, s);
		x.tile_slot = tile_slot.p;
	}
	k_time_begin(g);
	if (fi)
		particles_remove_copy_kernel<true><<<grid_for(tiles, 1, 1u << 16), kCB, 0, s>>>(x);
	else
		particles_remove_copy_kernel<false><<<grid_for(tiles, 1, 1u << 16), kCB, 0, s>>>(x);
	HIP_CHECK(hipGetLastError());
	k_time_end(g);
	if (old_total > local_bytes)
		HIP_CHECK(hipMemcpyAsync(nd.p + kept * rec, f.data.p + local_bytes, old_total - local_bytes,
		                         hipMemcpyDeviceToDevice, s));
	HIP_CHECK(hipStreamSynchronize(s));
	f.data.swap(nd);
	f.voff.swap(noff);
	field_written(f);
	if (fi) field_written(*fi);
}

}  // namespace dccrgx
