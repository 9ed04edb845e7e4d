// The advection solver's kernels beside the sweep (tests/advection of the
// reference): the time-step bound (solve.hpp:289-333), check_for_adaptation
// (adapter.hpp:47-178: max_diff, candidates, bands, requests) and adapt_grid
// (adapter.hpp:260-305: merged parents, velocity and length reset), with
// their launchers.  The driver is advection.hip, the sweeps advection_sweep.hip.
#include <cstdlib>
#include <cstring>

#include "dccrgx_internal.hpp"

namespace dccrgx {

namespace {

// max_time_step local part (solve.hpp:289-333): block minima
__global__ void adv_dt_kernel(const double* __restrict__ vx, const double* __restrict__ vy,
                              const double* __restrict__ vz, const double* __restrict__ lx,
                              const double* __restrict__ ly, const double* __restrict__ lz, size_t n,
                              double* partial) {
	__shared__ double red[256];
	double mn = 1.7976931348623157e308;
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x) {
		const double a = lx[s] / fabs(vx[s]), b = ly[s] / fabs(vy[s]), c = lz[s] / fabs(vz[s]);
		if (__builtin_isnormal(a)) mn = fmin(mn, a);
		if (__builtin_isnormal(b)) mn = fmin(mn, b);
		if (__builtin_isnormal(c)) mn = fmin(mn, c);
	}
	red[threadIdx.x] = mn;
	__syncthreads();
	for (int k = blockDim.x / 2; k > 0; k >>= 1) {
		if (threadIdx.x < k) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + k]);
		__syncthreads();
	}
	if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// the minimum of n partial minima into out[0] (one block; fmin is exact, so
// the order does not matter)
__global__ __launch_bounds__(256) void min_partials_kernel(const double* __restrict__ part, size_t n,
                                                           double* __restrict__ out) {
	__shared__ double red[256];
	double mn = 1.7976931348623157e308;
	for (size_t i = threadIdx.x; i < n; i += 256) mn = fmin(mn, part[i]);
	red[threadIdx.x] = mn;
	__syncthreads();
	for (int k = 128; k > 0; k >>= 1) {
		if (int(threadIdx.x) < k) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + k]);
		__syncthreads();
	}
	if (threadIdx.x == 0) out[0] = red[0];
}

// max_diff of check_for_adaptation (tests/advection/adapter.hpp:47-123) of
// one local cell over the fixed-width face table: the largest relative
// density difference over its face neighbors whose transverse offsets are
// zero (the x, y, z offset test of 84-102, the same from either side of a
// face): a same-size neighbor always counts, a coarser one only when the
// cell sits at the corner of the coarser cell's face, of four finer ones only
// the first (the one at the cell's corner); lvl8: the level of every slot
__device__ double adv_max_diff(MapCtx m, const double* __restrict__ rho, const int32_t* __restrict__ ell,
                               const int32_t* __restrict__ fine, const uint8_t* __restrict__ lvl8,
                               const uint64_t* __restrict__ slot_ids, size_t s, double diff_threshold, int& lvl) {
	typedef int i2v __attribute__((ext_vector_type(2)));
	const unsigned lv = lvl8[s];
	lvl = int(lv & 31u);
	const unsigned oct = lv >> 5;
	int32_t e6[6];
	const i2v* ev = reinterpret_cast<const i2v*>(ell + 6 * s);
#pragma unroll
	for (int j = 0; j < 3; j++) {
		const i2v v = ev[j];
		e6[2 * j] = v.x;
		e6[2 * j + 1] = v.y;
	}
	const double a = rho[s];
	double md = 0;
#pragma unroll
	for (int dir = 0; dir < 6; dir++) {
		const int32_t e = e6[dir];
		if (e == -1) continue;
		int32_t nsl;
		if (e >= 0) {
			nsl = e;
			// coarser: only when the cell sits at the corner of its face
			if (int(lvl8[e] & 31u) < lvl && (oct & ~(1u << (dir >> 1))) != 0) continue;
		} else {
			nsl = fine[4 * size_t(-2 - e)];
		}
		const double b = rho[nsl];
		const double diff = fabs(a - b) / (fmin(a, b) + diff_threshold);
		md = fmax(diff, md);
	}
	return md;
}

__global__ void adv_candidates_kernel(MapCtx m, const double* __restrict__ rho, const int32_t* __restrict__ ell,
                                      const int32_t* __restrict__ fine, const uint8_t* __restrict__ lvl8,
                                      const uint64_t* __restrict__ slot_ids, size_t n,
                                      double diff_increase, double diff_threshold, uint64_t* out,
                                      unsigned long long* counter) {
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x) {
		int lvl;
		const double md = adv_max_diff(m, rho, ell, fine, lvl8, slot_ids, s, diff_threshold, lvl);
		if (md > (lvl + 1) * diff_increase) out[atomicAdd(counter, 1ull)] = slot_ids[s];
	}
}

// the band of each local cell (adapter.hpp:124-176): 2 refine, 1 keep (no
// unrefine), 0 unrefine
__global__ void adv_bands_kernel(MapCtx m, const double* __restrict__ rho, const int32_t* __restrict__ ell,
                                 const int32_t* __restrict__ fine, const uint8_t* __restrict__ lvl8,
                                 const uint64_t* __restrict__ slot_ids, size_t n,
                                 double diff_increase, double diff_threshold, double unrefine_sensitivity,
                                 uint8_t* __restrict__ band) {
#pragma clang fp contract(off)
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x) {
		int lvl;
		const double md = adv_max_diff(m, rho, ell, fine, lvl8, slot_ids, s, diff_threshold, lvl);
		const double refine_diff = (lvl + 1) * diff_increase, unrefine_diff = unrefine_sensitivity * refine_diff;
		band[s] = md > refine_diff ? 2 : (md >= unrefine_diff ? 1 : 0);
	}
}

// the requests check_for_adaptation issues from the bands (adapter.hpp:
// 124-176), per local slot on Morton-ordered slots: a refine request for a
// band-2 leaf below the maximum level; per family (a run of consecutive slots
// with one parent, level > 0) headed at this slot: all 8 members here -> kept
// when any member's band is >= 1, else one unrefine request; fewer -> the
// run goes to the host, which merges the runs of a parent (families split
// between runs or processes).  Lists are appended through counters
// cnt[0] refines, cnt[1] unrefines, cnt[2] kept families, cnt[3] partial runs.
//
// Coalesced: a wave covers 64 x kJ consecutive slots, lane l taking slots
// base + 64 j + l (j < kJ) and the tail chunk base + 64 kJ + l (the runs that
// start in the last chunk reach up to 7 slots past it); the neighbors'
// parents and bands come from the other lanes by shuffles (slot + q is lane
// l + q of the same chunk, or of the next one past lane 63).  List positions
// are reserved per block (block_reserve4).  Every id and band load is issued
// before the parents are computed.  (Round 5: 282 -> 136 us a config-3 step,
// of which the per-block reservation took 277 -> 191, the solo shortcut
// 191 -> 165 and lane-uniform MapCtx reads the rest)
// Positions in the four request lists for a block of W waves: one atomic per
// block and list (per-wave atomics on the same four counters serialise at the
// device-coherent level - 4 x ~17000 of them a config-3 step).  c and the
// result in counter order: refine, unrefine, kept, partial.
template <int W>
__device__ __forceinline__ void block_reserve4(unsigned long long* __restrict__ cnt, const unsigned c[4],
                                               unsigned long long out[4]) {
	__shared__ unsigned tot[W][4];
	__shared__ unsigned long long at[W][4];
	const int lane = int(threadIdx.x & 63u), w = int(threadIdx.x >> 6);
	unsigned incl[4];
#pragma unroll
	for (int k = 0; k < 4; k++) {
		incl[k] = c[k];
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const unsigned v = __shfl_up(incl[k], d, 64);
			if (lane >= d) incl[k] += v;
		}
		if (lane == 63) tot[w][k] = incl[k];
	}
	__syncthreads();
	if (threadIdx.x < 4) {
		const int k = int(threadIdx.x);
		unsigned run = 0;
		for (int v = 0; v < W; v++) run += tot[v][k];
		unsigned long long b = run ? atomicAdd(&cnt[k], static_cast<unsigned long long>(run)) : 0ull;
		for (int v = 0; v < W; v++) {
			at[v][k] = b;
			b += tot[v][k];
		}
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < 4; k++) out[k] = at[w][k] + (incl[k] - c[k]);
}

// solo: every cell of the grid is local and the slots are in Morton order, so
// a family's leaves are one run and a partial run (k < 8) always has a
// sibling with children - no lookups needed to know it.
template <int BS>
__global__ __launch_bounds__(BS) void adv_requests_kernel(MapCtx m, DevMesh M, const uint64_t* __restrict__ ids,
                                                               const uint8_t* __restrict__ band, size_t n, bool solo,
                                                               int rank, uint64_t* __restrict__ ref, uint64_t* __restrict__ unref,
                                                               uint32_t* __restrict__ part,
                                                               unsigned long long* __restrict__ cnt) {
	constexpr int kJ = 8;
	constexpr int kSpan = BS * kJ;  // a block's slots: wave w takes [64 kJ w, 64 kJ (w + 1))
	// the parents (~0: level 0 or none) and bands of the block's slots, of
	// the slot before them and of the seven after them (entry i = slot
	// base0 + i - 1): a run head reads its run from here, every other slot
	// only its predecessor (round 5's form shuffled all seven neighbors of
	// every slot)
	__shared__ uint64_t sp[kSpan + 8];
	__shared__ uint8_t sb[kSpan + 8];
	const size_t base0 = size_t(blockIdx.x) * kSpan;
	for (int i = int(threadIdx.x); i < kSpan + 8; i += BS) {
		const bool ok = (base0 + size_t(i) >= 1) && base0 + size_t(i) - 1 < n;
		const uint64_t id = ok ? ids[base0 + size_t(i) - 1] : 0;
		sp[i] = map_level(m, id) > 0 ? map_parent(m, id) : ~uint64_t(0);
		sb[i] = ok ? band[base0 + size_t(i) - 1] : uint8_t(0);
	}
	__syncthreads();
	const int lane = int(threadIdx.x & 63u);
	const int w = int(threadIdx.x >> 6);
	uint32_t flags = 0;  // per j, 4 bits: 1 refine, 2 partial run head, 4 kept family head, 8 unrefine head
	uint32_t runk = 0;   // per j, 4 bits: the run length of a partial run head
	unsigned cr = 0, cp = 0, ck = 0, cu = 0;
#pragma unroll
	for (int j = 0; j < kJ; j++) {
		const int li = 64 * kJ * w + 64 * j + lane;  // block-local slot; its entries li + 1 (own), li (before)
		const size_t sj = base0 + size_t(li);
		if (sj >= n) continue;
		const uint64_t p = sp[li + 1];
		const uint64_t prev = sp[li];
		const uint32_t bj = sb[li + 1];
		const int lvl = p == ~uint64_t(0) ? 0 : map_level(m, p) + 1;
		uint32_t what = 0;
		if (bj == 2 && lvl < int(m.R)) {
			what |= 1;
			cr++;
		}
		if (lvl > 0 && prev != p) {
			uint32_t k = 1;
			bool keep = bj >= 1;
			for (int q = 1; q < 8; q++) {
				if (sp[li + 1 + q] != p) break;
				keep = keep || sb[li + 1 + q] >= 1;
				k++;
			}
			bool whole = !solo;  // every child of p is a leaf (some held elsewhere)
			// every child of p a local leaf (a family split between the inner
			// and outer runs): decided here, by the run headed by the first child
			// (-1: not local, 1: this run decides, 2: another run does)
			int local = 0;
			bool keep8 = false;
			if (k < 8 && whole) {
				// the slot just before or just after the run holding a child of a
				// sibling (a grandchild of p) settles it without lookups
				const uint64_t after = sp[li + 1 + int(k)];
				auto grandchild_of_p = [&](uint64_t par_of_slot) {
					return par_of_slot != ~uint64_t(0) && map_level(m, par_of_slot) > 0 && map_parent(m, par_of_slot) == p;
				};
				if (grandchild_of_p(prev) || grandchild_of_p(after)) whole = false;
			}
			if (k < 8 && whole) {
				uint64_t ch[8];
				map_all_children(m, p, ch);
				local = 1;
				for (int i = 0; i < 8; i++) {
					int32_t o = -1, sl = -1;
					if (!dm_lookup(M, ch[i], o, sl)) {
						whole = false;
						break;
					}
					if (o != rank || sl < 0 || size_t(sl) >= n) local = -1;
					else keep8 = keep8 || band[sl] >= 1;
				}
				if (local == 1 && ids[sj] != ch[0]) local = 2;
			}
			if (k < 8 && whole && local == 2) {
				// counted by the run of the first child
			} else if (k < 8 && whole && local == 1) {
				// 2679-2733 as decide() on the host: a kept family is counted, a
				// whole local family not kept is unrefined (its first child's id)
				if (keep8) ck++;
				else {
					what |= 8;
					cu++;
				}
			} else if (k < 8 && !whole) {
				// a sibling has children: the family cannot be unrefined in
				// this round (unrefine_completely refuses, a dont_unrefine mark
				// changes nothing), so the host never sees it; counted as the
				// host's decide() would count it
				if (keep) ck++;
			} else if (k < 8) {
				what |= 2;
				runk |= k << (4 * j);
				cp++;
			} else if (keep) {
				ck++;
			} else {
				what |= 8;
				cu++;
			}
		}
		flags |= what << (4 * j);
	}
	const unsigned c[4] = {cr, cu, ck, cp};
	unsigned long long b[4];
	block_reserve4<BS / 64>(cnt, c, b);
	unsigned long long ar = b[0], au = b[1], ap = b[3];
#pragma unroll
	for (int j = 0; j < kJ; j++) {
		const uint32_t what = (flags >> (4 * j)) & 15u;
		if (!what) continue;
		const size_t sj = base0 + size_t(64 * kJ * w + 64 * j + lane);
		if (what & 1) ref[ar++] = ids[sj];
		if (what & 2) part[ap++] = uint32_t(sj) | (((runk >> (4 * j)) & 15u) << 28);
		if (what & 8) unref[au++] = ids[sj];
	}
}

__global__ void gather_ids_bands_kernel(const uint64_t* __restrict__ ids, const uint8_t* __restrict__ band,
                                        const uint32_t* __restrict__ at, size_t n, uint64_t* __restrict__ oid,
                                        uint8_t* __restrict__ ob) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		oid[i] = ids[at[i]];
		ob[i] = band[at[i]];
	}
}

// adapt_grid (adapter.hpp:294-305): velocity (solve.hpp:336-342) and lengths
// (Cartesian_Geometry get_center / get_length, dccrg_cartesian_geometry.hpp:
// 282-362) of every local cell
// (+ the block minima of adv_dt_kernel's bound over the values written, when
// dt_partial is given: the next max_time_step needs no pass of its own).
// STRETCHED: center and lengths are Stretched_Cartesian_Geometry's
// (dccrg_stretched_cartesian_geometry.hpp:298-403, geometry_fill_kernel's
// expressions) from the packed coordinates G.
template <bool STRETCHED>
__global__ __launch_bounds__(256) void adv_reset_kernel(MapCtx m, const uint64_t* __restrict__ slot_ids, size_t n,
                                                        double s0, double s1, double l00, double l01, double l02,
                                                        StretchedView G, double* vx, double* vy, double* vz,
                                                        double* lx, double* ly, double* lz, double* dt_partial) {
#pragma clang fp contract(off)
	__shared__ double red[256];
	const double st[3] = {s0, s1, 0.0};
	const double l0[3] = {l00, l01, l02};
	double mn = 1.7976931348623157e308;
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x) {
		uint64_t ind[3];
		const int lvl = map_indices(m, slot_ids[s], ind[0], ind[1], ind[2]);
		const double sf = 1.0 / double(uint64_t(1) << lvl);
		double L[3], c[2];
		if constexpr (STRETCHED) {
			const uint64_t l0i = uint64_t(1) << m.R;
			for (int d = 0; d < 3; d++) {
				const uint64_t i0 = ind[d] / l0i;
				const double c0 = G.c[G.off[d] + i0];
				const double extent = G.c[G.off[d] + i0 + 1] - c0;
				L[d] = extent / double(uint64_t(1) << lvl);
				if (d < 2) {
					const double length_of_index = extent / double(l0i);
					const double in_cell = length_of_index * double(ind[d] - i0 * l0i);
					const double low = c0 + in_cell;
					c[d] = low + L[d] / 2;
				}
			}
		} else {
			for (int d = 0; d < 3; d++) L[d] = l0[d] * sf;
			for (int d = 0; d < 2; d++) c[d] = st[d] + double(ind[d]) * l0[d] / double(uint64_t(1) << m.R) + L[d] / 2;
		}
		const double v[3] = {-c[1] + 0.5, +c[0] - 0.5, 0.0};
		vx[s] = v[0];
		vy[s] = v[1];
		vz[s] = v[2];
		lx[s] = L[0];
		ly[s] = L[1];
		lz[s] = L[2];
		if (dt_partial) {
			// adv_dt_kernel's expression on the same values
			const double a = L[0] / fabs(v[0]), b = L[1] / fabs(v[1]), cc = L[2] / fabs(v[2]);
			if (__builtin_isnormal(a)) mn = fmin(mn, a);
			if (__builtin_isnormal(b)) mn = fmin(mn, b);
			if (__builtin_isnormal(cc)) mn = fmin(mn, cc);
		}
	}
	if (!dt_partial) return;  // grid-uniform
	red[threadIdx.x] = mn;
	__syncthreads();
	for (int k = blockDim.x / 2; k > 0; k >>= 1) {
		if (threadIdx.x < k) red[threadIdx.x] = fmin(red[threadIdx.x], red[threadIdx.x + k]);
		__syncthreads();
	}
	if (threadIdx.x == 0) dt_partial[blockIdx.x] = red[0];
}

}  // namespace

void k_adv_dt(const double* const f[7], size_t n, double* partial, size_t nblocks, hipStream_t s) {
	adv_dt_kernel<<<unsigned(nblocks), 256, 0, s>>>(f[1], f[2], f[3], f[4], f[5], f[6], n, partial);
	HIP_CHECK(hipGetLastError());
}

void k_min_partials(const double* partial, size_t n, double* out, hipStream_t s) {
	min_partials_kernel<<<1, 256, 0, s>>>(partial, n, out);
	HIP_CHECK(hipGetLastError());
}

void k_adv_bands(const MapCtx& m, const double* rho, const FaceView& F, const uint8_t* lvl8, size_t n,
                 double diff_increase, double diff_threshold, double unrefine_sensitivity, uint8_t* band,
                 hipStream_t s) {
	launch_per_item(adv_bands_kernel, n, s, m, rho, F.ell, F.fine, lvl8, F.slot_ids, n, diff_increase,
	                diff_threshold, unrefine_sensitivity, band);
}

// adapt_grid's merged parents (adapter.hpp:260-290) from the removed store's
// ids `rm` (store order): parents grouped, their eight children in ascending
// id, the parents' local slots, then the mean density
void k_adv_merge_parents(const MapCtx& m, const DevMesh& dm, size_t n_local, LazyIds& rm, double* rho,
                         const double* removed_rho, hipStream_t s, const uint64_t* parents, size_t np_given) {
	if (rm.empty()) return;
	// the rows and the kernel of the fields that follow the mesh
	// (field_adapt.hip): one copy of the mean's arithmetic
	DBuf<int32_t> cidx, pslot;
	const size_t np = k_merged_rows(m, dm, n_local, rm, parents, np_given, cidx, pslot, s);
	FollowSet F;
	F.n = 1;
	F.data[0] = rho;
	F.removed[0] = removed_rho;
	F.mode[0] = DCCRGX_FOLLOW_MEAN;
	k_field_merge_parents(F, pslot.p, cidx.p, np, s);
}

static void k_gather_ids_bands(const uint64_t* ids, const uint8_t* band, const uint32_t* at, size_t n, uint64_t* oid,
                               uint8_t* ob, hipStream_t s) {
	gather_ids_bands_kernel<<<grid_for(n, 256), 256, 0, s>>>(ids, band, at, n, oid, ob);
	HIP_CHECK(hipGetLastError());
}

AdvRequests k_adv_requests(const MapCtx& m, const DevMesh& dm, const uint64_t* slot_ids, const uint8_t* band, size_t n,
                           bool solo, int rank, hipStream_t s) {
	AdvRequests out;
	if (!n) return out;
	DX_REQUIRE(n < (size_t(1) << 28), "too many local cells for the request runs");
	DBuf<uint64_t> ref, unref;
	DBuf<uint32_t> part;
	DBuf<unsigned long long> cnt;
	ref.alloc(n);
	unref.alloc(n / 8 + 1);
	part.alloc(n);
	cnt.alloc(4);
	HIP_CHECK(hipMemsetAsync(cnt.p, 0, 4 * sizeof(unsigned long long), s));
	// 512 threads (4096 slots, 37 KB of LDS, four blocks per CU): a config-3
	// step's ~2100 blocks end in a shorter partial last round than 1024's
	// ~1050 two-per-CU blocks (122 -> 92 us; r06zj_requests_bs_ab.txt).
	// DCCRGX_REQ_BS=256 / 1024: the other sizes measured
	const char* rb = std::getenv("DCCRGX_REQ_BS");
	const int bs = rb && *rb ? std::atoi(rb) : 512;
	if (bs == 256)
		adv_requests_kernel<256><<<unsigned((n + 256 * 8 - 1) / (256 * 8)), 256, 0, s>>>(m, dm, slot_ids, band, n, solo,
		                                                                                rank, ref.p, unref.p, part.p, cnt.p);
	else if (bs == 512)
		adv_requests_kernel<512><<<unsigned((n + 512 * 8 - 1) / (512 * 8)), 512, 0, s>>>(m, dm, slot_ids, band, n, solo,
		                                                                                rank, ref.p, unref.p, part.p, cnt.p);
	else
		adv_requests_kernel<1024><<<unsigned((n + 1024 * 8 - 1) / (1024 * 8)), 1024, 0, s>>>(m, dm, slot_ids, band, n, solo,
		                                                                                    rank, ref.p, unref.p, part.p, cnt.p);
	HIP_CHECK(hipGetLastError());
	unsigned long long h[4];
	d2h_small(h, cnt.p, sizeof(h), s);
	// ascending ids (the lists the host merges and stop_refining sorts), sorted
	// here before they leave the device
	sort_u64(ref.p, size_t(h[0]), s, map_id_bits(m));
	sort_u64(unref.p, size_t(h[1]), s, map_id_bits(m));
	// the three lists gathered on the device and read at once
	const size_t b0 = 8 * size_t(h[0]), b1 = 8 * size_t(h[1]), b3 = 4 * size_t(h[3]);
	std::vector<uint32_t> runs(static_cast<size_t>(h[3]));
	out.refine.resize(size_t(h[0]));
	out.unrefine.resize(size_t(h[1]));
	if (b0 + b1 + b3) {
		DBuf<uint8_t> stage;
		stage.alloc(b0 + b1 + b3);
		if (b0) HIP_CHECK(hipMemcpyAsync(stage.p, ref.p, b0, hipMemcpyDeviceToDevice, s));
		if (b1) HIP_CHECK(hipMemcpyAsync(stage.p + b0, unref.p, b1, hipMemcpyDeviceToDevice, s));
		if (b3) HIP_CHECK(hipMemcpyAsync(stage.p + b0 + b1, part.p, b3, hipMemcpyDeviceToDevice, s));
		const std::vector<uint8_t> hb = download(stage.p, b0 + b1 + b3, s);
		if (b0) std::memcpy(out.refine.data(), hb.data(), b0);
		if (b1) std::memcpy(out.unrefine.data(), hb.data() + b0, b1);
		if (b3) std::memcpy(runs.data(), hb.data() + b0 + b1, b3);
	}
	out.refine_dev = std::move(ref);
	out.unrefine_dev = std::move(unref);
	out.kept = size_t(h[2]);
	// the partial runs' members: ids and bands
	for (uint32_t r : runs) {
		const size_t s0 = r & ((1u << 28) - 1u), k = r >> 28;
		out.part_slot.push_back(s0);
		out.part_len.push_back(uint32_t(k));
	}
	if (!runs.empty()) {
		std::vector<uint32_t> mem;
		for (size_t i = 0; i < out.part_slot.size(); i++)
			for (uint32_t j = 0; j < out.part_len[i]; j++) mem.push_back(uint32_t(out.part_slot[i] + j));
		DBuf<uint32_t> dm;
		upload(dm, mem, s);
		DBuf<uint64_t> gid;
		DBuf<uint8_t> gb;
		gid.alloc(mem.size());
		gb.alloc(mem.size());
		k_gather_ids_bands(slot_ids, band, dm.p, mem.size(), gid.p, gb.p, s);
		out.part_ids = download(gid.p, mem.size(), s);
		out.part_bands = download(gb.p, mem.size(), s);
	}
	return out;
}

size_t k_adv_reset(const MapCtx& m, const uint64_t* slot_ids, size_t n, const double start[3], const double l0[3],
                   const StretchedView& G, double* const f[7], hipStream_t s, double* dt_partial) {
	if (!n) return 0;
	const unsigned nb = grid_for(n, 256, kDtPartials);
	if (G.c)
		adv_reset_kernel<true><<<nb, 256, 0, s>>>(m, slot_ids, n, start[0], start[1], l0[0], l0[1], l0[2], G, f[1], f[2],
		                                          f[3], f[4], f[5], f[6], dt_partial);
	else
		adv_reset_kernel<false><<<nb, 256, 0, s>>>(m, slot_ids, n, start[0], start[1], l0[0], l0[1], l0[2], G, f[1], f[2],
		                                           f[3], f[4], f[5], f[6], dt_partial);
	HIP_CHECK(hipGetLastError());
	return nb;
}

size_t k_adv_candidates(const MapCtx& m, const double* rho, const FaceView& F, const uint8_t* lvl8, size_t n,
                        double diff_increase, double diff_threshold, uint64_t* out, hipStream_t s) {
	if (!n) return 0;
	DevCounter ctr;
	adv_candidates_kernel<<<grid_for(n, 256), 256, 0, s>>>(m, rho, F.ell, F.fine, lvl8, F.slot_ids, n, diff_increase,
	                                                       diff_threshold, out, ctr.zero(s));
	HIP_CHECK(hipGetLastError());
	return ctr.read(s);
}

}  // namespace dccrgx
