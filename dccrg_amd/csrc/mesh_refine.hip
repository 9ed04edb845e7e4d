// The ghost region around the local cells, and the refinement closure
// (override_unrefines dccrg.hpp:9796-9898, execute_refines 10104-10554).
#include <cstring>

#include "dccrgx_internal.hpp"
#include "dccrgx_wave.hpp"

namespace dccrgx {

namespace {

__device__ __forceinline__ bool sorted_has(const uint64_t* a, size_t n, uint64_t v) {
	size_t lo = 0, hi = n;
	while (lo < hi) {
		const size_t mid = (lo + hi) >> 1;
		if (a[mid] < v) lo = mid + 1;
		else hi = mid;
	}
	return lo < n && a[lo] == v;
}

// ---- ghost region ---------------------------------------------------------------
// (level-0 parent, volume in finest-level cells) of every local cell
__global__ void l0_volume_kernel(MapCtx m, const uint64_t* ids, size_t n, uint64_t* l0, uint64_t* vol) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const int lvl = map_level(m, ids[i]);
		l0[i] = map_level0_parent(m, ids[i]);
		vol[i] = uint64_t(1) << (3 * (m.R - lvl));
	}
}

// keys-only hash set (wholly local level-0 cells): same probing as the mesh table
__global__ void keyset_insert_kernel(uint64_t* tab, uint64_t mask, uint32_t shift, const uint64_t* keys,
                                     const uint64_t* vals, uint64_t want, size_t n) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		if (vals && vals[i] != want) continue;
		const uint64_t id = keys[i];
		uint64_t h = hash_home(id, shift);
		for (;;) {
			const unsigned long long prev =
			    atomicCAS(reinterpret_cast<unsigned long long*>(tab + h), 0ull, (unsigned long long)id);
			if (prev == 0ull || prev == id) break;
			h = (h + 1) & mask;
		}
	}
}

struct KeySet {
	const uint64_t* tab;
	uint64_t mask;
	uint32_t shift;
	__device__ __forceinline__ bool has(uint64_t id) const {
		if (!tab) return false;
		uint64_t h = hash_home(id, shift);
		for (;;) {
			const uint64_t k = tab[h];
			if (k == id) return true;
			if (k == 0) return false;
			h = (h + 1) & mask;
		}
	}
};

// per distinct level-0 parent p of local cells: every level-0 cell q within
// Chebyshev distance `radius` (periodic wrap) that is not wholly local
// (full[] sorted; implicit grids: the block partition decides) is emitted
__global__ void ghost_l0_kernel(MapCtx m, DevMesh M, int rank, const uint64_t* par, size_t n, KeySet full,
                                int radius, uint64_t* out, unsigned long long* counter, unsigned long long cap) {
	MapCtx m0 = m;  // level-0 index space
	const int side = 2 * radius + 1;
	const int cube = side * side * side;
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		uint64_t x, y, z;
		map_indices(m, par[i], x, y, z);
		const int64_t len0 = int64_t(1) << m.R;
		const int64_t b[3] = {int64_t(x), int64_t(y), int64_t(z)};
		for (int k = 0; k < cube; k++) {
			const int dx = k % side - radius, dy = (k / side) % side - radius, dz = k / (side * side) - radius;
			uint64_t w[3];
			if (!map_wrap(m0, 0, b[0] + dx * len0, w[0]) || !map_wrap(m0, 1, b[1] + dy * len0, w[1]) ||
			    !map_wrap(m0, 2, b[2] + dz * len0, w[2]))
				continue;
			const uint64_t q = map_from_indices(m, w[0], w[1], w[2], 0);
			bool local_full;
			if (M.implicit) local_full = M.bp.owner(q) == rank;
			else local_full = full.has(q);
			if (local_full) continue;
			const unsigned long long pos = atomicAdd(counter, 1ull);
			if (pos < cap) out[pos] = q;
		}
	}
}

__global__ void cells_under_kernel(MapCtx m, const uint64_t* ids, size_t n, const uint64_t* l0, size_t nl0,
                                   uint64_t* out, unsigned long long* counter) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		if (sorted_has(l0, nl0, map_level0_parent(m, ids[i]))) out[atomicAdd(counter, 1ull)] = ids[i];
	}
}

}  // namespace

std::vector<uint64_t> k_ghost_level0(const MapCtx& m, const DevMesh& M, int rank, const uint64_t* local, size_t n,
                                     int radius, hipStream_t s) {
	if (!n) return {};
	// distinct level-0 parents of the local cells; the wholly local ones
	// (leaf volume 8^R) in a keys-only hash set.  Implicit grids: every local
	// cell is a level-0 cell and the block partition tells what is local.
	DBuf<uint64_t> uk, uv, set;
	const uint64_t* par = local;
	size_t np = n;
	KeySet ks{nullptr, 0, 63};
	if (!M.implicit) {
		DBuf<uint64_t> l0, vol, l0s, vols;
		l0.alloc(n);
		vol.alloc(n);
		l0s.alloc(n);
		vols.alloc(n);
		uk.alloc(n);
		uv.alloc(n);
		launch_per_item(l0_volume_kernel, n, s, m, local, n, l0.p, vol.p);
		DevCounter nu;
		nu.word();
		with_temp(cub_sort_pairs(l0.p, l0s.p, vol.p, vols.p, n, 64, s),
		          cub_sum_by_key(l0s.p, uk.p, vols.p, uv.p, nu.d.p, n, s));
		np = nu.read(s);
		par = uk.p;
		uint32_t bits = 4;
		while ((uint64_t(1) << bits) < 2 * np) bits++;
		set.alloc(size_t(1) << bits);
		HIP_CHECK(hipMemsetAsync(set.p, 0, set.n * 8, s));
		ks = KeySet{set.p, set.n - 1, 64u - bits};
		launch_per_item(keyset_insert_kernel, np, s, set.p, ks.mask, ks.shift, uk.p, uv.p,
		                uint64_t(1) << (3 * m.R), np);
	}
	return collect_sorted_unique(size_t(1) << 22, map_id_bits(m), s,
	                             [&](uint64_t* out, unsigned long long* ctr, unsigned long long cap) {
		                             ghost_l0_kernel<<<grid_for(np, 256), 256, 0, s>>>(m, M, rank, par, np, ks, radius, out,
		                                                                               ctr, cap);
	                             });
}

std::vector<uint64_t> k_cells_under(const MapCtx& m, const uint64_t* local, size_t n, const std::vector<uint64_t>& l0,
                                    hipStream_t s) {
	if (!n || l0.empty()) return {};
	DBuf<uint64_t> dl0, out;
	upload(dl0, l0, s);
	out.alloc(n);
	DevCounter ctr;
	launch_per_item(cells_under_kernel, n, s, m, local, n, dl0.p, l0.size(), out.p, ctr.zero(s));
	const size_t k = ctr.read(s);
	sort_u64(out.p, k, s, map_id_bits(m));
	return download(out.p, k, s);
}

// ---- refinement -------------------------------------------------------------------
// (k_induced_refines walks the stencil items: neighbor_build.hip)
namespace {
// override_unrefines (9796-9898): the family under parent p (children of
// level L) may merge only if no leaf in p's neighborhood is finer than L and
// none of level L is being refined.  The reference walks the face-neighbor
// graph from the unrefined cell while is_neighbor(p, .) holds; the leaves it
// reaches are the ones inside p's neighborhood boxes, checked here box by
// box: a box covered by one leaf of p's level or coarser passes, otherwise
// each of its eight level-L cells must be a leaf that is not being refined.
__global__ void unrefine_check_kernel(MapCtx m, const int32_t* hood, int nh, DevMesh M, const uint64_t* parents,
                                      size_t n, const uint64_t* S, size_t nS, uint32_t* ok) {
	// one thread per (parent, neighborhood box); ok starts 1, a failing box
	// clears it
	const DevExists ex{M};
	for (size_t t = blockIdx.x * size_t(blockDim.x) + threadIdx.x; t < n * size_t(nh); t += size_t(gridDim.x) * blockDim.x) {
		const size_t i = t / size_t(nh);
		const int k = int(t - i * size_t(nh));
		uint64_t c[3];
		int pl;
		cell_coords(m, parents[i], c, pl);
		const int64_t len = int64_t(1) << (m.R - pl);
		uint64_t w[3];
		bool inside = true;
		for (int d = 0; d < 3; d++) inside = inside && map_wrap(m, d, int64_t(c[d]) + int64_t(hood[3 * k + d]) * len, w[d]);
		if (!inside) continue;
		bool covered = false;
		for (int l = pl; l >= 0 && !covered; l--) covered = ex(map_from_indices(m, w[0], w[1], w[2], l));
		if (covered) continue;
		const uint64_t hl = uint64_t(len / 2);
		bool good = true;
		for (int q = 0; q < 8 && good; q++) {
			const uint64_t id = map_from_indices(m, w[0] + (q & 1) * hl, w[1] + ((q >> 1) & 1) * hl,
			                                     w[2] + ((q >> 2) & 1) * hl, pl + 1);
			if (!ex(id) || sorted_has(S, nS, id)) good = false;
		}
		if (!good) ok[i] = 0;
	}
}

// override_unrefines' candidates (9796-9898): the parents of the requested
// cells (level-0 cells have none: ~0, dropped by the sort)
__global__ void request_parents_kernel(MapCtx m, const uint64_t* req, size_t n, uint64_t* par) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t c = req[i];
		par[i] = map_level(m, c) > 0 ? map_parent(m, c) : ~uint64_t(0);
	}
}

// a family is blocked when one of its children is being refined or is
// marked dont_unrefine
__global__ void family_blocked_kernel(MapCtx m, const uint64_t* cand, size_t n, const uint64_t* S, size_t nS,
                                      const uint64_t* DU, size_t nDU, uint32_t* ok) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		uint64_t ch[8];
		map_all_children(m, cand[i], ch);
		bool blocked = false;
		for (int k = 0; k < 8; k++) blocked = blocked || sorted_has(S, nS, ch[k]) || sorted_has(DU, nDU, ch[k]);
		if (blocked) ok[i] = 0;
	}
}
}  // namespace

std::vector<uint64_t> k_unrefine_families(const MapCtx& m, const int32_t* hood, int nh, const DevMesh& M,
                                          const std::vector<uint64_t>& req, const std::vector<uint64_t>& S,
                                          const std::vector<uint64_t>& DU, hipStream_t s, const uint64_t* dS_given,
                                          const uint64_t* dreq_heads) {
	// dreq_heads: req on the device, ascending octant-0 children of level > 0,
	// so their parents come out ascending and distinct (no sort, no marker)
	if (req.empty()) return {};
	DBuf<uint64_t> dr_own, par, dS_own, dDU;
	const uint64_t* drp = given_or_upload(dreq_heads, req, dr_own, s);
	const uint64_t* dS = given_or_upload(dS_given, S, dS_own, s);
	upload(dDU, DU, s);
	par.alloc(req.size() + 1);
	launch_per_item(request_parents_kernel, req.size(), s, m, drp, req.size(), par.p);
	size_t n = dreq_heads ? req.size() : sort_unique_u64(par.p, req.size(), s);
	if (!dreq_heads) {
		// the level-0 requests' marker sorts last
		uint64_t last = 0;
		if (n) d2h_small(&last, par.p + n - 1, 8, s);
		if (n && last == ~uint64_t(0)) n--;
	}
	if (!n) return {};
	DBuf<uint32_t> ok;
	ok.alloc(n);
	k_fill_i32(reinterpret_cast<int32_t*>(ok.p), n, 1, s);
	family_blocked_kernel<<<grid_for(n, 256), 256, 0, s>>>(m, par.p, n, dS, S.size(), dDU.p, DU.size(), ok.p);
	if (nh > 0)
		unrefine_check_kernel<<<grid_for(n * size_t(nh), 256), 256, 0, s>>>(m, hood, nh, M, par.p, n, dS, S.size(), ok.p);
	HIP_CHECK(hipGetLastError());
	// candidates and verdicts in one read
	DBuf<uint8_t> stage;
	stage.alloc(12 * n);
	HIP_CHECK(hipMemcpyAsync(stage.p, par.p, 8 * n, hipMemcpyDeviceToDevice, s));
	HIP_CHECK(hipMemcpyAsync(stage.p + 8 * n, ok.p, 4 * n, hipMemcpyDeviceToDevice, s));
	const std::vector<uint8_t> hb = download(stage.p, 12 * n, s);
	std::vector<uint64_t> out;
	for (size_t i = 0; i < n; i++) {
		uint32_t v;
		std::memcpy(&v, hb.data() + 8 * n + 4 * i, 4);
		if (v) {
			uint64_t c;
			std::memcpy(&c, hb.data() + 8 * i, 8);
			out.push_back(c);
		}
	}
	return out;
}

namespace {
// execute_refines (10104-10554): children replace refined leaves and inherit
// the owner (10228-10237); the children of an unrefined parent are replaced
// by the parent, owned by the owner of its first child (10298)
__global__ void refine_count_kernel(MapCtx m, const uint64_t* kid, size_t n, const uint64_t* S, size_t nS,
                                    const uint64_t* F, size_t nF, uint32_t* cnt) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint64_t c = kid[i];
		uint32_t k = 1u;
		if (sorted_has(S, nS, c)) {
			k = 8u;
		} else if (nF) {
			const uint64_t p = map_parent(m, c);
			if (p != c && sorted_has(F, nF, p)) k = map_child(m, p) == c ? 1u : 0u;
		}
		cnt[i] = k;
	}
}

__global__ void refine_fill_kernel(MapCtx m, const uint64_t* kid, const int32_t* kown, size_t n, const uint32_t* pos,
                                   const uint32_t* cnt, const uint64_t* F, size_t nF, uint64_t* oid, int32_t* oown) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const size_t p = pos[i];
		if (cnt[i] == 0u) continue;
		if (cnt[i] == 1u) {
			uint64_t c = kid[i];
			if (nF) {
				const uint64_t par = map_parent(m, c);
				if (par != c && sorted_has(F, nF, par)) c = par;
			}
			oid[p] = c;
			oown[p] = kown[i];
		} else {
			uint64_t ch[8];
			map_all_children(m, kid[i], ch);
			for (int k = 0; k < 8; k++) {
				oid[p + k] = ch[k];
				oown[p + k] = kown[i];
			}
		}
	}
}

// The own-leaf prefix of the known list (Mesh::n_prefix: kid index = slot)
// classified by lookups of the refined cells and the merged families'
// children instead of a search per entry: cls 1 refined, 2 a family's first
// child (becomes the parent), 3 another child (drops out), 0 unchanged.
__global__ void mark_refined_kernel(DevMesh M, const uint64_t* S, size_t nS, size_t n_prefix, uint8_t* cls) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < nS; i += size_t(gridDim.x) * blockDim.x) {
		const int32_t sl = dm_slot(M, S[i]);
		if (sl >= 0 && size_t(sl) < n_prefix) cls[sl] = 1;
	}
}

__global__ void mark_families_kernel(MapCtx m, DevMesh M, const uint64_t* F, size_t nF, size_t n_prefix, uint8_t* cls) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < 8 * nF; i += size_t(gridDim.x) * blockDim.x) {
		uint64_t ch[8];
		map_all_children(m, F[i >> 3], ch);
		const int k = int(i & 7);
		const int32_t sl = dm_slot(M, ch[k]);
		if (sl >= 0 && size_t(sl) < n_prefix) cls[sl] = k == 0 ? 2 : 3;
	}
}

__global__ void prefix_count_kernel(const uint8_t* cls, size_t n, uint32_t* cnt) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint8_t c = cls[i];
		cnt[i] = c == 1 ? 8u : (c == 3 ? 0u : 1u);
	}
}

// src (optional): per output entry the input index its payload comes from
// (-1: a merged parent, which starts zeroed)
__global__ void prefix_fill_kernel(MapCtx m, const uint64_t* kid, const int32_t* kown, const uint8_t* cls, size_t n,
                                   const uint32_t* pos, uint64_t* oid, int32_t* oown, int32_t* src) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const uint8_t c = cls[i];
		const size_t p = pos[i];
		if (c == 3) continue;
		if (c == 1) {
			uint64_t ch[8];
			map_all_children(m, kid[i], ch);
			for (int k = 0; k < 8; k++) {
				oid[p + k] = ch[k];
				oown[p + k] = kown[i];
				if (src) src[p + k] = int32_t(i);
			}
		} else {
			oid[p] = c == 2 ? map_parent(m, kid[i]) : kid[i];
			oown[p] = kown[i];
			if (src) src[p] = c == 2 ? -1 : int32_t(i);
		}
	}
}
}  // namespace

void k_apply_refines(const MapCtx& m, const uint64_t* kid, const int32_t* kown, size_t n, const std::vector<uint64_t>& S,
                     const std::vector<uint64_t>& F, DBuf<uint64_t>& out_id, DBuf<int32_t>& out_own, size_t& n_out,
                     hipStream_t s, const size_t* at, size_t* pos_at, int n_at, size_t n_prefix, const DevMesh* dm,
                     DBuf<int32_t>* src, const uint64_t* dS_given, const uint64_t* dF_given) {
	DBuf<uint64_t> dS_own, dF_own;
	const uint64_t* dS = given_or_upload(dS_given, S, dS_own, s);
	const uint64_t* dF = given_or_upload(dF_given, F, dF_own, s);
	DBuf<uint32_t> cnt, pos;
	cnt.alloc(n + 1);
	pos.alloc(n + 1);
	HIP_CHECK(hipMemsetAsync(cnt.p, 0, (n + 1) * 4, s));
	// [0, np): the own-leaf prefix classified by lookups; the rest searched
	const size_t np = dm ? std::min(n_prefix, n) : 0;
	DBuf<uint8_t> cls;
	if (np) {
		cls.alloc(np);
		HIP_CHECK(hipMemsetAsync(cls.p, 0, np, s));
		if (!S.empty()) mark_refined_kernel<<<grid_for(S.size(), 256), 256, 0, s>>>(*dm, dS, S.size(), np, cls.p);
		if (!F.empty())
			mark_families_kernel<<<grid_for(8 * F.size(), 256), 256, 0, s>>>(m, *dm, dF, F.size(), np, cls.p);
		launch_per_item(prefix_count_kernel, np, s, cls.p, np, cnt.p);
	}
	if (n > np) {
		launch_per_item(refine_count_kernel, n - np, s, m, kid + np, n - np, dS, S.size(), dF, F.size(), cnt.p + np);
	}
	// the total and where input positions at[k] land (the expanded list's run
	// boundaries), one read
	DX_REQUIRE(n_at >= 0 && n_at <= 3, "internal error: too many run boundaries");
	uint32_t landed[3] = {0, 0, 0};
	n_out = scan_exclusive_u32_at(cnt.p, pos.p, n, s, at, n_at, landed);
	for (int k = 0; k < n_at; k++) pos_at[k] = landed[k];
	out_id.alloc(n_out + 1);
	out_own.alloc(n_out + 1);
	if (src) {
		src->alloc(n_out + 1);
		// prefix_fill_kernel writes every output of the prefix; only the rest
		// (refine_fill_kernel writes no sources) starts at -1
		if (np < n) HIP_CHECK(hipMemsetAsync(src->p, 0xff, (n_out + 1) * 4, s));
		else HIP_CHECK(hipMemsetAsync(src->p + n_out, 0xff, 4, s));
	}
	if (np) {
		launch_per_item(prefix_fill_kernel, np, s, m, kid, kown, cls.p, np, pos.p, out_id.p, out_own.p,
		                src ? src->p : nullptr);
	}
	if (n > np) {
		launch_per_item(refine_fill_kernel, n - np, s, m, kid + np, kown + np, n - np, pos.p + np, cnt.p + np, dF,
		                F.size(), out_id.p, out_own.p);
	}
	// stream-ordered for rebuild (its readers run on s); the temporaries go
	// back to the pool, which holds them until a device sync
}

namespace {
// the children of the refined cells owned by `rank` (stop_refining's
// created cells); one thread per refined cell, full waves (wave_reserve)
__global__ void created_children_kernel(MapCtx m, DevMesh M, int rank, const uint64_t* S, size_t nS, uint64_t* out,
                                        unsigned long long* ctr) {
	const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
	const bool mine = i < nS && dm_owner(M, S[i]) == rank;
	const unsigned long long at = wave_reserve(ctr, mine ? 8u : 0u);
	if (!mine) return;
	uint64_t ch[8];
	map_all_children(m, S[i], ch);
	for (int k = 0; k < 8; k++) out[at + k] = ch[k];
}
}  // namespace

size_t k_created_children(const MapCtx& m, const DevMesh& M, int rank, const std::vector<uint64_t>& S,
                          DBuf<uint64_t>& out, hipStream_t s, const uint64_t* dS_given, bool sorted) {
	if (S.empty()) return 0;
	DBuf<uint64_t> dS_own;
	const uint64_t* dS = given_or_upload(dS_given, S, dS_own, s);
	out.alloc(8 * S.size() + 1);
	DevCounter ctr;
	created_children_kernel<<<unsigned((S.size() + 255) / 256), 256, 0, s>>>(m, M, rank, dS, S.size(), out.p,
	                                                                         ctr.zero(s));
	HIP_CHECK(hipGetLastError());
	const size_t n = ctr.read(s);
	if (sorted) sort_u64(out.p, n, s, map_id_bits(m));
	return n;
}

namespace {
// the children of merged families that stay on `rank` (owned here, as is the
// family's first child, which becomes the parent's owner), with their slots
__global__ void kept_children_kernel(MapCtx m, DevMesh M, int rank, const uint64_t* F, size_t nF, uint64_t* out,
                                     int32_t* out_slot, unsigned long long* ctr) {
	const size_t t = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
	bool keep = false;
	uint64_t c = 0;
	int32_t sl = -1;
	if (t < 8 * nF) {
		uint64_t ch[8];
		map_all_children(m, F[t >> 3], ch);
		c = ch[t & 7];
		keep = dm_owner(M, c) == rank && dm_owner(M, ch[0]) == rank;
		if (keep) sl = dm_slot(M, c);
	}
	const unsigned long long at = wave_reserve(ctr, keep ? 1u : 0u);
	if (!keep) return;
	out[at] = c;
	out_slot[at] = sl;
}

// Every child of every merged family local (one process): the children in
// ascending id without a sort.  F ascending, so its families come in level
// groups, and within a group the children of one octant k ascend with their
// parents (the id's (z, y, x) digits are the parent's doubled plus the
// octant's bits), so a child's position is the number of smaller children of
// each octant in its group, found by binary search of that octant's stream.
struct LevelGroups {
	uint32_t lo[kRangeLevels + 1];  // group g: families [lo[g], lo[g + 1])
	int n;
};
__global__ void family_children_kernel(MapCtx m, const uint64_t* __restrict__ F, size_t nF, uint64_t* __restrict__ ch) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < nF; i += size_t(gridDim.x) * blockDim.x) {
		uint64_t c[8];
		map_all_children(m, F[i], c);
#pragma unroll
		for (int k = 0; k < 8; k++) ch[8 * i + k] = c[k];
	}
}
__global__ void kept_ordered_kernel(DevMesh M, const uint64_t* __restrict__ ch, size_t nF, LevelGroups G,
                                    uint64_t* __restrict__ out, int32_t* __restrict__ out_slot) {
	for (size_t t = blockIdx.x * size_t(blockDim.x) + threadIdx.x; t < 8 * nF; t += size_t(gridDim.x) * blockDim.x) {
		const uint32_t i = uint32_t(t >> 3);
		const int k = int(t & 7);
		uint32_t g0 = 0, g1 = uint32_t(nF);
		for (int g = 0; g < G.n; g++)
			if (i >= G.lo[g] && i < G.lo[g + 1]) {
				g0 = G.lo[g];
				g1 = G.lo[g + 1];
			}
		const uint64_t c = ch[t];
		size_t pos = 8 * size_t(g0) + (i - g0);  // its own octant's smaller ones
		for (int q = 0; q < 8; q++) {
			if (q == k) continue;
			uint32_t lo = g0, hi = g1;
			while (lo < hi) {
				const uint32_t mid = (lo + hi) >> 1;
				if (ch[8 * size_t(mid) + q] < c) lo = mid + 1;
				else hi = mid;
			}
			pos += lo - g0;
		}
		out[pos] = c;
		out_slot[pos] = dm_slot(M, c);
	}
}
}  // namespace

size_t k_kept_children(const MapCtx& m, const DevMesh& M, int rank, const std::vector<uint64_t>& F,
                       DBuf<uint64_t>& ids, DBuf<int32_t>& slots, hipStream_t s, const uint64_t* dF_given,
                       bool all_local) {
	ids.release();
	slots.release();
	if (F.empty()) return 0;
	DBuf<uint64_t> dF_own, k1, k2;
	DBuf<int32_t> v1;
	const uint64_t* dF = given_or_upload(dF_given, F, dF_own, s);
	const size_t cap = 8 * F.size();
	if (all_local && F.size() < (size_t(1) << 31)) {
		LevelGroups G{};
		G.n = 0;
		int last = -1;
		for (size_t i = 0; i < F.size(); i++) {
			const int L = map_level(m, F[i]);
			if (L != last) {
				DX_REQUIRE(G.n < kRangeLevels && L > last, "internal error: merged families not ascending");
				G.lo[G.n++] = uint32_t(i);
				last = L;
			}
		}
		G.lo[G.n] = uint32_t(F.size());
		ids.alloc(cap + 1);
		slots.alloc(cap + 1);
		k1.alloc(cap + 1);
		family_children_kernel<<<grid_for(F.size(), 256), 256, 0, s>>>(m, dF, F.size(), k1.p);
		launch_per_item(kept_ordered_kernel, cap, s, M, k1.p, F.size(), G, ids.p, slots.p);
		return cap;
	}
	k1.alloc(cap + 1);
	k2.alloc(cap + 1);
	v1.alloc(cap + 1);
	slots.alloc(cap + 1);
	DevCounter ctr;
	kept_children_kernel<<<unsigned((cap + 255) / 256), 256, 0, s>>>(m, M, rank, dF, F.size(), k1.p, v1.p, ctr.zero(s));
	HIP_CHECK(hipGetLastError());
	const size_t n = ctr.read(s);
	if (n) {
		with_temp(cub_sort_pairs(k1.p, k2.p, v1.p, slots.p, n, map_id_bits(m), s));
		ids.swap(k2);
	}
	return n;
}

}  // namespace dccrgx
