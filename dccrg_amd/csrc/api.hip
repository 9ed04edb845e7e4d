// dccrgx C ABI (include/dccrgx.h): every entry point wraps the host driver
// in an exception guard and returns a status code.  Wrappers only: the
// drivers are functions of Grid& in the other sources (dccrgx_grid.hpp).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <limits>

#include "dccrgx_grid.hpp"
#include "dccrgx_reduce.hpp"

namespace dccrgx {

static thread_local std::string g_last_error;

template <class F>
static int guard(F&& f) {
	try {
		return f();
	} catch (const Error& e) {
		g_last_error = e.what();
		return e.code;
	} catch (const std::exception& e) {
		g_last_error = e.what();
		return DCCRGX_EINVAL;
	}
}

static int copy_out_u64(const std::vector<uint64_t>& v, uint64_t* out, size_t cap, size_t* n) {
	if (n) *n = v.size();
	if (v.size() > cap || (!out && !v.empty())) return DCCRGX_ERANGE;
	if (!v.empty()) std::memcpy(out, v.data(), v.size() * 8);
	return DCCRGX_OK;
}

}  // namespace dccrgx

// ============================================================================
// C ABI
// ============================================================================
using namespace dccrgx;

struct dccrgx_grid {
	Grid g;
};

#define GRID_OR_FAIL(gp) \
	if (!(gp)) throw Error(DCCRGX_EINVAL, "null grid"); \
	Grid& g = (gp)->g

static dccrgx_grid* new_grid(int rank, int size, int device) {
	DX_REQUIRE(size >= 1 && rank >= 0 && rank < size, "invalid rank/size");
	HIP_CHECK(hipSetDevice(device));
	auto* h = new dccrgx_grid();
	Grid& g = h->g;
	g.rank = rank;
	g.size = size;
	g.device = device;
	HIP_CHECK(hipStreamCreateWithFlags(&g.s_comp, hipStreamNonBlocking));
	HIP_CHECK(hipStreamCreateWithFlags(&g.s_comm, hipStreamNonBlocking));
	HIP_CHECK(hipEventCreateWithFlags(&g.ev_comp, hipEventDisableTiming));
	HIP_CHECK(hipEventCreateWithFlags(&g.ev_halo, hipEventDisableTiming));
	mesh_init_implicit(g);
	return h;
}

extern "C" {

#if DCCRGX_PHASE_TIMING
// analysis build only: forget the phase totals so far (e.g. after a warm-up)
void dccrgx_phase_reset(void) { phase_reset(); }
#endif

const char* dccrgx_last_error(void) { return g_last_error.c_str(); }
int dccrgx_abi_version(void) { return DCCRGX_ABI_VERSION; }

int dccrgx_get_unique_id(void* out) {
	return guard([&] {
		ncclUniqueId id;
		NCCL_CHECK(ncclGetUniqueId(&id));
		std::memcpy(out, &id, sizeof(id));
		return 0;
	});
}

int dccrgx_create(int rank, int size, int device, const void* nccl_id, dccrgx_grid** out) {
	return guard([&] {
		DX_REQUIRE(out, "null output");
		dccrgx_grid* h = new_grid(rank, size, device);
		if (nccl_id) {  // without an id: a detached view of one rank (no transport)
			ncclUniqueId id;
			std::memcpy(&id, nccl_id, sizeof(id));
			const ncclResult_t r = ncclCommInitRank(&h->g.nccl, size, id, rank);
			if (r != ncclSuccess) {
				delete h;
				throw Error(DCCRGX_ECOMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
			}
		}
		*out = h;
		return 0;
	});
}

int dccrgx_create_with_exchange(int rank, int size, int device, dccrgx_exchange_fn fn, void* ctx, dccrgx_grid** out) {
	return guard([&] {
		DX_REQUIRE(out && fn, "null output or exchange function");
		dccrgx_grid* h = new_grid(rank, size, device);
		h->g.xfn = fn;
		h->g.xctx = ctx;
		*out = h;
		return 0;
	});
}

int dccrgx_device_count(int* n) {
	return guard([&] {
		DX_REQUIRE(n, "null output");
		HIP_CHECK(hipGetDeviceCount(n));
		return 0;
	});
}

int dccrgx_get_cells_by_criteria(dccrgx_grid* gp, const int32_t* criteria, size_t nc, int exact_match, int hood,
                                 uint64_t* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		DX_REQUIRE(criteria || !nc, "null criteria");
		if (hood != DCCRGX_DEFAULT_HOOD && !g.uhoods.count(hood)) return copy_out_u64({}, out, cap, n);
		return copy_out_u64(cells_by_criteria(g, criteria, nc, exact_match != 0, hood), out, cap, n);
	});
}

int dccrgx_get_slots(dccrgx_grid* gp, const uint64_t* ids, size_t n, int64_t* slots) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE((ids && slots) || !n, "null argument");
		for (size_t i = 0; i < n; i++) slots[i] = lookup_slot(g, ids[i]);
		return 0;
	});
}

int dccrgx_download_user_csr(dccrgx_grid* gp, int hood, int kind, uint32_t* ptr, uint64_t* ids, int32_t* offs,
                             size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		if (!g.uhoods.count(hood)) return DCCRGX_ENOTFOUND;
		DX_REQUIRE(kind == 0 || kind == 1, "invalid CSR kind");
		UserHood& h = ensure_uhood(g, hood);
		const size_t nl = g.n_local;
		const std::vector<uint32_t> hp = download(kind == 0 ? h.nof_ptr.p : h.nto_ptr.p, nl + 1, g.s_comp);
		const size_t tot = hp[nl];
		if (n) *n = tot;
		if (tot > cap) return DCCRGX_ERANGE;
		std::memcpy(ptr, hp.data(), (nl + 1) * 4);
		if (!tot) return 0;
		d2h_small(ids, kind == 0 ? h.nof_id.p : h.nto_id.p, tot * 8, g.s_comp);
		if (offs && kind == 0) d2h_small(offs, h.nof_off.p, tot * 12, g.s_comp);
		return 0;
	});
}

int dccrgx_destroy(dccrgx_grid* gp) {
	return guard([&] {
		if (!gp) return 0;
		Grid& g = gp->g;
		(void)hipDeviceSynchronize();
		drain_timing(g);
		if (g.nccl) ncclCommDestroy(g.nccl);
		if (g.pin_stage) (void)hipHostFree(g.pin_stage);
		if (g.ev_comp) (void)hipEventDestroy(g.ev_comp);
		if (g.ev_halo) (void)hipEventDestroy(g.ev_halo);
		if (g.s_comp) (void)hipStreamDestroy(g.s_comp);
		if (g.s_comm) (void)hipStreamDestroy(g.s_comm);
		delete gp;
		return 0;
	});
}

int dccrgx_set_initial_length(dccrgx_grid* gp, const uint64_t length[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(!g.initialized, "set_initial_length after initialize");
		for (int d = 0; d < 3; d++) DX_REQUIRE(length[d] > 0, "grid length must be > 0");
		for (int d = 0; d < 3; d++) g.len[d] = length[d];
		return 0;
	});
}

int dccrgx_get_initial_length(dccrgx_grid* gp, uint64_t length[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		for (int d = 0; d < 3; d++) length[d] = g.len[d];
		return 0;
	});
}

int dccrgx_get_periodic(dccrgx_grid* gp, int periodic[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		for (int d = 0; d < 3; d++) periodic[d] = g.per[d] ? 1 : 0;
		return 0;
	});
}

int dccrgx_set_maximum_refinement_level(dccrgx_grid* gp, int level) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(!g.initialized, "set_maximum_refinement_level after initialize");
		const int maxpos = max_possible_level(g.len);
		if (level < 0) level = maxpos;
		DX_REQUIRE(level <= maxpos && level < kMaxLevels, "refinement level too large for the grid");
		g.R = level;
		return 0;
	});
}

int dccrgx_get_maximum_refinement_level(dccrgx_grid* gp, int* level) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		*level = g.R;
		return 0;
	});
}

int dccrgx_get_neighborhood_length(dccrgx_grid* gp, unsigned* length) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(length != nullptr, "null output");
		*length = g.hood_len;
		return 0;
	});
}

int dccrgx_set_periodic(dccrgx_grid* gp, int x, int y, int z) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(!g.initialized, "set_periodic after initialize");
		g.per[0] = x != 0;
		g.per[1] = y != 0;
		g.per[2] = z != 0;
		return 0;
	});
}

int dccrgx_set_neighborhood_length(dccrgx_grid* gp, unsigned length) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(!g.initialized, "set_neighborhood_length after initialize");
		DX_REQUIRE(length <= max_hood_length(),
		           "neighborhood length > " + std::to_string(max_hood_length()) + " not supported");
		g.hood_len = length;
		return 0;
	});
}

int dccrgx_initialize(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		init_impl(g);
		return 0;
	});
}

int dccrgx_set_geometry(dccrgx_grid* gp, const double start[3], const double l0[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		for (int d = 0; d < 3; d++) DX_REQUIRE(l0[d] > 0, "cell length must be > 0");
		for (int d = 0; d < 3; d++) {
			g.start[d] = start[d];
			g.l0[d] = l0[d];
		}
		// back to Cartesian: the coordinates and the block made from them go
		// (a block given through dccrgx_set_geometry_block stays)
		if (g.str.active) {
			g.str.drop();
			g.geo_block.clear();
		}
		return 0;
	});
}

int dccrgx_set_stretched_geometry(dccrgx_grid* gp, const double* const coords[3], const size_t n[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(coords && n, "null pointer");
		set_stretched_geometry(g, coords, n);
		return 0;
	});
}

int dccrgx_get_stretched_geometry(dccrgx_grid* gp, int dim, double* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(n != nullptr, "null count");
		DX_REQUIRE(dim >= 0 && dim < 3, "dimension must be 0, 1 or 2");
		const std::vector<double>& c = g.str.c[dim];
		*n = g.str.active ? c.size() : 0;
		if (!out || !*n) return 0;
		DX_REQUIRE(cap >= c.size(), "buffer too small for the coordinates");
		std::memcpy(out, c.data(), c.size() * 8);
		return 0;
	});
}

int dccrgx_geometry_fill(dccrgx_grid* gp, const int center_fields[3], const int length_fields[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		geometry_fill(g, center_fields, length_fields);
		return 0;
	});
}

int dccrgx_get_geometry(dccrgx_grid* gp, double start[3], double l0[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		for (int d = 0; d < 3; d++) {
			if (start) start[d] = g.start[d];
			if (l0) l0[d] = g.l0[d];
		}
		return 0;
	});
}

int dccrgx_set_geometry_block(dccrgx_grid* gp, const void* bytes, size_t n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		set_geometry_block(g, bytes, n);
		return 0;
	});
}

int dccrgx_get_geometry_block(dccrgx_grid* gp, void* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(n != nullptr, "null count");
		*n = g.geo_block.size();
		if (!out) return 0;
		DX_REQUIRE(cap >= g.geo_block.size(), "buffer too small for the geometry block");
		if (!g.geo_block.empty()) std::memcpy(out, g.geo_block.data(), g.geo_block.size());
		return 0;
	});
}

int dccrgx_geometry_batch(dccrgx_grid* gp, const uint64_t* ids, size_t n, double* center, double* length) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(ids || !n, "null ids");
		geometry_batch(g, ids, n, center, length);
		return 0;
	});
}

uint64_t dccrgx_get_cell_from_indices(dccrgx_grid* gp, const uint64_t ind[3], int level) {
	if (!gp) return error_cell;
	MapCtx m;
	map_init(m, gp->g.len, gp->g.R, gp->g.per);
	return map_from_indices(m, ind[0], ind[1], ind[2], level);
}

int dccrgx_mapping_batch(dccrgx_grid* gp, const uint64_t* ids, size_t n, int32_t* level, uint64_t* out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE((ids && level && out) || !n, "null argument");
		mapping_batch(g, ids, n, level, out);
		return 0;
	});
}

int dccrgx_get_indices(dccrgx_grid* gp, uint64_t cell, uint64_t ind[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		MapCtx m;
		map_init(m, g.len, g.R, g.per);
		const int l = map_indices(m, cell, ind[0], ind[1], ind[2]);
		return l < 0 ? DCCRGX_ENOTFOUND : 0;
	});
}

int dccrgx_get_refinement_level(dccrgx_grid* gp, uint64_t cell) {
	if (!gp) return -1;
	MapCtx m;
	map_init(m, gp->g.len, gp->g.R, gp->g.per);
	return map_level(m, cell);
}

uint64_t dccrgx_get_last_cell(dccrgx_grid* gp) {
	if (!gp) return 0;
	MapCtx m;
	map_init(m, gp->g.len, gp->g.R, gp->g.per);
	return m.last;
}

int dccrgx_get_counts(dccrgx_grid* gp, size_t* ni, size_t* no, size_t* nr, size_t* ns) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		if (ni) *ni = g.n_inner;
		if (no) *no = g.n_outer;
		if (nr) *nr = g.n_recv;
		if (ns) *ns = g.n_slots;
		return 0;
	});
}

int dccrgx_get_cells(dccrgx_grid* gp, int which, uint64_t* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		const auto& ids = slot_ids_host(g);
		std::vector<uint64_t> v;
		switch (which) {
		case DCCRGX_CELLS_LOCAL: v.assign(ids.begin(), ids.begin() + ptrdiff_t(g.n_local)); break;
		case DCCRGX_CELLS_INNER: v.assign(ids.begin(), ids.begin() + ptrdiff_t(g.n_inner)); break;
		case DCCRGX_CELLS_OUTER: v.assign(ids.begin() + ptrdiff_t(g.n_inner), ids.begin() + ptrdiff_t(g.n_local)); break;
		case DCCRGX_CELLS_REMOTE: v.assign(ids.begin() + ptrdiff_t(g.n_local), ids.end()); break;
		case DCCRGX_CELLS_ALL: v = ids; break;
		default: throw Error(DCCRGX_EINVAL, "invalid selection");
		}
		std::sort(v.begin(), v.end());
		return copy_out_u64(v, out, cap, n);
	});
}

int dccrgx_get_slot_ids(dccrgx_grid* gp, uint64_t* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		return copy_out_u64(slot_ids_host(g), out, cap, n);
	});
}

int dccrgx_get_neighbors_of(dccrgx_grid* gp, uint64_t cell, uint64_t* ids, int32_t* offs, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		const int64_t s = lookup_slot(g, cell);
		if (s < 0 || size_t(s) >= g.n_local) return DCCRGX_ENOTFOUND;
		ensure_csr(g);
		uint32_t be[2];
		d2h_small(be, g.nof_ptr.p + s, 8, g.s_comp);
		const size_t k = be[1] - be[0];
		if (n) *n = k;
		if (k > cap) return DCCRGX_ERANGE;
		if (k) {
			d2h_small(ids, g.nof_id.p + be[0], k * 8, g.s_comp);
			if (offs) d2h_small(offs, g.nof_off.p + 3 * size_t(be[0]), k * 12, g.s_comp);
		}
		return 0;
	});
}

int dccrgx_get_neighbors_to(dccrgx_grid* gp, uint64_t cell, uint64_t* ids, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		const int64_t s = lookup_slot(g, cell);
		if (s < 0 || size_t(s) >= g.n_local) return DCCRGX_ENOTFOUND;
		ensure_csr(g);
		uint32_t be[2];
		d2h_small(be, g.nto_ptr.p + s, 8, g.s_comp);
		const size_t k = be[1] - be[0];
		if (n) *n = k;
		if (k > cap) return DCCRGX_ERANGE;
		if (k) d2h_small(ids, g.nto_id.p + be[0], k * 8, g.s_comp);
		return 0;
	});
}

int dccrgx_get_face_neighbors_of(dccrgx_grid* gp, uint64_t cell, uint64_t* ids, int32_t* dirs, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		static const int dmap[6] = {-1, +1, -2, +2, -3, +3};
		const int64_t s = lookup_slot(g, cell);
		if (s < 0 || size_t(s) >= g.n_local) {
			// a remote cell this process knows (e.g. a copy in all_cells()): its
			// faces from the known leaves, probed at every level at each face's
			// probe point (the leaf there must be known, else the face lies
			// beyond the ghost region and the cell is not answered)
			if (lookup_owner(g, cell) < 0) return DCCRGX_ENOTFOUND;
			const MapCtx& m = g.m;
			uint64_t c[3], p[3];
			const int lvl = map_indices(m, cell, c[0], c[1], c[2]);
			std::vector<uint64_t> cand;
			for (int dir = 0; dir < 6; dir++)
				if (face_probe(m, c, lvl, dir, p))
					for (int l = 0; l <= m.R; l++) cand.push_back(map_from_indices(m, p[0], p[1], p[2], l));
			std::sort(cand.begin(), cand.end());
			cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
			std::vector<int32_t> own(cand.size());
			lookup_batch(g, cand.data(), cand.size(), own.data(), nullptr);
			const auto exists = [&](uint64_t id) {
				const auto it = std::lower_bound(cand.begin(), cand.end(), id);
				return it != cand.end() && *it == id && own[size_t(it - cand.begin())] >= 0;
			};
			std::vector<std::pair<uint64_t, int>> out;
			for (int dir = 0; dir < 6; dir++) {
				if (!face_probe(m, c, lvl, dir, p)) continue;
				bool any = false;
				for (int l = 0; l <= m.R && !any; l++) any = exists(map_from_indices(m, p[0], p[1], p[2], l));
				if (!any) throw Error(DCCRGX_ENOTFOUND, "a face of this remote cell lies beyond the ghost region");
				uint64_t f[4];
				const int k = face_dir(m, c, lvl, dir, exists, f);
				for (int i = 0; i < k; i++) out.push_back({f[i], dmap[dir]});
			}
			if (n) *n = out.size();
			if (out.size() > cap) return DCCRGX_ERANGE;
			for (size_t i = 0; i < out.size(); i++) {
				ids[i] = out[i].first;
				if (dirs) dirs[i] = out[i].second;
			}
			return 0;
		}
		ensure_face_csr(g);
		uint32_t be[2];
		d2h_small(be, g.face_ptr.p + s, 8, g.s_comp);
		const size_t k = be[1] - be[0];
		if (n) *n = k;
		if (k > cap) return DCCRGX_ERANGE;
		std::vector<int32_t> ent(k);
		if (k) d2h_small(ent.data(), g.face_ent.p + be[0], k * 4, g.s_comp);
		const auto& sid = slot_ids_host(g);
		for (size_t i = 0; i < k; i++) {
			ids[i] = sid[size_t(ent[i] >> 3)];
			if (dirs) dirs[i] = dmap[ent[i] & 7];
		}
		return 0;
	});
}

int dccrgx_download_csr(dccrgx_grid* gp, int kind, uint32_t* ptr, uint64_t* ids, int32_t* aux, size_t cap,
                        size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(kind >= 0 && kind <= 3, "invalid CSR kind");
		const size_t nl = g.n_local;
		const uint32_t* dptr = nullptr;
		if (kind == 2) {
			ensure_face_csr(g);
			dptr = g.face_ptr.p;
		} else {
			ensure_csr(g);
			dptr = kind == 0 ? g.nof_ptr.p : kind == 1 ? g.nto_ptr.p : g.it_ptr.p;
		}
		std::vector<uint32_t> hp = download(dptr, nl + 1, g.s_comp);
		const size_t tot = hp[nl];
		if (n) *n = tot;
		if (tot > cap) return DCCRGX_ERANGE;
		std::memcpy(ptr, hp.data(), (nl + 1) * 4);
		if (!tot) return 0;
		const auto& sid = slot_ids_host(g);
		if (kind == 0) {
			d2h_small(ids, g.nof_id.p, tot * 8, g.s_comp);
			if (aux) d2h_small(aux, g.nof_off.p, tot * 12, g.s_comp);
		} else if (kind == 1) {
			d2h_small(ids, g.nto_id.p, tot * 8, g.s_comp);
		} else if (kind == 2) {
			std::vector<int32_t> ent = download(g.face_ent.p, tot, g.s_comp);
			static const int dmap[6] = {-1, +1, -2, +2, -3, +3};
			for (size_t i = 0; i < tot; i++) {
				ids[i] = sid[size_t(ent[i] >> 3)];
				if (aux) aux[i] = dmap[ent[i] & 7];
			}
		} else {
			std::vector<int32_t> sl = download(g.it_slot.p, tot, g.s_comp);
			for (size_t i = 0; i < tot; i++) ids[i] = sid[size_t(sl[i])];
			if (aux) d2h_small(aux, g.it_off.p, tot * 12, g.s_comp);
		}
		return 0;
	});
}

int dccrgx_is_local(dccrgx_grid* gp, uint64_t cell) {
	if (!gp) return 0;
	try {
		return is_local_cell(gp->g, cell) ? 1 : 0;
	} catch (const std::exception& e) {
		g_last_error = e.what();
		return 0;
	}
}

int dccrgx_get_process(dccrgx_grid* gp, uint64_t cell) {
	if (!gp) return -1;
	try {
		return lookup_owner(gp->g, cell);
	} catch (const std::exception& e) {
		g_last_error = e.what();
		return -1;
	}
}

int64_t dccrgx_get_slot(dccrgx_grid* gp, uint64_t cell) {
	if (!gp) return -1;
	try {
		return lookup_slot(gp->g, cell);
	} catch (const std::exception& e) {
		g_last_error = e.what();
		return -1;
	}
}

int dccrgx_get_peers(dccrgx_grid* gp, int32_t* peers, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		if (n) *n = g.peers.size();
		if (g.peers.size() > cap) return DCCRGX_ERANGE;
		for (size_t i = 0; i < g.peers.size(); i++) peers[i] = g.peers[i];
		return 0;
	});
}

int dccrgx_get_cells_to_send(dccrgx_grid* gp, int peer, uint64_t* ids, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		auto it = g.halo.send_ids.find(peer);
		static const std::vector<uint64_t> empty;
		return copy_out_u64(it == g.halo.send_ids.end() ? empty : it->second, ids, cap, n);
	});
}

int dccrgx_get_cells_to_receive(dccrgx_grid* gp, int peer, uint64_t* ids, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		auto it = g.halo.recv_ids.find(peer);
		static const std::vector<uint64_t> empty;
		return copy_out_u64(it == g.halo.recv_ids.end() ? empty : it->second, ids, cap, n);
	});
}

int dccrgx_get_cell_process(dccrgx_grid* gp, uint64_t* ids, int32_t* owners, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		std::vector<uint64_t> k;
		std::vector<int32_t> o;
		known_leaves(g, k, o);
		if (n) *n = k.size();
		if (!ids) return 0;
		if (cap < k.size()) return int(DCCRGX_ERANGE);
		std::copy(k.begin(), k.end(), ids);
		if (owners) std::copy(o.begin(), o.end(), owners);
		return 0;
	});
}

static int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

int dccrgx_find_neighbors_of(dccrgx_grid* gp, uint64_t cell, const int32_t* items, size_t n_items, uint64_t* ids,
                             int32_t* offs, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		DX_REQUIRE(items || !n_items, "null neighborhood");
		const MapCtx& m = g.m;
		if (lookup_owner(g, cell) < 0) return DCCRGX_ENOTFOUND;  // 4354-4362: unknown cell
		uint64_t c[3];
		const int lvl = map_indices(m, cell, c[0], c[1], c[2]);
		const bool local = is_local_cell(g, cell);
		const int64_t len = int64_t(1) << (m.R - lvl), l0 = int64_t(1) << m.R;
		const int64_t r = std::max(1, int(g.hood_len));
		// the three cells an item's box can resolve to (nof_item): finer,
		// same size and coarser, all probed in one device lookup
		std::vector<uint64_t> cand;
		for (size_t i = 0; i < n_items; i++) {
			const int32_t* h = items + 3 * i;
			uint64_t w[3];
			bool inside = true;
			for (int d = 0; d < 3; d++) {
				const int64_t lo = int64_t(c[d]) + int64_t(h[d]) * len;
				// a local cell's box must lie in the level-0 cells this rank
				// knows (its ghost region); a remote cell's list may be
				// incomplete, as the reference documents (4327-4328)
				if (local) {
					const int64_t own = int64_t(c[d]) / l0;
					if (std::abs(floor_div(lo, l0) - own) > r || std::abs(floor_div(lo + len - 1, l0) - own) > r)
						throw Error(DCCRGX_EINVAL, "neighborhood item beyond the ghost region of this process");
				}
				inside = inside && map_wrap(m, d, lo, w[d]);
			}
			if (!inside) continue;
			for (int l = std::max(0, lvl - 1); l <= std::min(m.R, lvl + 1); l++)
				cand.push_back(map_from_indices(m, w[0], w[1], w[2], l));
		}
		std::sort(cand.begin(), cand.end());
		cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
		std::vector<int32_t> own(cand.size());
		lookup_batch(g, cand.data(), cand.size(), own.data(), nullptr);
		const auto exists = [&](uint64_t id) {
			const auto it = std::lower_bound(cand.begin(), cand.end(), id);
			return it != cand.end() && *it == id && own[size_t(it - cand.begin())] >= 0;
		};
		std::vector<uint64_t> oi;
		std::vector<int32_t> oo;
		ItemOut o;
		for (size_t i = 0; i < n_items; i++) {
			nof_item(m, c, lvl, items + 3 * i, exists, o);
			for (int k = 0; k < o.n; k++) {
				oi.push_back(o.id[k]);
				oo.insert(oo.end(), o.off[k], o.off[k] + 3);
			}
		}
		if (n) *n = oi.size();
		if (oi.size() > cap || (!ids && !oi.empty())) return DCCRGX_ERANGE;
		std::copy(oi.begin(), oi.end(), ids);
		if (offs) std::copy(oo.begin(), oo.end(), offs);
		return 0;
	});
}

int dccrgx_get_face_cache(dccrgx_grid* gp, uint64_t* ids, uint64_t* nbrs, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		const MapCtx& m = g.m;
		std::vector<uint64_t> k;
		std::vector<int32_t> o;
		known_leaves(g, k, o);
		// every leaf under a known level-0 cell is known (own + ghost region)
		std::vector<uint64_t> l0;
		for (uint64_t id : k) l0.push_back(map_level0_parent(m, id));
		std::sort(l0.begin(), l0.end());
		l0.erase(std::unique(l0.begin(), l0.end()), l0.end());
		const auto exists = [&](uint64_t id) { return std::binary_search(k.begin(), k.end(), id); };
		std::vector<uint64_t> oi, on;
		for (uint64_t id : k) {
			uint64_t c[3];
			const int lvl = map_indices(m, id, c[0], c[1], c[2]);
			std::array<uint64_t, 6> e;
			bool known = true;
			for (int dir = 0; dir < 6 && known; dir++) {
				uint64_t p[3], f[4];
				e[size_t(dir)] = error_cell;
				if (!face_probe(m, c, lvl, dir, p)) continue;
				// the probe's level-0 cell must be known for the entry to be exact
				known = std::binary_search(l0.begin(), l0.end(), map_from_indices(m, p[0], p[1], p[2], 0));
				if (known && face_dir(m, c, lvl, dir, exists, f) > 0) e[size_t(dir)] = f[0];
			}
			if (!known) continue;
			oi.push_back(id);
			on.insert(on.end(), e.begin(), e.end());
		}
		if (n) *n = oi.size();
		if (oi.size() > cap || (!ids && !oi.empty())) return DCCRGX_ERANGE;
		std::copy(oi.begin(), oi.end(), ids);
		if (nbrs) std::copy(on.begin(), on.end(), nbrs);
		return 0;
	});
}

int dccrgx_unpin_all_cells(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		g.pins.clear();
		return 0;
	});
}

int dccrgx_get_number_of_update_cells(dccrgx_grid* gp, uint64_t* ns, uint64_t* nr) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		if (ns) *ns = g.halo.n_send;
		if (nr) *nr = g.halo.n_recv;
		return 0;
	});
}

int dccrgx_refine_completely(dccrgx_grid* gp, uint64_t cell) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		return refine_completely(g, cell);
	});
}

int dccrgx_unrefine_completely(dccrgx_grid* gp, uint64_t cell) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		return unrefine_completely(g, cell);
	});
}

// dont_unrefine (2679-2733): the family of a local leaf is not merged by the
// next stop_refining (local requests of its siblings are dropped now)
int dccrgx_dont_unrefine(dccrgx_grid* gp, uint64_t cell) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		if (!is_local_cell(g, cell)) return DCCRGX_ENOTFOUND;
		if (map_level(g.m, cell) == 0) return 0;
		flush_bulk_requests(g);
		uint64_t sib[8];
		map_siblings(g.m, cell, sib);
		for (uint64_t s : sib)
			if (g.dont_unrefine_cells.count(s)) return 0;
		for (uint64_t s : sib) g.unrefine_requests.erase(s);
		g.dont_unrefine_cells.insert(cell);
		return 0;
	});
}

// dont_refine (2744-2784): the local leaf and, in stop_refining, its finer
// neighbors (override_refines) are not refined by request; the spread set
// persists after stop_refining (10039) until balance_load clears it (3812)
int dccrgx_dont_refine(dccrgx_grid* gp, uint64_t cell) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		if (!is_local_cell(g, cell)) return DCCRGX_ENOTFOUND;
		if (map_level(g.m, cell) >= g.R) return 0;
		flush_bulk_requests(g);
		g.refine_requests.erase(cell);
		g.dont_refine_cells.insert(cell);
		return 0;
	});
}

int dccrgx_get_removed_cells(dccrgx_grid* gp, uint64_t* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		return copy_out_u64(g.removed_ids.host(g.s_comp), out, cap, n);
	});
}

int dccrgx_removed_field_download(dccrgx_grid* gp, int fid, void* host, size_t cap_bytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = fixed_field(g, fid);
		const size_t bytes = g.removed_ids.size() * f.elem;
		DX_REQUIRE(cap_bytes >= bytes, "buffer too small for the removed cells' payloads");
		if (bytes) d2h_small(host, f.removed.p, bytes, g.s_comp);
		return 0;
	});
}

int dccrgx_removed_field_device_ptr(dccrgx_grid* gp, int fid, void** ptr) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(ptr, "null pointer");
		*ptr = g.removed_ids.empty() ? nullptr : fixed_field(g, fid).removed.p;
		return 0;
	});
}

int dccrgx_stop_refining(dccrgx_grid* gp, uint64_t* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		stop_refining_impl(g);
		if (!out) {
			if (n) *n = g.new_cells.size();
			return 0;
		}
		return copy_out_u64(g.new_cells.host(g.s_comp), out, cap, n);
	});
}

int dccrgx_get_new_cells(dccrgx_grid* gp, uint64_t* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		return copy_out_u64(g.new_cells.host(g.s_comp), out, cap, n);
	});
}

int dccrgx_set_cells(dccrgx_grid* gp, const uint64_t* ids, const int32_t* owners, size_t n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		DX_REQUIRE(!g.mig.active, "balance_load in progress");
		std::vector<uint64_t> L(ids, ids + n);
		std::vector<int32_t> O(owners, owners + n);
		for (size_t i = 0; i < n; i++) {
			DX_REQUIRE(L[i] != error_cell && L[i] <= g.m.last, "invalid cell id");
			DX_REQUIRE(i == 0 || L[i] > L[i - 1], "cell ids must be strictly ascending");
			DX_REQUIRE(O[i] >= 0 && O[i] < g.size, "invalid owner");
		}
		Mesh nm;
		mesh_from_global(g, nm, L, O);
		rebuild(g, nm);
		g.pins.clear();
		return 0;
	});
}

int dccrgx_pin(dccrgx_grid* gp, uint64_t cell, int process) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(process >= 0 && process < g.size, "invalid process");
		if (!is_local_cell(g, cell)) return DCCRGX_ENOTFOUND;  // 5877-5887: local leaves only
		g.pins[cell] = process;
		return 0;
	});
}

int dccrgx_unpin(dccrgx_grid* gp, uint64_t cell) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		g.pins.erase(cell);
		return 0;
	});
}

int dccrgx_add_neighborhood(dccrgx_grid* gp, int id, const int32_t* offsets, size_t n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		// add_neighborhood 6383-6520: the reference returns false for these
		DX_REQUIRE(id != DCCRGX_DEFAULT_HOOD, "neighborhood id is the default id");
		DX_REQUIRE(!g.uhoods.count(id), "neighborhood id already exists");
		for (size_t i = 0; i < n; i++) {
			const int32_t* o = offsets + 3 * i;
			if (g.hood_len > 0) {
				for (int d = 0; d < 3; d++)
					DX_REQUIRE(unsigned(std::abs(o[d])) <= g.hood_len, "offset outside the default neighborhood");
				DX_REQUIRE(o[0] || o[1] || o[2], "offset (0, 0, 0)");
			} else {
				int zeros = 0;
				for (int d = 0; d < 3; d++) {
					zeros += o[d] == 0;
					DX_REQUIRE(std::abs(o[d]) <= 1, "offset outside the face neighborhood");
				}
				DX_REQUIRE(zeros == 2, "face neighborhood offsets must be unit face offsets");
			}
		}
		UserHood& h = g.uhoods[id];
		h.of.assign(offsets, offsets + 3 * n);
		h.to.resize(h.of.size());
		for (size_t i = 0; i < h.of.size(); i++) h.to[i] = -h.of[i];
		upload(h.d_of, h.of, g.s_comp);
		upload(h.d_to, h.to, g.s_comp);
		HIP_CHECK(hipStreamSynchronize(g.s_comp));
		ensure_uhood(g, id);
		return 0;
	});
}

int dccrgx_remove_neighborhood(dccrgx_grid* gp, int id) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		g.uhoods.erase(id);
		return 0;
	});
}

int dccrgx_get_user_neighbors(dccrgx_grid* gp, int id, uint64_t cell, int kind, uint64_t* ids, int32_t* offs,
                              size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		if (!g.uhoods.count(id)) return DCCRGX_ENOTFOUND;
		const int64_t s = lookup_slot(g, cell);
		if (s < 0 || size_t(s) >= g.n_local) return DCCRGX_ENOTFOUND;
		UserHood& h = ensure_uhood(g, id);
		const DBuf<uint32_t>& ptr = kind == 0 ? h.nof_ptr : h.nto_ptr;
		uint32_t be[2];
		d2h_small(be, ptr.p + s, 8, g.s_comp);
		const size_t k = be[1] - be[0];
		if (n) *n = k;
		if (k > cap) return DCCRGX_ERANGE;
		if (k) {
			d2h_small(ids, (kind == 0 ? h.nof_id.p : h.nto_id.p) + be[0], k * 8, g.s_comp);
			if (offs && kind == 0)
				d2h_small(offs, h.nof_off.p + 3 * size_t(be[0]), k * 12, g.s_comp);
		}
		return 0;
	});
}

int dccrgx_get_user_update_list(dccrgx_grid* gp, int id, int peer, int receive, uint64_t* ids, size_t cap,
                                size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		if (!g.uhoods.count(id)) return DCCRGX_ENOTFOUND;
		UserHood& h = ensure_uhood(g, id);
		const auto& mp = receive ? h.plan.recv_ids : h.plan.send_ids;
		auto it = mp.find(peer);
		static const std::vector<uint64_t> empty;
		return copy_out_u64(it == mp.end() ? empty : it->second, ids, cap, n);
	});
}

int dccrgx_update_copies_of_remote_neighbors_hood(dccrgx_grid* gp, int id) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		if (id == DCCRGX_DEFAULT_HOOD) {
			halo_start(g);
			halo_wait(g);
		} else {
			uhood_halo(g, id);
		}
		return 0;
	});
}

int dccrgx_halo_message_size(dccrgx_grid* gp, int hood, int peer, size_t* sb, size_t* rb) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		size_t a = 0, b = 0;
		halo_message_size(g, hood, peer, a, b);
		if (sb) *sb = a;
		if (rb) *rb = b;
		return 0;
	});
}

int dccrgx_halo_pack(dccrgx_grid* gp, int hood, int peer, void* buf, size_t cap) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		halo_pack_peer(g, hood, peer, static_cast<uint8_t*>(buf), cap);
		return 0;
	});
}

int dccrgx_halo_place(dccrgx_grid* gp, int hood, int peer, const void* buf, size_t bytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		halo_place_peer(g, hood, peer, static_cast<const uint8_t*>(buf), bytes);
		return 0;
	});
}

int dccrgx_balance_load(dccrgx_grid* gp, int use_partitioner) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		initialize_balance_load_impl(g, use_partitioner != 0, nullptr, nullptr, 0);
		continue_balance_load_impl(g);
		finish_balance_load_impl(g);
		return 0;
	});
}

int dccrgx_balance_load_to(dccrgx_grid* gp, const uint64_t* cells, const int32_t* procs, size_t n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		DX_REQUIRE((cells && procs) || !n, "null export list");
		initialize_balance_load_impl(g, false, cells, procs, n);
		continue_balance_load_impl(g);
		finish_balance_load_impl(g);
		return 0;
	});
}

int dccrgx_initialize_balance_load(dccrgx_grid* gp, int use_partitioner, const uint64_t* cells, const int32_t* procs,
                                   size_t n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE((cells && procs) || !n, "null export list");
		initialize_balance_load_impl(g, use_partitioner != 0, cells, procs, n);
		return 0;
	});
}

int dccrgx_make_new_partition(dccrgx_grid* gp, uint64_t* cells, int32_t* procs, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		std::vector<uint64_t> c;
		std::vector<int32_t> o;
		rcb_partition(g, c, o);
		if (n) *n = c.size();
		if (c.size() > cap) return DCCRGX_ERANGE;
		if (!c.empty()) {
			std::copy(c.begin(), c.end(), cells);
			std::copy(o.begin(), o.end(), procs);
		}
		return 0;
	});
}

int dccrgx_set_load_balancing_method(dccrgx_grid* gp, const char* method) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(method, "null method");
		const std::string m(method);
		// the native partitioner is RCB; "NONE" keeps the partition (pins only)
		if (m != "RCB" && m != "NONE") return DCCRGX_EINVAL;
		g.lb_method = m;
		return 0;
	});
}

int dccrgx_get_load_balancing_method(dccrgx_grid* gp, char* out, size_t cap) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(out && cap > g.lb_method.size(), "buffer too small");
		std::memcpy(out, g.lb_method.c_str(), g.lb_method.size() + 1);
		return 0;
	});
}

int dccrgx_set_cell_weight(dccrgx_grid* gp, uint64_t cell, double weight) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "not initialized");
		if (!is_local_cell(g, cell)) return DCCRGX_ENOTFOUND;  // 6225-6235: local leaves only
		// the native partitioner cuts on fixed-point weights: a negative or
		// non-finite weight has no meaning there
		DX_REQUIRE(std::isfinite(weight) && weight >= 0 && weight * 65536.0 < 9.2e18,
		           "cell weight must be finite and non-negative");
		g.weights[cell] = weight;
		return 0;
	});
}

double dccrgx_get_cell_weight(dccrgx_grid* gp, uint64_t cell) {
	const double nan = std::numeric_limits<double>::quiet_NaN();
	if (!gp || !gp->g.initialized) return nan;
	Grid& g = gp->g;
	try {
		if (!is_local_cell(g, cell)) return nan;
	} catch (...) {
		return nan;
	}
	auto it = g.weights.find(cell);
	return it == g.weights.end() ? 1.0 : it->second;
}

int dccrgx_continue_balance_load(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		continue_balance_load_impl(g);
		return 0;
	});
}

int dccrgx_finish_balance_load(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		finish_balance_load_impl(g);
		return 0;
	});
}

int dccrgx_migration_message_size(dccrgx_grid* gp, int peer, size_t* sb, size_t* rb) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		size_t a = 0, b = 0;
		migration_message_size(g, peer, a, b);
		if (sb) *sb = a;
		if (rb) *rb = b;
		return 0;
	});
}

int dccrgx_migration_pack(dccrgx_grid* gp, int peer, void* buf, size_t cap) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		migration_pack_peer(g, peer, static_cast<uint8_t*>(buf), cap);
		return 0;
	});
}

int dccrgx_migration_place(dccrgx_grid* gp, int peer, const void* buf, size_t bytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		for (auto& f : g.fields) f.local_zero = false;
		migration_place_peer(g, peer, static_cast<const uint8_t*>(buf), bytes);
		return 0;
	});
}

int dccrgx_save_grid_data(dccrgx_grid* gp, const char* path, uint64_t offset, const void* header,
                          size_t header_bytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		save_grid_impl(g, path, offset, header, header_bytes);
		return 0;
	});
}

int dccrgx_load_grid_data(dccrgx_grid* gp, const char* path, uint64_t offset, size_t header_bytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		load_grid_impl(g, path, offset, header_bytes);
		return 0;
	});
}

int dccrgx_start_loading_grid_data(dccrgx_grid* gp, const char* path, uint64_t offset, size_t header_bytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		start_load_impl(g, path, offset, header_bytes);
		return 0;
	});
}

int dccrgx_continue_loading_grid_data(dccrgx_grid* gp, int field_id, const uint64_t* sizes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		for (auto& f : g.fields) f.local_zero = false;
		continue_load_impl(g, field_id, sizes);
		return 0;
	});
}

int dccrgx_finish_loading_grid_data(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		finish_load_impl(g);
		return 0;
	});
}

int dccrgx_grid_file_bytes_left(dccrgx_grid* gp, uint64_t* bytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		grid_file_bytes_left(g, bytes);
		return 0;
	});
}

int dccrgx_add_field(dccrgx_grid* gp, const char* name, size_t elem, int transfer, int* fid) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(elem > 0, "element size must be > 0");
		Field f;
		f.name = name ? name : "";
		f.elem = elem;
		f.win_len = elem;
		f.transfer = transfer != 0;
		g.fields.push_back(std::move(f));
		Field& nf = g.fields.back();
		if (g.initialized) {
			nf.data.alloc(g.n_slots * elem);
			if (nf.data.n) HIP_CHECK(hipMemsetAsync(nf.data.p, 0, nf.data.n, g.s_comp));
		}
		*fid = int(g.fields.size() - 1);
		return 0;
	});
}

// ---- variable-size fields (tests/variable_data_size; varfield.hip) ----------
int dccrgx_add_variable_field(dccrgx_grid* gp, const char* name, int transfer, int* fid) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(fid, "null pointer");
		Field f;
		f.name = name ? name : "";
		f.var = true;
		f.transfer = transfer != 0;
		g.fields.push_back(std::move(f));
		if (g.initialized) var_reset(g.fields.back(), g.n_slots, g.s_comp);
		*fid = int(g.fields.size() - 1);
		return 0;
	});
}

static Field& var_field(Grid& g, int fid, size_t slot0, size_t n) {
	Field& f = field(g, fid);
	DX_REQUIRE(f.var, "not a variable-size field");
	DX_REQUIRE(g.initialized, "not initialized");
	DX_REQUIRE(slot0 + n <= g.n_slots, "slot range out of bounds");
	return f;
}

int dccrgx_variable_field_sizes(dccrgx_grid* gp, int fid, size_t slot0, size_t n, uint64_t* sizes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = var_field(g, fid, slot0, n);
		DX_REQUIRE(sizes || !n, "null pointer");
		const std::vector<uint64_t> o = download(f.voff.p + slot0, n + 1, g.s_comp);
		for (size_t i = 0; i < n; i++) sizes[i] = o[i + 1] - o[i];
		return 0;
	});
}

int dccrgx_variable_field_resize(dccrgx_grid* gp, int fid, size_t slot0, size_t n, const uint64_t* sizes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = var_field(g, fid, slot0, n);
		DX_REQUIRE(sizes || !n, "null pointer");
		DBuf<uint64_t> all;
		all.alloc(g.n_slots + 1);
		var_sizes(f, nullptr, 0, g.n_slots, all.p, g.s_comp);
		if (n) h2d(all.p + slot0, sizes, n * 8, g.s_comp);
		var_resize(f, g.n_slots, all.p, g.s_comp);
		return 0;
	});
}

int dccrgx_variable_field_upload(dccrgx_grid* gp, int fid, size_t slot0, size_t n, const void* bytes, size_t nbytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = var_field(g, fid, slot0, n);
		uint64_t a = 0, b = 0;
		HIP_CHECK(hipMemcpyAsync(&a, f.voff.p + slot0, 8, hipMemcpyDeviceToHost, g.s_comp));
		d2h_small(&b, f.voff.p + slot0 + n, 8, g.s_comp);
		DX_REQUIRE(nbytes == b - a, "byte count differs from the cells' sizes (resize them first)");
		if (nbytes) {
			HIP_CHECK(hipMemcpyAsync(f.data.p + a, bytes, nbytes, hipMemcpyHostToDevice, g.s_comp));
			HIP_CHECK(hipStreamSynchronize(g.s_comp));
		}
		return 0;
	});
}

int dccrgx_variable_field_download(dccrgx_grid* gp, int fid, size_t slot0, size_t n, void* bytes, size_t cap,
                                   size_t* nbytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = var_field(g, fid, slot0, n);
		uint64_t a = 0, b = 0;
		HIP_CHECK(hipMemcpyAsync(&a, f.voff.p + slot0, 8, hipMemcpyDeviceToHost, g.s_comp));
		d2h_small(&b, f.voff.p + slot0 + n, 8, g.s_comp);
		if (nbytes) *nbytes = size_t(b - a);
		if (b - a > cap) return DCCRGX_ERANGE;
		if (b > a) d2h_small(bytes, f.data.p + a, b - a, g.s_comp);
		return 0;
	});
}

int dccrgx_variable_field_device_ptr(dccrgx_grid* gp, int fid, void** data, const uint64_t** offsets) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = var_field(g, fid, 0, 0);
		if (data) *data = f.data.p;
		if (offsets) *offsets = f.voff.p;
		return 0;
	});
}

int dccrgx_removed_variable_field_download(dccrgx_grid* gp, int fid, uint64_t* sizes, void* bytes, size_t cap,
                                           size_t* nbytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = field(g, fid);
		DX_REQUIRE(f.var, "not a variable-size field");
		const size_t n = g.removed_ids.size();
		if (!n || !f.rm_off.p) {
			if (nbytes) *nbytes = 0;
			return 0;
		}
		const std::vector<uint64_t> o = download(f.rm_off.p, n + 1, g.s_comp);
		if (nbytes) *nbytes = size_t(o[n]);
		if (sizes)
			for (size_t i = 0; i < n; i++) sizes[i] = o[i + 1] - o[i];
		if (o[n] > cap) return DCCRGX_ERANGE;
		if (o[n] && bytes) d2h_small(bytes, f.removed.p, o[n], g.s_comp);
		return 0;
	});
}

// ---- particles in cells (tests/particles; particles.hip) ----------------------
int dccrgx_get_existing_cells_at(dccrgx_grid* gp, const double* xyz, size_t n, uint64_t* ids) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		existing_cells_at(g, xyz, n, ids);
		return 0;
	});
}

int dccrgx_particles_step(dccrgx_grid* gp, int var_field, int record_doubles, const double* velocity, double dt,
                          uint64_t* stats) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_step(g, var_field, record_doubles, velocity, dt, stats);
		return 0;
	});
}

// refined_cell_data (dccrg.hpp:10215-10219) / unrefined_cell_data (10387)
// applied on the device by stop_refining's rebuild, located as
// get_existing_cell (6316-6336)
int dccrgx_particles_follow_mesh(dccrgx_grid* gp, int var_field, int record_doubles) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_follow_set(g, var_field, record_doubles);
		return 0;
	});
}

int dccrgx_particles_adapt_stats(dccrgx_grid* gp, int var_field, uint64_t out[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		const Field& f = field(g, var_field);
		DX_REQUIRE(f.var, "not a variable-size field");
		DX_REQUIRE(out, "null pointer");
		for (int k = 0; k < 3; k++) out[k] = f.adapt_stats[k];
		return 0;
	});
}

// particles <-> cell fields: the two halves of the transfer share one weight
int dccrgx_particles_deposit(dccrgx_grid* gp, int var_field, int record_doubles, int shape, int weight_double,
                             int out_field, int per_volume) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_deposit(g, var_field, record_doubles, shape, weight_double, out_field, per_volume);
		return 0;
	});
}

int dccrgx_particles_gather(dccrgx_grid* gp, int var_field, int record_doubles, int shape, const int* cell_fields,
                            int n, int first_double) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_gather(g, var_field, record_doubles, shape, cell_fields, n, first_double);
		return 0;
	});
}

int dccrgx_particles_accelerate(dccrgx_grid* gp, int var_field, int record_doubles, int first_double,
                                int weight_double, double factor) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_accelerate(g, var_field, record_doubles, first_double, weight_double, factor);
		return 0;
	});
}

int dccrgx_particles_deposit_moments(dccrgx_grid* gp, int var_field, int record_doubles, int shape, int weight_double,
                                     const int* factors, const int* out_fields, int n, int per_volume) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_deposit_moments(g, var_field, record_doubles, shape, weight_double, factors, out_fields, n,
		                          per_volume);
		return 0;
	});
}

int dccrgx_particles_boris(dccrgx_grid* gp, int var_field, int record_doubles, int e_first, int b_first,
                           int weight_double, double factor) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_boris(g, var_field, record_doubles, e_first, b_first, weight_double, factor);
		return 0;
	});
}

int dccrgx_particles_create(dccrgx_grid* gp, int var_field, int record_doubles, int count_field, double count,
                            int round_random, const int* recipe_i, const double* recipe_d, uint64_t seed,
                            uint64_t* created) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_create(g, var_field, record_doubles, count_field, count, round_random, recipe_i, recipe_d, seed,
		                 created);
		return 0;
	});
}

int dccrgx_particles_remove(dccrgx_grid* gp, int var_field, int record_doubles, const int* test_i, const double* test_d,
                            int n_tests, int mask_field, int prob_field, double prob, uint64_t seed, int rescale,
                            int weight_double, const int* tally_factors, const int* tally_fields, int n_tally,
                            int into_field, uint64_t stats[4]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_remove(g, var_field, record_doubles, test_i, test_d, n_tests, mask_field, prob_field, prob, seed,
		                 rescale, weight_double, tally_factors, tally_fields, n_tally, into_field, stats);
		return 0;
	});
}

// cells_to_send / cells_to_receive while a balance_load is in progress
// (initialize_balance_load fills them with the migration lists, 3746-3884)
int dccrgx_get_migration_cells(dccrgx_grid* gp, int peer, int incoming, uint64_t* ids, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.mig.active, "no balance_load in progress");
		const auto& m = incoming ? g.mig.in : g.mig.out;
		const auto it = m.find(peer);
		const size_t k = it == m.end() ? 0 : it->second.size();
		if (n) *n = k;
		if (k > cap) return DCCRGX_ERANGE;
		for (size_t i = 0; i < k; i++) ids[i] = it->second[i];
		return 0;
	});
}

// set_send_single_cells 6677 / get_send_single_cells 6684: on, the halo's
// fixed-size payloads go on the wire one cell at a time (comm.hip
// wire_pieces); the received payloads are the same either way
int dccrgx_set_send_single_cells(dccrgx_grid* gp, int on) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		g.send_single_cells = on != 0;
		return 0;
	});
}

int dccrgx_get_send_single_cells(dccrgx_grid* gp, int* on) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(on, "null pointer");
		*on = g.send_single_cells ? 1 : 0;
		return 0;
	});
}

int dccrgx_set_field_transfer(dccrgx_grid* gp, int fid, int transfer) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field(g, fid).transfer = transfer != 0;
		return 0;
	});
}

int dccrgx_set_field_window(dccrgx_grid* gp, int fid, size_t offset, size_t bytes) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = fixed_field(g, fid);
		DX_REQUIRE(offset + bytes <= f.elem && bytes > 0, "window outside the element");
		f.win_off = offset;
		f.win_len = bytes;
		return 0;
	});
}

int dccrgx_field_device_ptr(dccrgx_grid* gp, int fid, void** ptr) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field(g, fid).local_zero = false;
		Field& f = fixed_field(g, fid);
		field_written(f);
		f.external = true;  // writes through the pointer are not seen
		*ptr = f.data.p;
		return 0;
	});
}

int dccrgx_field_upload(dccrgx_grid* gp, int fid, size_t slot0, size_t n, const void* host) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field(g, fid).local_zero = false;
		Field& f = fixed_field(g, fid);
		DX_REQUIRE(slot0 + n <= g.n_slots, "slot range out of bounds");
		field_written(f);
		HIP_CHECK(hipStreamSynchronize(g.s_comp));
		if (n) {
			HIP_CHECK(hipMemcpyAsync(f.data.p + slot0 * f.elem, host, n * f.elem, hipMemcpyHostToDevice, g.s_comp));
			HIP_CHECK(hipStreamSynchronize(g.s_comp));
		}
		return 0;
	});
}

int dccrgx_field_download(dccrgx_grid* gp, int fid, size_t slot0, size_t n, void* host) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		Field& f = fixed_field(g, fid);
		DX_REQUIRE(slot0 + n <= g.n_slots, "slot range out of bounds");
		HIP_CHECK(hipStreamSynchronize(g.s_comp));
		if (n) d2h_small(host, f.data.p + slot0 * f.elem, n * f.elem, g.s_comp);
		return 0;
	});
}

int dccrgx_update_copies_of_remote_neighbors(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		halo_start(g);
		halo_wait(g);
		return 0;
	});
}

int dccrgx_start_remote_neighbor_copy_updates(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		halo_start(g);
		return 0;
	});
}

int dccrgx_wait_remote_neighbor_copy_update_receives(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		halo_wait(g);
		return 0;
	});
}

int dccrgx_wait_remote_neighbor_copy_update_sends(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		halo_wait(g);
		return 0;
	});
}

int dccrgx_wait_remote_neighbor_copy_updates(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		halo_wait(g);
		return 0;
	});
}

int dccrgx_gol_step(dccrgx_grid* gp, int sf, int region) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		gol_step(g, sf, region);
		return 0;
	});
}

int dccrgx_gol_commit(dccrgx_grid* gp, int sf) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		commit(g, field(g, sf));
		return 0;
	});
}

// ---- refined game of life (tests/game_of_life/solve.hpp; gol_amr.hip) ---------
int dccrgx_gol_amr(dccrgx_grid* gp, int phase, int sf, int lf, int region) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		gol_amr_phase(g, phase, sf, lf, region);
		return 0;
	});
}

int dccrgx_get_live_neighbors(dccrgx_grid* gp, int sf, int lf) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		gol_live_neighbors(g, sf, lf);
		return 0;
	});
}

int dccrgx_advection_step(dccrgx_grid* gp, const int fids[7], double dt, int region) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_step(g, fids, dt, region);
		return 0;
	});
}

int dccrgx_advection_layout(dccrgx_grid* gp, uint64_t out[12]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_layout(g, out);
		return 0;
	});
}

int dccrgx_advection_occupancy(dccrgx_grid* gp, uint64_t out[6]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_occupancy(g, out);
		return 0;
	});
}

int dccrgx_advection_length_source(dccrgx_grid* gp, const int fids[7], int* out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_length_source(g, fids, out);
		return 0;
	});
}

int dccrgx_advection_velocity_source(dccrgx_grid* gp, const int fids[7], int* mask) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_velocity_source(g, fids, mask);
		return 0;
	});
}

int dccrgx_advection_divide_source(dccrgx_grid* gp, const int fids[7], int* out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_divide_source(g, fids, out);
		return 0;
	});
}

int dccrgx_advection_commit(dccrgx_grid* gp, int df) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_commit(g, df);
		return 0;
	});
}

int dccrgx_advection_initialize(dccrgx_grid* gp, const int fids[7]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_initialize(g, fids);
		return 0;
	});
}

int dccrgx_advection_max_time_step(dccrgx_grid* gp, const int fids[7], double* out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_max_time_step(g, fids, out);
		return 0;
	});
}

int dccrgx_advection_max_time_step_device(dccrgx_grid* gp, const int fids[7], double* d_out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_max_time_step_device(g, fids, d_out);
		return 0;
	});
}

int dccrgx_advection_refine_candidates(dccrgx_grid* gp, int df, double diff_increase, double diff_threshold,
                                       uint64_t* out, size_t cap, size_t* n) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		return copy_out_u64(advection_refine_candidates(g, df, diff_increase, diff_threshold), out, cap, n);
	});
}

int dccrgx_advection_check_adaptation(dccrgx_grid* gp, int df, double diff_increase, double diff_threshold,
                                      double unrefine_sensitivity, uint64_t counts[3]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_check_adaptation(g, df, diff_increase, diff_threshold, unrefine_sensitivity, counts);
		return 0;
	});
}

int dccrgx_advection_adapt(dccrgx_grid* gp, const int fids[7], uint64_t out[2]) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		advection_adapt(g, fids, out);
		return 0;
	});
}

int dccrgx_allreduce_f64(dccrgx_grid* gp, double* v, int count, int op) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		comm_allreduce_f64(g, v, count, op);
		return 0;
	});
}

int dccrgx_allreduce_f64_device(dccrgx_grid* gp, const double* d_in, double* d_out, int count, int op) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(count >= 0 && (count == 0 || (d_in && d_out)), "allreduce: null device buffer");
		comm_allreduce_f64_dev(g, d_in, d_out, count, op, g.s_comp);
		return 0;
	});
}

int dccrgx_barrier(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		HIP_CHECK(hipStreamSynchronize(g.s_comp));
		double z = 0;
		comm_allreduce_f64(g, &z, 1, 0);
		return 0;
	});
}

int dccrgx_get_transport(dccrgx_grid* gp, int* kind, int* comm_ranks) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		int k = DCCRGX_TRANSPORT_NONE, n = 1;
		if (g.xfn) {
			k = DCCRGX_TRANSPORT_HOST;
			n = g.size;
		} else if (g.nccl) {
			k = DCCRGX_TRANSPORT_RCCL;
			NCCL_CHECK(ncclCommCount(g.nccl, &n));
		}
		if (kind) *kind = k;
		if (comm_ranks) *comm_ranks = n;
		return 0;
	});
}

int dccrgx_comm_loopback(dccrgx_grid* gp, int field_id, size_t slot0, size_t n, size_t dst_slot0) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.nccl && !g.xfn, "loopback needs the RCCL transport");
		Field& f = field(g, field_id);
		DX_REQUIRE(!f.var, "loopback of a variable-size field");
		DX_REQUIRE(slot0 + n <= g.n_slots && dst_slot0 + n <= g.n_slots, "slot range beyond the field");
		DX_REQUIRE(slot0 + n <= dst_slot0 || dst_slot0 + n <= slot0, "overlapping slot ranges");
		f.local_zero = false;  // the receive may land in local slots
		field_written(f);
		HIP_CHECK(hipStreamSynchronize(g.s_comp));  // the field's producers
		comm_loopback(g, f.data.p + slot0 * f.elem, f.data.p + dst_slot0 * f.elem, n * f.elem,
		              g.send_single_cells ? f.elem : 0, g.s_comm);
		HIP_CHECK(hipStreamSynchronize(g.s_comm));
		return 0;
	});
}

int dccrgx_synchronize(dccrgx_grid* gp) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		HIP_CHECK(hipStreamSynchronize(g.s_comm));
		HIP_CHECK(hipStreamSynchronize(g.s_comp));
		return 0;
	});
}

void* dccrgx_compute_stream(dccrgx_grid* gp) { return gp ? (void*)gp->g.s_comp : nullptr; }

int dccrgx_kernel_timing(dccrgx_grid* gp, int enable, double* total_ms, int64_t* count) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		drain_timing(g);
		if (total_ms) *total_ms = g.timed_ms;
		if (count) *count = g.timed_count;
		if (enable == 1) {
			g.timing = true;
			g.timed_ms = 0;
			g.timed_count = 0;
		} else if (enable == 0) {
			g.timing = false;
		}
		return 0;
	});
}

// ---- Poisson (tests/poisson/poisson_solve.hpp) ----------------------------
int dccrgx_poisson_cache(dccrgx_grid* gp, int rhs_field, int solution_field, const uint64_t* solve_cells,
                         size_t n_solve, const uint64_t* skip_cells, size_t n_skip) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(g.initialized, "grid not initialized");
		DX_REQUIRE((solve_cells || !n_solve) && (skip_cells || !n_skip), "null cell list");
		poisson_cache(g, rhs_field, solution_field, solve_cells, n_solve, skip_cells, n_skip);
		return 0;
	});
}

int dccrgx_poisson_solve(dccrgx_grid* gp, unsigned max_iterations, unsigned min_iterations, double stop_residual,
                         double p_of_norm, double stop_after_residual_increase, int failsafe, unsigned* iterations,
                         double* residual) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		poisson_solve(g, max_iterations, min_iterations, stop_residual, p_of_norm, stop_after_residual_increase,
		              failsafe != 0, iterations, residual);
		return 0;
	});
}

int dccrgx_poisson_field(dccrgx_grid* gp, const char* name, int* fid) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(name && fid, "null argument");
		*fid = poisson_field(g, name);
		return 0;
	});
}

// ---- operators on fp64 cell fields (field_ops.hip) ------------------------------
int dccrgx_gradient(dccrgx_grid* gp, int in_field, const int out_fields[3], double scale, int region) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field_gradient(g, in_field, out_fields, scale, region);
		return 0;
	});
}

// cell fields follow the mesh: restriction and prolongation of a fixed fp64
// field inside stop_refining (field_adapt.hip)
int dccrgx_field_follow_mesh(dccrgx_grid* gp, int field_id, int mode) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field_follow_set(g, field_id, mode);
		return 0;
	});
}

int dccrgx_field_follow_mode(dccrgx_grid* gp, int field_id, int* mode) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(mode, "null pointer");
		const Field& f = fixed_field(g, field_id);
		DX_REQUIRE(f.elem == 8, "a field that follows the mesh must be a fixed-size field of 8-byte elements (fp64)");
		*mode = f.follow_mode;
		return 0;
	});
}

int dccrgx_curl(dccrgx_grid* gp, const int in_fields[3], const int out_fields[3], double scale, int accumulate,
                int region) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field_curl(g, in_fields, out_fields, scale, accumulate != 0, region);
		return 0;
	});
}

int dccrgx_divergence(dccrgx_grid* gp, const int in_fields[3], int out_field, double scale, int accumulate,
                      int region) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field_divergence(g, in_fields, out_field, scale, accumulate != 0, region);
		return 0;
	});
}

int dccrgx_field_axpy(dccrgx_grid* gp, int y_field, double a, int x_field, int region) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field_axpy(g, y_field, a, x_field, region);
		return 0;
	});
}

int dccrgx_field_reduce_device(dccrgx_grid* gp, const int* terms, int n, int by_volume, int region, int collective,
                               double* d_out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		field_reduce_device(g, terms, n, by_volume, region, collective, d_out);
		return 0;
	});
}

// the device form into the grid's own doubles, then one synchronising copy
int dccrgx_field_reduce(dccrgx_grid* gp, const int* terms, int n, int by_volume, int region, int collective,
                        double* out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(out, "null pointer");
		g.red_val.reserve(kRedTerms);
		field_reduce_device(g, terms, n, by_volume, region, collective, g.red_val.p);
		d2h_small(out, g.red_val.p, size_t(n) * sizeof(double), g.s_comp);
		return 0;
	});
}

int dccrgx_particles_reduce_device(dccrgx_grid* gp, int var_field, int record_doubles, int weight_double,
                                   const int* terms, int n, int collective, double* d_out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		particles_reduce(g, var_field, record_doubles, weight_double, terms, n, collective, d_out);
		return 0;
	});
}

int dccrgx_particles_reduce(dccrgx_grid* gp, int var_field, int record_doubles, int weight_double, const int* terms,
                            int n, int collective, double* out) {
	return guard([&] {
		GRID_OR_FAIL(gp);
		DX_REQUIRE(out, "null pointer");
		g.red_val.reserve(kRedTerms);
		particles_reduce(g, var_field, record_doubles, weight_double, terms, n, collective, g.red_val.p);
		d2h_small(out, g.red_val.p, size_t(n) * sizeof(double), g.s_comp);
		return 0;
	});
}

}  // extern "C"
