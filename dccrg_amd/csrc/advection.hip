// The advection solver's host driver (tests/advection of the reference):
// the sweep, the time step, check_for_adaptation and adapt_grid over device
// fields, and the caches they keep (Grid::DtCache, NbRecords, LenTable,
// VelUniform, BandRec).  The C ABI wrappers are in api.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "dccrgx_grid.hpp"

namespace dccrgx {

// one of the advection switches DCCRGX_NBREC, LEN_TABLE, VEL_UNIFORM,
// DIV_POW2, BAND_CACHE: whether the variable is set to `value` now (read per
// call: tests switch them)
static bool adv_switch(const char* name, int value = 1) {
	const char* e = std::getenv(name);
	return e && std::atoi(e) == value;
}

static void adv_fields(Grid& g, const int fids[7], const double* f[7]) {
	for (int k = 0; k < 7; k++) {
		Field& F = field(g, fids[k]);
		DX_REQUIRE(F.elem == 8, "advection fields must be fp64");
		f[k] = (const double*)F.data.p;
		g.adv_fids[k] = fids[k];  // (dccrgx_advection_layout reports the sweep of these)
	}
	g.adv_fids_valid = true;
}

// the block minima now in g.dt_part (nb of them) belong to fields fids as
// they are now (Grid::DtCache); not kept while one of the six is external
// (its device pointer is out: writes through it are not seen)
static void dt_cache_set(Grid& g, const int fids[7], size_t nb) {
	Grid::DtCache& C = g.dt_cache;
	C.key.take(g, fids + 1);
	C.n_local = g.n_local;
	C.nb = nb;
	C.valid = nb > 0 && C.key.trackable(g, fids + 1);
}

// The neighbor records of the tile sweeps (Grid::NbRecords) for the fields
// fids: kept while the six velocity / length fields are the same fields with
// the same write epochs and arrays and the tiles are the same; rebuilt
// otherwise (one pass over the slots, 48 B read + 72 B written per slot, on
// the compute stream, so it follows every queued write of those fields).
// nullptr - the sweeps read the fields - when one of them is external (its
// device pointer is out), when the slots exceed the records' 32-bit indexing,
// and unless DCCRGX_NBREC=1: the records are an experiment that lost (paired
// A/B, DESIGN §5: the record lines are touched by neighbor reads alone, so
// they miss where the field lines hit because the neighbor tile's own reads
// brought them into L2: 0.182 -> 0.235 ms of sweep kernels on config 3).
const double* ensure_nbrec(Grid& g, const int fids[7]) {
	Grid::NbRecords& R = g.nbrec;
	if (!adv_switch("DCCRGX_NBREC") || g.n_slots == 0 || g.n_slots >= (size_t(1) << 29)) return nullptr;
	if (!R.key.trackable(g, fids + 1)) return nullptr;
	if (R.valid && R.tiles_gen == g.tiles_gen && R.n_slots == g.n_slots && R.key.same(g, fids + 1)) return R.r.p;
	const double* f[7];
	adv_fields(g, fids, f);
	R.r.alloc(9 * g.n_slots);
	k_nbrec(f, g.n_slots, R.r.p, g.s_comp);
	R.key.take(g, fids + 1);
	R.tiles_gen = g.tiles_gen;
	R.n_slots = g.n_slots;
	R.valid = true;
	return R.r.p;
}

// a finite, positive, normal double with a zero mantissa
static bool normal_pow2(double x) {
	uint64_t b;
	std::memcpy(&b, &x, sizeof(b));
	const uint64_t e = (b >> 52) & 0x7ffu;
	return (b >> 63) == 0 && e != 0 && e != 0x7ffu && (b & ((uint64_t(1) << 52) - 1)) == 0;
}

// The reciprocals behind the 96 lengths of table h (kLenTabP2 doubles): per
// level 1 / (2 l_a), the divisor of a face between two cells of that level,
// and 1 / (lx ly lz), the product in the kernels' operand order.  True when
// the sweeps may multiply by them instead of dividing: each l0 and, at every
// level, each length, divisor and reciprocal is a normal power of two, so
// the reciprocal is exact and the product rounds the real number the
// quotient rounds.  One verdict for the three axes; the entries are written
// either way (a false verdict leaves them unread).
static bool len_table_reciprocals(const double l0[3], double* h) {
	bool ok = normal_pow2(l0[0]) && normal_pow2(l0[1]) && normal_pow2(l0[2]);
	auto reciprocal = [&](double d) {
		const double r = 1.0 / d;
		ok = ok && normal_pow2(d) && normal_pow2(r) && r * d == 1.0;
		return r;
	};
	for (int lvl = 0; lvl < 32; lvl++) {
		const double* row = h + 3 * lvl;
		for (int d = 0; d < 3; d++) {
			ok = ok && normal_pow2(row[d]);
			h[96 + 3 * lvl + d] = reciprocal(row[d] + row[d]);
		}
		h[192 + lvl] = reciprocal(row[0] * row[1] * row[2]);
	}
	return ok;
}

// The per-level length table of the tile sweeps (Grid::LenTable) for the
// fields fids, or nullptr: the sweeps read the length fields.  The table is
// l0[d] * (1 / 2^level), the expression of dccrgx_advection_initialize and of
// advection_adapt's reset pass, so on a Cartesian grid whose length fields
// were set by either (or by geometry.get_length) every slot's lengths are
// bitwise its level's row.  That is verified, not assumed: one pass over all
// slots (remote copies too, the sweeps read them as neighbors) on the compute
// stream, one flag read back, cached on the tiles, the slot count, l0 and the
// three fields' ids, write epochs and arrays.  A key found changed at two
// sweeps in a row means the lengths are rewritten every step: the fields are
// then read without checking until a sweep finds the key unchanged.
const double* ensure_len_table(Grid& g, const int fids[7], bool sweep) {
	Grid::LenTable& L = g.lentab;
	// (the record kernels do not take the table)
	if (adv_switch("DCCRGX_LEN_TABLE", 0) || adv_switch("DCCRGX_NBREC")) return nullptr;
	if (!g.geo_block.empty() || g.n_slots == 0 || !g.tiles_valid) return nullptr;
	if (!L.key.trackable(g, fids + 4)) return nullptr;
	if (L.keyed && L.tiles_gen == g.tiles_gen && L.n_slots == g.n_slots && L.key.same(g, fids + 4) &&
	    std::equal(L.l0, L.l0 + 3, g.l0)) {
		if (sweep) L.changed = 0;
		if (L.checked) return L.ok ? L.tab.p : nullptr;
	} else {
		L.key.take(g, fids + 4);
		std::copy(g.l0, g.l0 + 3, L.l0);
		L.tiles_gen = g.tiles_gen;
		L.n_slots = g.n_slots;
		L.keyed = true;
		L.checked = false;
		if (sweep && ++L.changed >= 2) return nullptr;
	}
	if (!L.tab.p || L.tab_l0[0] != g.l0[0] || L.tab_l0[1] != g.l0[1] || L.tab_l0[2] != g.l0[2]) {
		double h[kLenTabP2];
		for (int lvl = 0; lvl < 32; lvl++)
			for (int d = 0; d < 3; d++) h[3 * lvl + d] = g.l0[d] * (1.0 / double(uint64_t(1) << lvl));
		L.pow2 = len_table_reciprocals(g.l0, h);
		L.tab.alloc(kLenTabP2);
		L.flag.alloc(1);
		h2d(L.tab.p, h, sizeof(h), g.s_comp);
		HIP_CHECK(hipStreamSynchronize(g.s_comp));  // h is a local
		for (int d = 0; d < 3; d++) L.tab_l0[d] = g.l0[d];
	}
	const double* f[7];
	for (int k = 0; k < 7; k++) f[k] = (const double*)field(g, fids[k]).data.p;
	k_len_check(f, g.slot_lvl.p, g.n_slots, L.tab.p, L.flag.p, g.s_comp);
	int bad = 1;
	d2h_small(&bad, L.flag.p, sizeof(int), g.s_comp);
	L.ok = bad == 0;
	L.checked = true;
	return L.ok ? L.tab.p : nullptr;
}

// The uniform velocity components of the tile sweeps (Grid::VelUniform) for
// the fields fids: verified as ensure_len_table verifies the lengths - one
// pass over all slots (remote copies too) on the compute stream, one small
// copy back - and cached on the tiles, the slot count and the three fields'
// ids, write epochs (epoch, not local_epoch: halo receives count) and arrays.
// While the key is found changed sweep after sweep (advection_adapt rewrites
// the velocities every step) no pass is made and the fields are read.
VelMask ensure_vel_uniform(Grid& g, const int fids[7], bool sweep, const double* len) {
	Grid::VelUniform& U = g.veluni;
	VelMask none;
	if (adv_switch("DCCRGX_VEL_UNIFORM", 0) || g.n_slots == 0) return none;
	if (!U.key.trackable(g, fids + 1)) return none;
	// (the key is followed while the sweeps read the length fields too: when
	// advection_adapt stops, both verdicts return at the same sweep)
	if (U.keyed && U.tiles_gen == g.tiles_gen && U.n_slots == g.n_slots && U.key.same(g, fids + 1)) {
		if (sweep) U.changed = 0;
	} else {
		U.key.take(g, fids + 1);
		U.tiles_gen = g.tiles_gen;
		U.n_slots = g.n_slots;
		U.keyed = true;
		U.checked = false;
		if (sweep) ++U.changed;
	}
	if (!len) return none;
	if (!U.checked) {
		if (U.changed >= 2) return none;
		const double* f[7];
		for (int k = 0; k < 7; k++) f[k] = (const double*)field(g, fids[k]).data.p;
		U.out.alloc(4);
		k_vel_check(f, g.n_slots, U.out.p, g.s_comp);
		uint64_t h[4] = {7, 0, 0, 0};
		d2h_small(h, U.out.p, sizeof(h), g.s_comp);
		U.mask = int(~h[0] & 7u);
		std::memcpy(U.v, h + 1, sizeof(U.v));
		U.checked = true;
	}
	VelMask r;
	r.mask = U.mask;
	std::copy(U.v, U.v + 3, r.v);
	return r;
}

// What a tile sweep of fields fids runs with, for every caller that sweeps
// or reports on the sweep.  The four rules are written here and nowhere
// else: the records exclude the table; a uniform component needs the table
// and no records; the masks exist only in the register-length / level-row
// builds of the length-table kernels (kRegMasks / kGenMasks); the kernels
// multiply by the table's reciprocals (pow2) with the table, where the host
// found every divisor a power of two (LenTable::pow2), in those builds, and
// unless DCCRGX_DIV_POW2=0.
AdvSweepPlan adv_sweep_plan(Grid& g, const int fids[7], bool sweep) {
	AdvSweepPlan P;
	P.rec = ensure_nbrec(g, fids);
	const double* len = ensure_len_table(g, fids, sweep);
	// (the velocity key is followed whichever kernels run)
	const VelMask vm = ensure_vel_uniform(g, fids, sweep, len);
	P.len = P.rec ? nullptr : len;
	const int um = P.len ? vm.mask : 0;
	P.um[0] = kRegMasks ? um : 0;
	P.um[1] = kGenMasks ? um : 0;
	std::copy(vm.v, vm.v + 3, P.uv);
	P.pow2 = P.len && g.lentab.pow2 && kRegMasks && kGenMasks && !adv_switch("DCCRGX_DIV_POW2", 0);
	return P;
}

void advection_step(Grid& g, const int fids[7], double dt, int region) {
	const double* f[7];
	adv_fields(g, fids, f);
	Field& rho = field(g, fids[0]);
	ensure_scratch(g, rho);
	size_t s0, s1;
	region_range(g, region, s0, s1);
	if (s1 <= s0) return;
	DX_LAPS(g.s_comp);
	// tiles for a mesh already swept once (DCCRGX_TILES=always / never
	// overrides): building them costs ~10 sweeps, so the first step on a
	// freshly adapted mesh sweeps the face table (bitwise the same
	// densities)
	static const char* tp = std::getenv("DCCRGX_TILES");
	const bool tiles = g.tiles_valid || (tp && std::strcmp(tp, "always") == 0) ||
	                   (!(tp && std::strcmp(tp, "never") == 0) && g.adv_commits_on_mesh > 0);
	if (tiles) ensure_tiles(g);
	else ensure_face(g);
	DX_LAP("step.0_ensure_tiles");
	if (tiles) {
		// (outside the timed interval: a rebuild happens once per mesh or
		// field change, not per step)
		const AdvSweepPlan plan = adv_sweep_plan(g, fids, true);
		DX_LAP("step.0_nbrec");
		k_time_begin(g);
		// tiles never straddle the inner / outer runs
		if (s0 < g.n_inner) k_advection_tiles(f, (double*)rho.scratch.p, g, 0, dt, g.s_comp, plan);
		if (s1 > g.n_inner) k_advection_tiles(f, (double*)rho.scratch.p, g, 1, dt, g.s_comp, plan);
	} else {
		// the bands of the check that follows computed by the sweep (with the
		// last check's parameters), recorded per run for band_cache_ok
		const bool bands = g.band_params_valid && !adv_switch("DCCRGX_BAND_CACHE", 0) && FieldKey<1>::trackable(g, fids);
		BandArgs B{};
		if (bands) {
			if (g.band_cache.n < g.n_local + 1) {
				g.band_cache.alloc(g.n_local + 1);
				g.band_rec[0].valid = g.band_rec[1].valid = false;
			}
			B = BandArgs{g.m, g.slot_lvl.p, g.slot_ids.p, g.band_inc, g.band_thr, g.band_uns, g.band_cache.p};
			FieldKey<1> now;
			now.take(g, fids);
			for (int run = 0; run < 2; run++) {
				const size_t r0 = run == 0 ? 0 : g.n_inner, r1 = run == 0 ? g.n_inner : g.n_local;
				if (r1 > r0 && s0 <= r0 && s1 >= r1) g.band_rec[run] = Grid::BandRec{true, g.face_gen, now};
			}
		}
		k_time_begin(g);
		k_advection_ell(f, (double*)rho.scratch.p, g.face_ell.p, g.face_fine.p, s0, s1, dt, g.s_comp,
		                bands ? &B : nullptr);
	}
	k_time_end(g);
	DX_LAP("step.1_sweep");
}

void advection_layout(Grid& g, uint64_t out[12]) {
	DX_REQUIRE(out, "null output");
	ensure_tiles(g);
	const uint64_t nt = g.n_tiles_inner + g.n_tiles_outer;
	uint32_t entries = 0;
	d2h_small(&entries, g.face_ptr.p + g.n_local, 4, g.s_comp);
	const uint64_t n = g.n_local;
	out[0] = uint64_t(g.tile);
	out[1] = nt;
	out[2] = g.total_ext;
	out[3] = g.max_ext;
	out[4] = g.n_fine_faces;
	out[5] = entries;
	// 64 B per cell (7 fp64 fields read, density written) +
	// the face CSR (4 B per entry + 4 B row pointer)
	out[6] = 64 * n + 4 * (n + 1) + 4 * uint64_t(entries);
	out[7] = 64 * n;
	const size_t nreg = g.tcount[0] + g.tcount[1];
	out[8] = nreg;
	out[9] = 512 * nreg;
	uint64_t ext_reg = 0, ext_reg_ax[3] = {0, 0, 0};  // (per axis of the side)
	if (nreg) {
		std::vector<RegTileMeta> rm(nreg);
		d2h_small(rm.data(), g.tregmeta.p, nreg * sizeof(RegTileMeta), g.s_comp);
		for (const auto& r : rm)
			for (int d = 0; d < 6; d++) ext_reg_ax[d >> 1] += r.nst[d] >= 0 ? 64 : 0;
		ext_reg = ext_reg_ax[0] + ext_reg_ax[1] + ext_reg_ax[2];
	}
	out[10] = ext_reg;
	// 40 B per out-of-tile neighbor from the fields (density, three
	// lengths, the velocity along the face); 32 B with the records
	// (DCCRGX_NBREC=1, ensure_nbrec)
	uint64_t per_ext = adv_switch("DCCRGX_NBREC") ? 32 : 40;
	const uint64_t n_irr_cells = n - out[9], ext_irr = g.total_ext - ext_reg;
	// with the per-level length table (ensure_len_table, for the fields
	// last passed to an advection call): an out-of-tile neighbor is its
	// density and one velocity (+ a level byte in the other tiles), an own
	// cell 40 B (+ a level byte) instead of 64 B
	uint64_t own = 64, lvl_byte = 0, uniform = 0;
	const AdvSweepPlan plan = g.adv_fids_valid ? adv_sweep_plan(g, g.adv_fids, false) : AdvSweepPlan{};
	if (plan.len) {
		per_ext = 16;
		lvl_byte = 1;
		if (DCCRGX_LEN_OWN) own = 40;
		// a uniform velocity component (ensure_vel_uniform) is not read: 8 B
		// less per own cell and component, per regular out-of-tile neighbor
		// across a side of its axis, and per general out-of-tile entry all of
		// whose axis bits are uniform (it is then its density alone; an entry
		// with another axis bit still counts the one velocity of per_ext)
		const int um = plan.um[0];
		if (um) {
			Grid::VelUniform& U = g.veluni;
			if (!U.ext_valid || U.ext_gen != g.tiles_gen) {
				DBuf<uint64_t> d;
				d.alloc(8);
				const size_t ni = g.tmeta.n ? g.tcount[2] + g.tcount[3] : 0;
				k_ext_axis_count(g.tmeta.p, ni, g.ext_pk.p, d.p, g.s_comp);
				d2h_small(U.ext_ax, d.p, sizeof(U.ext_ax), g.s_comp);
				U.ext_gen = g.tiles_gen;
				U.ext_valid = true;
			}
			for (int a = 0; a < 3; a++)
				if ((um >> a) & 1) uniform += 8 * n + 8 * ext_reg_ax[a];
			for (int ax = 1; ax < 8; ax++)
				if ((ax & ~um) == 0) uniform += 8 * U.ext_ax[ax];
		}
	}
	out[11] = own * n + (12 + (own == 40 ? lvl_byte : 0)) * n_irr_cells + (per_ext + lvl_byte + 4) * ext_irr +
	          per_ext * ext_reg + 8 * uint64_t(g.n_fine_faces) + 32 * nt - uniform;
}

void advection_occupancy(Grid& g, uint64_t out[6]) {
	DX_REQUIRE(out, "null output");
	ensure_tiles(g);
	// the launch of the fields last passed to an advection call (before
	// the first sweep: the one it will make)
	const AdvSweepPlan plan = g.adv_fids_valid ? adv_sweep_plan(g, g.adv_fids, false) : AdvSweepPlan{};
	for (int kind = 0; kind < 2; kind++) {
		const Grid::SweepLaunch& L = adv_sweep_launch(g, kind, plan);
		int k = 0;
		HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&k, L.fn, 512, L.lds));
		out[3 * kind] = uint64_t(L.blocks_per_cu);
		out[3 * kind + 1] = uint64_t(k);
		out[3 * kind + 2] = L.lds;
	}
}

void advection_length_source(Grid& g, const int fids[7], int* out) {
	DX_REQUIRE(out, "null output");
	const double* f[7];
	adv_fields(g, fids, f);
	ensure_tiles(g);
	*out = adv_sweep_plan(g, fids, false).len ? 1 : 0;
}

void advection_velocity_source(Grid& g, const int fids[7], int* mask) {
	DX_REQUIRE(mask, "null output");
	const double* f[7];
	adv_fields(g, fids, f);
	ensure_tiles(g);
	*mask = adv_sweep_plan(g, fids, false).um[0];
}

void advection_divide_source(Grid& g, const int fids[7], int* out) {
	DX_REQUIRE(out, "null output");
	const double* f[7];
	adv_fields(g, fids, f);
	ensure_tiles(g);
	*out = adv_sweep_plan(g, fids, false).pow2 ? 1 : 0;
}

void advection_commit(Grid& g, int df) {
	commit(g, field(g, df));
	g.adv_commits_on_mesh++;
}

// tests/advection/initialize.hpp:36-82 + Cartesian_Geometry get_center /
// get_length (dccrg_cartesian_geometry.hpp:282-362), evaluated on the host
// with the reference's expression order so the initial state is bitwise the
// reference's.  With an active stretched geometry the center and the length
// are Stretched_Cartesian_Geometry's (initialize.hpp:45-46 take them from the
// grid's geometry, whichever it is).
void advection_initialize(Grid& g, const int fids[7]) {
	// local cells and remote copies alike: the analytic initial state of a
	// remote copy is what initialize() + update_copies_of_remote_neighbors()
	// with transfer_all_data = true would deliver (initialize.hpp:80)
	const auto& ids = slot_ids_host(g);
	const size_t n = g.n_slots;
	for (int k = 0; k < 7; k++) g.adv_fids[k] = fids[k];
	g.adv_fids_valid = true;
	const bool stretched = g.str.active;
	for (int d = 0; d < 3 && stretched; d++)
		DX_REQUIRE(g.str.c[d].size() == g.len[d] + 1, "the grid's length changed after set_stretched_geometry");
	std::vector<double> a[7];
	for (auto& v : a) v.resize(n);
	for (size_t i = 0; i < n; i++) {
		uint64_t ind[3];
		const int lvl = map_indices(g.m, ids[i], ind[0], ind[1], ind[2]);
		const double sf = 1.0 / double(uint64_t(1) << lvl);
		double L[3], c[3];
		if (stretched) {  // dccrgx_geometry_batch's expressions
			for (int d = 0; d < 3; d++) {
				const std::vector<double>& x = g.str.c[d];
				const uint64_t l0i = uint64_t(1) << g.R, i0 = ind[d] / l0i;
				L[d] = (x[i0 + 1] - x[i0]) / double(uint64_t(1) << lvl);
				const double length_of_index = (x[i0 + 1] - x[i0]) / double(l0i);
				c[d] = x[i0] + length_of_index * double(ind[d] - i0 * l0i) + L[d] / 2;
			}
		} else {
			for (int d = 0; d < 3; d++) L[d] = g.l0[d] * sf;
			for (int d = 0; d < 3; d++)
				c[d] = g.start[d] + double(ind[d]) * g.l0[d] / double(uint64_t(1) << g.R) + L[d] / 2;
		}
		const double radius = 0.15;
		const double hr = std::min(std::sqrt(std::pow(c[0] - 0.25, 2.0) + std::pow(c[1] - 0.5, 2.0)), radius) / radius;
		a[0][i] = 0.25 * (1 + std::cos(M_PI * hr));
		a[1][i] = -c[1] + 0.5;
		a[2][i] = +c[0] - 0.5;
		a[3][i] = 0;
		a[4][i] = L[0];
		a[5][i] = L[1];
		a[6][i] = L[2];
	}
	for (int k = 0; k < 7; k++) {
		Field& F = field(g, fids[k]);
		DX_REQUIRE(F.elem == 8, "advection fields must be fp64");
		field_written(F);
		if (n) {
			HIP_CHECK(hipMemcpyAsync(F.data.p, a[k].data(), n * 8, hipMemcpyHostToDevice, g.s_comp));
			HIP_CHECK(hipStreamSynchronize(g.s_comp));
		}
	}
}

// the block minima of the time-step bound of fields fids in g.dt_part (their
// count): the cached ones while the six velocity / length fields are
// unwritten since (advection_adapt's reset pass leaves them), else one pass.
// While one of them is external (its device pointer is out, writes through
// it are not seen) the minima are neither reused nor kept, as ensure_nbrec.
static size_t dt_partials(Grid& g, const int fids[7]) {
	const double* f[7];
	adv_fields(g, fids, f);
	Grid::DtCache& C = g.dt_cache;
	if (C.key.trackable(g, fids + 1) && C.valid && C.n_local == g.n_local && C.nb > 0 && C.key.same(g, fids + 1))
		return C.nb;
	const size_t nb = 512;
	g.dt_part.reserve(kDtPartials);
	k_adv_dt(f, g.n_local, g.dt_part.p, nb, g.s_comp);
	dt_cache_set(g, fids, nb);
	return nb;
}

void advection_max_time_step(Grid& g, const int fids[7], double* out) {
	const size_t nb = dt_partials(g, fids);
	auto h = download(g.dt_part.p, nb, g.s_comp);
	*out = *std::min_element(h.begin(), h.end());
}

void advection_max_time_step_device(Grid& g, const int fids[7], double* d_out) {
	DX_REQUIRE(d_out != nullptr, "null device pointer");
	const size_t nb = dt_partials(g, fids);
	k_min_partials(g.dt_part.p, nb, d_out, g.s_comp);
	comm_allreduce_f64_dev(g, d_out, d_out, 1, 1, g.s_comp);
}

std::vector<uint64_t> advection_refine_candidates(Grid& g, int df, double diff_increase, double diff_threshold) {
	ensure_face(g);
	Field& F = field(g, df);
	DBuf<uint64_t> d;
	d.alloc(g.n_local + 1);
	const FaceView fv{g.face_ell.p, g.face_fine.p, g.slot_ids.p, g.n_local};
	const size_t k = k_adv_candidates(g.m, (const double*)F.data.p, fv, g.slot_lvl.p, g.n_local, diff_increase,
	                                  diff_threshold, d.p, g.s_comp);
	auto v = download(d.p, k, g.s_comp);
	std::sort(v.begin(), v.end());
	return v;
}

// The sweep's bands (advection_step) stand for adv_bands_kernel's when the
// same parameters were given, the face table is the one swept, and the
// density array has not been written since: the inner run reads no remote
// copy, so only local writes matter there; the outer run's rows read the
// copies the halo placed before it.
static bool band_cache_ok(Grid& g, int df, double inc, double thr, double uns) {
	if (!g.band_params_valid || g.band_inc != inc || g.band_thr != thr || g.band_uns != uns) return false;
	if (!FieldKey<1>::trackable(g, &df) || g.band_cache.n < g.n_local + 1 || !g.face_valid) return false;
	for (int run = 0; run < 2; run++) {
		const size_t r0 = run == 0 ? 0 : g.n_inner, r1 = run == 0 ? g.n_inner : g.n_local;
		if (r1 <= r0) continue;
		const Grid::BandRec& R = g.band_rec[run];
		if (!R.valid || R.face_gen != g.face_gen || !R.key.same(g, &df, true)) return false;
		if (run == 1 && !R.key.same(g, &df)) return false;
	}
	return true;
}

// check_for_adaptation (tests/advection/adapter.hpp:47-178) + the requests
// adapt_grid makes from its sets (187-231): per local cell the band of its
// max_diff; band-2 cells are refined, a family with a band-1 member is kept
// (dont_unrefine), a family whose local members are all band 0 is unrefined.
// The reference builds the sets in local-cell order with sibling erasures;
// their outcome per family is the one above, whatever the order.  A family
// with a band-2 member is also marked kept: on one process the reference's
// sibling erasure keeps it even when that member is at the maximum level
// (whose refine request is a no-op); marking it makes every partition give
// that one-process outcome.
void advection_check_adaptation(Grid& g, int df, double diff_increase, double diff_threshold,
                                      double unrefine_sensitivity, uint64_t counts[3]) {
	DX_REQUIRE(g.initialized, "not initialized");
	Field& F = field(g, df);
	DX_REQUIRE(F.elem == 8, "advection fields must be fp64");
	if (counts) counts[0] = counts[1] = counts[2] = 0;
	if (g.R == 0) return;  // 61-63
	DX_LAPS(g.s_comp);
	ensure_face(g);
	DX_LAP("chk.0_face");
	const size_t n = g.n_local;
	DBuf<uint8_t> band_own;
	const uint8_t* band = nullptr;
	if (band_cache_ok(g, df, diff_increase, diff_threshold, unrefine_sensitivity)) {
		band = g.band_cache.p;  // the sweep's (advection_step)
	} else {
		band_own.alloc(n + 1);
		const FaceView fv{g.face_ell.p, g.face_fine.p, g.slot_ids.p, g.n_local};
		k_adv_bands(g.m, (const double*)F.data.p, fv, g.slot_lvl.p, n, diff_increase, diff_threshold,
		            unrefine_sensitivity, band_own.p, g.s_comp);
		band = band_own.p;
	}
	g.band_rec[0].valid = g.band_rec[1].valid = false;
	g.band_params_valid = true;  // the next sweeps compute the bands with these
	g.band_inc = diff_increase;
	g.band_thr = diff_threshold;
	g.band_uns = unrefine_sensitivity;
	DX_LAP("chk.1_bands");
	uint64_t nref = 0, nkeep = 0, nunref = 0;
	// decide one family from its local members (bands bb, ids ii, k of
	// them): dont_unrefine (2679-2733) when any member is kept or refined,
	// else unrefine it
	auto decide = [&](const uint8_t* bb, const uint64_t* ii, size_t k) {
		size_t first2 = k, first1 = k;
		for (size_t i = 0; i < k; i++) {
			if (bb[i] == 2 && first2 == k) first2 = i;
			if (bb[i] == 1 && first1 == k) first1 = i;
		}
		if (first2 != k || first1 != k) {
			// the mark can only cancel an unrefine request of this family: one
			// from another process (a family split across processes, k < 8)
			// or one made earlier here; a whole local family without a pending
			// request needs no mark (the outcome of stop_refining is the same)
			bool pending = k < 8;
			for (size_t i = 0; i < k && !pending && !g.unrefine_requests.empty(); i++)
				pending = g.unrefine_requests.count(ii[i]) != 0;
			if (pending) g.dont_unrefine_cells.insert(ii[first2 != k ? first2 : first1]);
			nkeep++;
		} else if (k == 8) {  // the whole family is local: every sibling a leaf here
			g.unrefine_requests.insert(ii[0]);
			nunref++;
		} else if (unrefine_completely(g, ii[0]) == DCCRGX_OK) {
			nunref++;
		}
	};
	// families: the local members of a parent are consecutive slots on
	// Morton-ordered meshes (a run of 8 is a whole family); shorter runs
	// (a family split between the inner and outer runs, or with members
	// elsewhere) are merged by parent
	std::unordered_map<uint64_t, std::pair<std::vector<uint8_t>, std::vector<uint64_t>>> partial;
	auto add_partial = [&](uint64_t parent, uint8_t band_v, uint64_t id) {
		auto& pr = partial[parent];
		pr.first.push_back(band_v);
		pr.second.push_back(id);
	};
	flush_bulk_requests(g);
	if (g.unrefine_requests.empty() && n < (size_t(1) << 28)) {
		// on the device: refine requests, whole-family decisions, partial runs
		// one process with Morton-ordered slots: each family's leaves are one run
		const bool solo = g.size == 1 && g.morton_slots;
		AdvRequests q = k_adv_requests(g.m, g.dm(), g.slot_ids.p, band, n, solo, g.rank, g.s_comp);
		DX_LAP("chk.2a_device_requests");
		// 2434-2520 (bulk lists: no set hashing of ~20 K ids per step)
		g.refine_bulk.insert(g.refine_bulk.end(), q.refine.begin(), q.refine.end());
		if (g.refine_requests.empty() && !q.refine.empty()) {
			// the whole refine request set: its device copy stays for stop_refining
			g.refine_dev = std::move(q.refine_dev);
			g.refine_dev_valid = true;
		}
		if (g.unrefine_requests.empty() && !q.unrefine.empty()) {
			g.unrefine_dev = std::move(q.unrefine_dev);
			g.unrefine_dev_valid = true;
		}
		nref = q.refine.size();
		nkeep = q.kept;
		g.unrefine_bulk.insert(g.unrefine_bulk.end(), q.unrefine.begin(), q.unrefine.end());
		nunref = q.unrefine.size();
		size_t at = 0;
		for (size_t r = 0; r < q.part_slot.size(); r++) {
			const uint64_t parent = map_parent(g.m, q.part_ids[at]);
			for (uint32_t j = 0; j < q.part_len[r]; j++, at++) add_partial(parent, q.part_bands[at], q.part_ids[at]);
		}
	} else {
		// unrefine requests pending from before (or more local cells than
		// the device runs encode): the same walk on the host
		const std::vector<uint8_t> b = download(band, n, g.s_comp);
		const auto& ids = slot_ids_host(g);
		std::vector<uint8_t> rb;
		std::vector<uint64_t> ri;
		uint64_t run_parent = error_cell;
		auto flush = [&] {
			if (ri.empty()) return;
			if (ri.size() == 8) decide(rb.data(), ri.data(), 8);
			else
				for (size_t i = 0; i < ri.size(); i++) add_partial(run_parent, rb[i], ri[i]);
			rb.clear();
			ri.clear();
		};
		for (size_t s = 0; s < n; s++) {
			const int lvl = map_level(g.m, ids[s]);
			if (b[s] == 2 && lvl < g.R) {
				g.refine_requests.insert(ids[s]);  // 2434-2520: a local leaf below the maximum level
				nref++;
			}
			if (lvl == 0) {
				flush();
				run_parent = error_cell;
				continue;
			}
			const uint64_t p = map_parent(g.m, ids[s]);
			if (p != run_parent) {
				flush();
				run_parent = p;
			}
			rb.push_back(b[s]);
			ri.push_back(ids[s]);
		}
		flush();
	}
	DX_LAP("chk.2_requests");
	for (auto& kv : partial) decide(kv.second.first.data(), kv.second.second.data(), kv.second.first.size());
	DX_LAP("chk.3_partial_families");
	if (counts) {
		counts[0] = nref;
		counts[1] = nkeep;
		counts[2] = nunref;
	}
}

// adapt_grid (tests/advection/adapter.hpp:232-309): stop_refining, the new
// children carry their parent's payload (density = parent's, 247), a merged
// parent's density = its removed children's / 8 (260-290), velocities and
// lengths of every local cell reset (294-305), then a halo of all seven
// fields (transfer_all_data, 2d.cpp:400-407).  out: created, removed cells.
void advection_adapt(Grid& g, const int fids[7], uint64_t out[2]) {
	DX_REQUIRE(g.initialized, "not initialized");
	const double* cf[7];
	adv_fields(g, fids, cf);
	DX_LAPS(g.s_comp);
	// velocities and lengths are reset for every local cell below
	// (adapter.hpp:292-309): the rebuild need not carry them (the removed
	// store still gets them, packed before the rebuild)
	{
		std::deque<Restore<bool>> carry;  // (back to false also when no rebuild ran: nothing changed)
		for (int k = 1; k < 7; k++)
			if (fids[k] != fids[0]) carry.emplace_back(field(g, fids[k]).no_carry, true);
		// the density keeps this call's rule (a child its parent's value, a
		// parent the mean below) whatever mode it follows the mesh with
		Restore<int> mode(field(g, fids[0]).follow_mode, DCCRGX_FOLLOW_OFF);
		stop_refining_impl(g);
	}
	DX_LAP("adapt.1_stop_refining");
	hipStream_t s = g.s_comp;
	double* f[7];
	for (int k = 0; k < 7; k++) {
		f[k] = (double*)field(g, fids[k]).data.p;
		field_written(field(g, fids[k]));
	}
	// merged parents (adapter.hpp:260-290): the removed children grouped by
	// parent on the device, each parent's mean of its eight children
	k_adv_merge_parents(g.m, g.dm(), g.n_local, g.removed_ids, f[0], (const double*)field(g, fids[0]).removed.p, s,
	                    g.merged_dev.p, g.n_merged);
	DX_LAP("adapt.2_parents");
	// the reset pass also leaves the next time step's block minima
	g.dt_part.reserve(kDtPartials);
	const size_t nb = k_adv_reset(g.m, g.slot_ids.p, g.n_local, g.start, g.l0, stretched_view(g), f, s, g.dt_part.p);
	dt_cache_set(g, fids, nb);
	HIP_CHECK(hipStreamSynchronize(s));
	DX_LAP("adapt.3_reset");
	// transfer_all_data: every field of the seven in this halo
	{
		std::deque<Restore<bool>> flags;
		for (int k = 0; k < 7; k++) flags.emplace_back(field(g, fids[k]).transfer, true);
		halo_start(g);
		halo_wait(g);
	}
	DX_LAP("adapt.4_halo");
	if (out) {
		out[0] = g.new_cells.size();
		out[1] = g.removed_ids.size();
	}
}

}  // namespace dccrgx
