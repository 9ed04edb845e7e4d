// The Poisson solver's host driver: Poisson_Solve
// (tests/poisson/poisson_solve.hpp:156-1056) over device fields.  The kernels
// and their launchers are in poisson_kernels.hip, the C ABI wrappers in api.hip.
#include <algorithm>
#include <cstdlib>
#include <deque>

#include "dccrgx_grid.hpp"

namespace dccrgx {

// halo update of exactly the given fields (the reference's
// Poisson_Cell::transfer_switch, 92-140)
static void halo_only(Grid& g, const std::vector<int>& fids) {
	if (g.size == 1 || g.peers.empty()) return;
	{
		std::deque<Restore<bool>> flags;  // every field's, back in place once the halo has started
		for (Field& f : g.fields) flags.emplace_back(f.transfer, false);
		for (int f : fids) field(g, f).transfer = true;
		halo_start(g);
	}
	halo_wait(g);
}

static int po_field(Grid& g, const char* name, size_t elem) {
	Field f;
	f.name = name;
	f.elem = elem;
	f.win_len = elem;
	f.transfer = false;
	g.fields.push_back(std::move(f));
	Field& nf = g.fields.back();
	nf.data.alloc(g.n_slots * elem);
	if (nf.data.n) HIP_CHECK(hipMemsetAsync(nf.data.p, 0, nf.data.n, g.s_comp));
	return int(g.fields.size() - 1);
}

static void po_ensure_fields(Grid& g) {
	PoissonState& P = g.po;
	if (P.type >= 0) return;
	P.type = po_field(g, "poisson.type", 4);
	P.p0 = po_field(g, "poisson.p0", 8);
	P.p1 = po_field(g, "poisson.p1", 8);
	P.r0 = po_field(g, "poisson.r0", 8);
	P.r1 = po_field(g, "poisson.r1", 8);
	P.ap0 = po_field(g, "poisson.A_dot_p0", 8);
	P.best = po_field(g, "poisson.best_solution", 8);
	P.sf = po_field(g, "poisson.scaling_factor", 8);
	static const char* fn[6] = {"poisson.f_x_neg", "poisson.f_x_pos", "poisson.f_y_neg",
	                            "poisson.f_y_pos", "poisson.f_z_neg", "poisson.f_z_pos"};
	for (int k = 0; k < 6; k++) P.f[k] = po_field(g, fn[k], 8);
}

static PoArrays po_arrays(Grid& g) {
	PoissonState& P = g.po;
	auto d = [&](int f) { return (double*)field(g, f).data.p; };
	PoArrays a{};
	a.ell = P.ell.p;
	a.fine = P.fine.p;
	a.type = (const int32_t*)field(g, P.type).data.p;
	a.rhs = d(P.rhs);
	a.sol = d(P.sol);
	a.best = d(P.best);
	a.p0 = d(P.p0);
	a.p1 = d(P.p1);
	a.r0 = d(P.r0);
	a.r1 = d(P.r1);
	a.ap0 = d(P.ap0);
	a.sf = d(P.sf);
	for (int k = 0; k < 6; k++) a.f[k] = d(P.f[k]);
	a.ft = P.valid && P.ft.p ? P.ft.p : nullptr;
	return a;
}

// the fields a solve or a cache pass writes: the solution and the solver's own
static void po_written(Grid& g) {
	const PoissonState& P = g.po;
	for (int id : {P.sol, P.type, P.best, P.p0, P.p1, P.r0, P.r1, P.ap0, P.sf})
		if (id >= 0 && size_t(id) < g.fields.size()) field_written(g.fields[size_t(id)]);
	for (int k = 0; k < 6; k++)
		if (P.f[k] >= 0 && size_t(P.f[k]) < g.fields.size()) field_written(g.fields[size_t(P.f[k])]);
}

// cache_system_info 827-971
void poisson_cache(Grid& g, int rhs, int sol, const uint64_t* solve, size_t ns, const uint64_t* skip, size_t nk) {
	DX_REQUIRE(field(g, rhs).elem == 8 && field(g, sol).elem == 8, "rhs and solution must be fp64 fields");
	po_ensure_fields(g);
	PoissonState& P = g.po;
	P.rhs = rhs;
	P.sol = sol;
	po_written(g);
	const FaceStencil F = face_stencil(g);
	hipStream_t s = g.s_comp;
	const size_t nl = g.n_local;
	int32_t* type = (int32_t*)field(g, P.type).data.p;
	// classify: local cells boundary, then skip, then solve (836-878)
	k_fill_i32(type, nl, 1, s);
	for (int pass = 0; pass < 2; pass++) {
		const uint64_t* ids = pass == 0 ? skip : solve;
		const size_t n = pass == 0 ? nk : ns;
		if (!n) continue;
		DBuf<uint64_t> d;
		d.alloc(n);
		h2d(d.p, ids, n * 8, s);
		k_po_classify(type, g.dm(), d.p, n, nl, pass == 0 ? 2 : 0, s);
		HIP_CHECK(hipStreamSynchronize(s));
	}
	halo_only(g, {P.type});  // TYPE (880-881)
	DBuf<int32_t> cls;
	cls.alloc(g.n_slots + 1);
	if (g.n_slots) HIP_CHECK(hipMemcpyAsync(cls.p, type, g.n_slots * 4, hipMemcpyDeviceToDevice, s));
	P.ell.alloc(6 * nl + 6);
	P.fine.alloc(g.face_fine.n);
	const PoArrays a = po_arrays(g);
	// the lengths of the geometry as it is now: Cartesian l0, or the active
	// stretched geometry's coordinates (a remote copy's length comes from its
	// id like a local cell's); the factors stay until the next cache pass
	k_po_cache(F, cls.p, nl, P.ell.p, P.fine.p, type, a, s);
	HIP_CHECK(hipStreamSynchronize(s));
	std::vector<int> geo{P.sf};  // GEOMETRY (969-970)
	for (int k = 0; k < 6; k++) geo.push_back(P.f[k]);
	halo_only(g, geo);
	// the neighbors' factors toward each cell, once per cache pass (phase B
	// reads them coalesced instead of gathering them every iteration;
	// DCCRGX_PO_FT=0 keeps the gathers)
	const char* ftv = std::getenv("DCCRGX_PO_FT");
	if (!(ftv && ftv[0] == '0') && nl) {
		P.ft.alloc(6 * nl);
		k_po_transpose(po_arrays(g), nl, P.ft.p, s);
	} else {
		P.ft.release();
	}
	HIP_CHECK(hipStreamSynchronize(s));
	P.valid = true;
}

// sums of the last phase -> (all ranks) -> scalar control flow
static void po_reduce(Grid& g, int k, unsigned nb, const PoParams& prm, int stage) {
	PoissonState& P = g.po;
	const bool one = g.size == 1;
	k_po_reduce(k, P.part.p, nb, P.red.p, P.st.p, prm, stage, one, g.s_comp);
	if (one) return;
	// MPI_Allreduce SUM (poisson_solve.hpp:349, 486, 684): the ranks' sums
	// all-gathered and added in rank order on every rank (the same result
	// over RCCL and the host exchange)
	comm_require(g, "Poisson solve");
	P.gath.reserve(size_t(g.size) * 2);
	comm_allgather_dev(g, P.red.p, size_t(k) * 8, reinterpret_cast<uint8_t*>(P.gath.p), g.s_comp);
	k_po_scalar(P.gath.p, g.size, k, P.st.p, prm, stage, g.s_comp);
}

static PoScalars po_read_scalars(Grid& g) {
	PoScalars h{};
	d2h_small(&h, g.po.st.p, sizeof(h), g.s_comp);
	return h;
}

// solve 251-522 / solve_failsafe 531-634 after poisson_cache; the host only
// enqueues kernels and polls the device's `done` flag every few iterations.
// Timed (dccrgx_kernel_timing): from the first phase of an iteration to its
// last, the reductions included, the halo excluded.
static PoScalars po_solve(Grid& g, const PoParams& prm, bool failsafe) {
	PoissonState& P = g.po;
	DX_REQUIRE(P.valid, "Poisson system not cached for the current mesh");
	po_written(g);
	hipStream_t s = g.s_comp;
	const size_t n = g.n_local;
	const unsigned nb = xcd_blocks(n);
	if (P.part.n < 2 * size_t(nb)) P.part.alloc(2 * size_t(nb));
	P.red.alloc(2);
	P.st.alloc(1);
	const PoArrays a = po_arrays(g);
	const int poll = 8;
	if (!failsafe) {
		halo_only(g, {P.sol});  // INIT (983-984)
		k_po_phase(PO_PHASE_INIT, a, n, prm, P.st.p, P.part.p, s);
		po_reduce(g, 1, nb, prm, PO_STAGE_INIT);
		for (unsigned it = 0; it < prm.max_it; it++) {
			halo_only(g, {P.p0, P.p1});  // SOLVING (283-284)
			k_time_begin(g);
			k_po_phase(PO_PHASE_A, a, n, prm, P.st.p, P.part.p, s);
			po_reduce(g, 2, nb, prm, PO_STAGE_A);
			k_po_phase(PO_PHASE_B, a, n, prm, P.st.p, P.part.p, s);
			po_reduce(g, 1, nb, prm, PO_STAGE_B);
			k_po_phase(PO_PHASE_C, a, n, prm, P.st.p, P.part.p, s);
			k_time_end(g);
			if ((it + 1) % poll == 0 && po_read_scalars(g).done) break;
		}
		k_po_phase(PO_PHASE_FINISH, a, n, prm, P.st.p, P.part.p, s);
	} else {
		k_po_reduce(1, P.part.p, 0, P.red.p, P.st.p, prm, PO_STAGE_JACOBI_INIT, true, s);
		for (unsigned it = 0; it < prm.max_it; it++) {
			halo_only(g, {P.sol});  // INIT (545, 551)
			k_time_begin(g);
			k_po_phase(PO_PHASE_JACOBI, a, n, prm, P.st.p, P.part.p, s);
			po_reduce(g, 1, nb, prm, PO_STAGE_JACOBI);
			k_po_phase(PO_PHASE_JACOBI_COPY, a, n, prm, P.st.p, P.part.p, s);
			k_time_end(g);
			if ((it + 1) % poll == 0 && po_read_scalars(g).done) break;
		}
	}
	return po_read_scalars(g);
}

void poisson_solve(Grid& g, unsigned max_iterations, unsigned min_iterations, double stop_residual, double p_of_norm,
                   double stop_after_residual_increase, bool failsafe, unsigned* iterations, double* residual) {
	DX_REQUIRE(p_of_norm > 0, "p_of_norm must be > 0");
	// solve() is a do-while (279-506): at least one iteration
	const unsigned max_it = failsafe ? max_iterations : std::max(1u, max_iterations);
	const PoParams prm{max_it, min_iterations, stop_residual, p_of_norm, stop_after_residual_increase};
	const PoScalars st = po_solve(g, prm, failsafe);
	if (iterations) *iterations = st.iteration;
	if (residual) *residual = failsafe ? st.norm : st.residual_min;
}

int poisson_field(Grid& g, const char* name) {
	DX_REQUIRE(g.po.type >= 0, "Poisson system not cached yet");
	const std::string want = std::string("poisson.") + name;
	for (size_t i = 0; i < g.fields.size(); i++)
		if (g.fields[i].name == want) return int(i);
	throw Error(DCCRGX_ENOTFOUND, "no Poisson field " + std::string(name));
}

}  // namespace dccrgx
