// A full electromagnetic particle-in-cell cycle through the drop-in facade, the
// fields never leaving the GPU: particles_deposit_moments makes the charge and
// the current density (cloud in cell, per volume), curl with accumulate is
// Faraday's law B <- B - dt curl E and Ampere's law E <- E + c^2 dt curl B,
// field_axpy carries the source term E <- E - (dt / eps_0) J, one
// particles_gather reads E and B back into the records, particles_boris kicks
// and particles_step pushes.  8 x 8 x 8 level-0 cells of length 1, fully
// periodic, unrefined, neighborhood length 1; c = eps_0 = 1.  Records of 13
// doubles: position, velocity, charge q, E, B.  Initially E = 0 and
// B = B_0 z + curl A for a seeded random A, made with curl itself.  Only
// diagnostics run on the host.
//
// usage: mpiexec -n P pic_electromagnetic
//   prints on rank 0 per cycle "cycle <i> max |div B| <v> bound <b> max |div E|
//   <w>", then "pic_electromagnetic cycles <n> records <before> <after> lost
//   <l>", "div B within its bound in <k> of <n> cycles" and PASSED when its
//   invariants hold in every cycle (exit status 1 otherwise):
//   * no record is lost and the record count is kept;
//   * max_c |div B| stays under a rounding bound.  On this grid every centre
//     distance is 1, so a = b = 1/2 exactly and D_d(F) = fl(fl(v+ - vc) / 2 +
//     fl(vc - v-) / 2) acts along d only: the operators commute and the
//     divergence of the exact curl of any fp64 fields is 0, as is that of the
//     uniform B_0.  What is left of div B is rounding, counted in units
//     u = 2^-53 with X the largest |input| of a curl call and B the largest
//     |B| so far.  A derivative is off by 3 u X (two differences of at most
//     2 X halved, one sum); r = p - q by 6 u X and its own u 2 X; t = scale r
//     by |scale| 8 u X and its own u |scale| 2 X; B + t by its own u B: an
//     update leaves an error of at most e = 10 u |scale| X + u B in a cell,
//     and the divergence of an error field is at most 3 max e (three
//     derivatives of at most max e each).  Evaluating the divergence of B
//     itself costs three derivatives (9 u B) and two sums (u 2 B, u 3 B):
//     14 u B.  After the initial curl of A and n Faraday steps of scale -dt
//       max |div B| <= 3 (10 u max|A| + u B) + 3 n (10 u dt max|E| + u B) + 14 u B
//     with max|E| and B the largest values of any cycle so far.
//   max |div E| is printed next to it: E has the source J, whose divergence is
//   not small, so the same measurement can tell the difference.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

#include "mpi.h"

#include "dccrg.hpp"

struct particle_cell {  // the reference's cell (tests/particles/cell.hpp), unused on the device path
	uint64_t number_of_particles = 0;
	std::tuple<void*, int, MPI_Datatype> get_mpi_datatype() {
		return std::make_tuple((void*)&number_of_particles, 1, MPI_UINT64_T);
	}
};

using Grid = dccrg::Dccrg<particle_cell, dccrg::Cartesian_Geometry>;
using Field3 = std::array<const dccrg::Device_Field<double>*, 3>;

// a seeded stream of doubles in [0, 1) per cell (splitmix64), the same at every process count
struct Stream {
	uint64_t s;
	double next() {
		uint64_t z = (s += 0x9E3779B97F4A7C15ull);
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		z ^= z >> 31;
		return double(z >> 11) * (1.0 / 9007199254740992.0);
	}
};

// the largest |value| of the local cells of the given fields, over all processes
static double global_max(const std::vector<const dccrg::Device_Field<double>*>& fields, const size_t n) {
	double m = 0, all = 0;
	for (const auto* f : fields)
		for (const double v : f->get(n)) m = std::max(m, std::fabs(v));
	MPI_Allreduce(&m, &all, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
	return all;
}

int main(int argc, char* argv[])
{
	MPI_Init(&argc, &argv);
	constexpr int K = 13, Q = 6, E0 = 7, B0 = 10, CYCLES = 4;
	constexpr double LX = 8, DT = 0.05, MASS = 1.0, BZ = 1.0, C2 = 1.0, EPS0 = 1.0, U = 1.1102230246251565e-16;
	int rank = 0;
	uint64_t before = 0, after = 0, lost = 0, count_off = 0;
	int div_ok = 0;
	{
		Grid grid;
		grid.set_initial_length({8, 8, 8}).set_neighborhood_length(1).set_maximum_refinement_level(0);
		grid.set_periodic(true, true, true).set_host_staging(false);
		grid.initialize(MPI_COMM_WORLD);
		rank = grid.get_rank();

		auto particles = grid.add_variable_field<double>("particles", true);
		const auto rho = grid.add_field<double>("rho", false);
		const auto jx = grid.add_field<double>("Jx", false);
		const auto jy = grid.add_field<double>("Jy", false);
		const auto jz = grid.add_field<double>("Jz", false);
		const auto ax = grid.add_field<double>("Ax", true);
		const auto ay = grid.add_field<double>("Ay", true);
		const auto az = grid.add_field<double>("Az", true);
		const auto ex = grid.add_field<double>("Ex", true);
		const auto ey = grid.add_field<double>("Ey", true);
		const auto ez = grid.add_field<double>("Ez", true);
		const auto bx = grid.add_field<double>("Bx", true);
		const auto by = grid.add_field<double>("By", true);
		const auto bz = grid.add_field<double>("Bz", true);
		const auto div = grid.add_field<double>("div", false);
		const Field3 A{{&ax, &ay, &az}}, E{{&ex, &ey, &ez}}, B{{&bx, &by, &bz}}, J{{&jx, &jy, &jz}};

		const size_t n = grid.get_number_of_local_slots();
		const std::vector<uint64_t> slots = grid.get_slot_ids();
		const std::vector<uint64_t> cells(slots.begin(), slots.begin() + ptrdiff_t(n));

		// E = 0, B = B_0 z + curl A
		for (int d = 0; d < 3; d++) {
			std::vector<double> a(n);
			for (size_t i = 0; i < n; i++) {
				Stream rnd{cells[i] * 3 + uint64_t(d) + 1000003};
				a[i] = 0.1 * (rnd.next() - 0.5);
			}
			A[size_t(d)]->set(a);
			E[size_t(d)]->set(std::vector<double>(n, 0.0));
			B[size_t(d)]->set(std::vector<double>(n, d == 2 ? BZ : 0.0));
		}
		grid.update_copies_of_remote_neighbors();  // A
		grid.curl(A, B, 1.0, true);
		const double a_max = global_max({&ax, &ay, &az}, n);
		double e_max = 0, b_max = global_max({&bx, &by, &bz}, n);

		// two records in every local cell: a slow drift, charges 1 + 0.1 cos(2 pi x / Lx)
		std::vector<std::vector<double>> lists(n);
		for (size_t i = 0; i < n; i++) {
			Stream rnd{cells[i]};
			const auto lo = grid.geometry.get_min(cells[i]), hi = grid.geometry.get_max(cells[i]);
			for (int k = 0; k < 2; k++) {
				double x[3];
				for (size_t d = 0; d < 3; d++) x[d] = lo[d] + (hi[d] - lo[d]) * rnd.next();
				for (size_t d = 0; d < 3; d++) lists[i].push_back(x[d]);
				for (size_t d = 0; d < 3; d++) lists[i].push_back(0.2 * (rnd.next() - 0.5));
				lists[i].push_back(1 + 0.1 * std::cos(2 * M_PI * x[0] / LX));
				for (size_t d = 0; d < 6; d++) lists[i].push_back(0);
			}
			before += 2;
		}
		particles.upload(lists);
		uint64_t total_before = 0;
		MPI_Allreduce(&before, &total_before, 1, MPI_UINT64_T, MPI_SUM, MPI_COMM_WORLD);

		for (int cycle = 0; cycle < CYCLES; cycle++) {
			grid.update_copies_of_remote_neighbors();  // the neighbors' records; E for Faraday's law
			grid.particles_deposit_moments(particles, {rho, jx, jy, jz}, {{{-1, -1}}, {{3, -1}}, {{4, -1}}, {{5, -1}}}, K,
			                               Q, 1, true);
			grid.curl(E, B, -DT, true);                // B <- B - dt curl E
			grid.update_copies_of_remote_neighbors();  // B
			grid.curl(B, E, C2 * DT, true);            // E <- E + c^2 dt curl B
			for (size_t d = 0; d < 3; d++) grid.field_axpy(*E[d], -DT / EPS0, *J[d]);  // E <- E - (dt / eps_0) J
			grid.update_copies_of_remote_neighbors();  // E and B
			grid.particles_gather(particles, {ex, ey, ez, bx, by, bz}, E0, K, 1);
			grid.particles_boris(particles, E0, B0, K, DT / (2 * MASS), Q);
			grid.update_copies_of_remote_neighbors();  // the kicked records
			lost += grid.particles_step(particles, K, nullptr, DT)[4];

			// diagnostics: the record count, div B against its bound, div E
			uint64_t held = 0, held_all = 0;
			for (const auto& l : particles.download(grid.get_number_of_local_slots())) held += l.size() / K;
			MPI_Allreduce(&held, &held_all, 1, MPI_UINT64_T, MPI_SUM, MPI_COMM_WORLD);
			if (held_all != total_before) count_off++;
			grid.divergence(B, div);
			const double div_b = global_max({&div}, n);
			grid.divergence(E, div);
			const double div_e = global_max({&div}, n);
			b_max = std::max(b_max, global_max({&bx, &by, &bz}, n));
			// (the E a Faraday step read is the one the previous cycle left)
			const double bound = 3 * (10 * U * a_max + U * b_max) + 3 * (cycle + 1) * (10 * U * DT * e_max + U * b_max) +
			                     14 * U * b_max;
			e_max = std::max(e_max, global_max({&ex, &ey, &ez}, n));
			if (div_b <= bound) div_ok++;
			if (rank == 0)
				std::printf("cycle %d max |div B| %.3e bound %.3e max |div E| %.3e\n", cycle, div_b, bound, div_e);
		}

		const size_t n_end = grid.get_number_of_local_slots();
		for (const auto& l : particles.download(n_end)) after += l.size() / K;
	}
	uint64_t mine[3] = {before, after, lost}, all[3] = {0, 0, 0};
	MPI_Reduce(mine, all, 3, MPI_UINT64_T, MPI_SUM, 0, MPI_COMM_WORLD);
	int status = 0;
	if (rank == 0) {
		// (the count and the maxima were reduced over all processes: every rank holds the same tallies)
		std::printf("pic_electromagnetic cycles %d records %llu %llu lost %llu\n", CYCLES, (unsigned long long)all[0],
		            (unsigned long long)all[1], (unsigned long long)all[2]);
		std::printf("div B within its bound in %d of %d cycles\n", div_ok, CYCLES);
		if (all[0] == all[1] && all[2] == 0 && count_off == 0 && div_ok == CYCLES) {
			std::printf("PASSED\n");
		} else {
			std::printf("FAILED\n");
			status = 1;
		}
	}
	MPI_Bcast(&status, 1, MPI_INT, 0, MPI_COMM_WORLD);
	MPI_Finalize();
	return status;
}
