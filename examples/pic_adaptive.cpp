// pic_electrostatic.cpp's cycle on a mesh that adapts while it runs, every
// stage on the GPU: the particles and the cell fields follow the mesh through
// stop_refining on the device.  8 x 8 x 8 level-0 cells of length 1, fully
// periodic, one refinement level, neighborhood length 1.  One record in every
// cell and a blob of eight more in each of the eight cells in the middle, which
// drifts along x; records of 10 doubles: position, velocity, charge q, E.
//
// Every second cycle the leaves whose deposited charge density is above
// 3 x the mean are refined and those below 1.5 x the mean unrefined, so the
// refined patch travels with the blob.  Followers:
//   particles   particles_follow_mesh
//   rho         DCCRGX_FOLLOW_MEAN    (charge density, deposit per volume)
//   qcell       DCCRGX_FOLLOW_SUM     (charge per cell, plain deposit)
//   phi         DCCRGX_FOLLOW_LINEAR  (the solver's starting guess)
//
// usage: mpiexec -n P pic_adaptive
//   prints on rank 0 per cycle the solver's iteration counts from the followed
//   phi and from zero, side by side, then
//   "pic adaptive cycles <n> records <before> <after> lost <l> created <c>
//   removed <r> off <k>" and PASSED when its invariants hold (exit status 1
//   otherwise):
//   * across every stop_refining the integral of rho (field_reduce by
//     volume) and the plain sum of qcell are unchanged within gamma(k) S:
//     both quantities are sums of non-negative terms, so S is the sum itself;
//     k counts the cells, one product with the volume and the sixteen rounded
//     operations of a restriction, gamma(m) = m u / (1 - m u), u = 2^-53;
//   * the collective record count is the same before and after it, and no
//     record is lost in an adaptation or a step.
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
using FT = Grid::Field_Term;

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

static double gamma_bound(const double m) {
	const double u = 1.0 / 9007199254740992.0;
	return m * u / (1 - m * u);
}

int main(int argc, char* argv[])
{
	MPI_Init(&argc, &argv);
	constexpr int K = 10, CYCLES = 8;
	constexpr double DT = 0.5, DRIFT = 0.5, KICK = 0.002;
	int rank = 0;
	uint64_t before = 0, after = 0, lost = 0, created = 0, removed = 0, off = 0;
	{
		Grid grid;
		grid.set_initial_length({8, 8, 8}).set_neighborhood_length(1).set_maximum_refinement_level(1);
		grid.set_periodic(true, true, true).set_host_staging(false);
		grid.initialize(MPI_COMM_WORLD);
		rank = grid.get_rank();

		auto particles = grid.add_variable_field<double>("particles", true);
		const auto rho = grid.add_field<double>("rho", false);
		const auto qcell = grid.add_field<double>("qcell", false);
		const auto rhs = grid.add_field<double>("rhs", false);
		const auto phi = grid.add_field<double>("phi", true);
		const auto phi0 = grid.add_field<double>("phi0", false);
		const auto ex = grid.add_field<double>("Ex", true);
		const auto ey = grid.add_field<double>("Ey", true);
		const auto ez = grid.add_field<double>("Ez", true);
		const std::array<const dccrg::Device_Field<double>*, 3> E{{&ex, &ey, &ez}};
		grid.particles_follow_mesh(particles, K);
		grid.field_follow_mesh(rho, DCCRGX_FOLLOW_MEAN);
		grid.field_follow_mesh(qcell, DCCRGX_FOLLOW_SUM);
		grid.field_follow_mesh(phi, DCCRGX_FOLLOW_LINEAR);

		size_t n = grid.get_number_of_local_slots();
		std::vector<uint64_t> slots = grid.get_slot_ids();
		std::vector<uint64_t> cells(slots.begin(), slots.begin() + ptrdiff_t(n));

		// one record in every cell, eight more in each of the eight cells in
		// the middle; the blob drifts along x
		std::vector<std::vector<double>> lists(n);
		for (size_t i = 0; i < n; i++) {
			Stream rnd{cells[i]};
			const auto lo = grid.geometry.get_min(cells[i]), hi = grid.geometry.get_max(cells[i]);
			const auto c = grid.geometry.get_center(cells[i]);
			bool blob = true;
			for (size_t d = 0; d < 3; d++) blob = blob && c[d] > 3 && c[d] < 5;
			const int count = blob ? 9 : 1;
			for (int k = 0; k < count; k++) {
				for (size_t d = 0; d < 3; d++) lists[i].push_back(lo[d] + (hi[d] - lo[d]) * rnd.next());
				lists[i].push_back(k ? DRIFT : 0.0);
				for (size_t d = 1; d < 3; d++) lists[i].push_back(0.05 * (rnd.next() - 0.5));
				lists[i].push_back(1.0);
				for (size_t d = 0; d < 3; d++) lists[i].push_back(0);
			}
			before += uint64_t(count);
		}
		particles.upload(lists);
		phi.set(std::vector<double>(n, 0.0));

		const std::vector<Grid::Record_Term> count_term{{DCCRGX_REDUCE_SUM, -1, -1}};
		for (int cycle = 0; cycle < CYCLES; cycle++) {
			grid.update_copies_of_remote_neighbors();  // the neighbors' records
			grid.particles_deposit(particles, rho, K, 6, 1, true);
			grid.particles_deposit(particles, qcell, K, 6, 1, false);
			// rhs = -(rho - mean rho): a periodic system is solvable for a zero-mean source
			const auto tot = grid.field_reduce({FT{DCCRGX_REDUCE_SUM, &rho, nullptr}, FT{DCCRGX_REDUCE_SUM, nullptr, nullptr}},
			                                   true, DCCRGX_REGION_ALL, true);
			const double mean = tot[0] / tot[1];
			std::vector<double> r = rho.get(n);
			for (size_t i = 0; i < n; i++) r[i] = -(r[i] - mean);
			rhs.set(r);
			// the same system from zero, for the comparison only, then from the phi that followed the mesh
			phi0.set(std::vector<double>(n, 0.0));
			grid.poisson_cache(rhs, phi0, cells);
			const auto cold = grid.poisson_solve(200, 0, 1e-8, 2, 10);
			grid.poisson_cache(rhs, phi, cells);
			const auto warm = grid.poisson_solve(200, 0, 1e-8, 2, 10);
			if (rank == 0)
				std::printf("cycle %d iterations followed %u zero %u\n", cycle, unsigned(warm.iterations),
				            unsigned(cold.iterations));
			grid.update_copies_of_remote_neighbors();  // phi
			grid.gradient(phi, E, -1.0);
			grid.update_copies_of_remote_neighbors();  // E
			grid.particles_gather(particles, {ex, ey, ez}, 7, K, 1);
			grid.particles_accelerate(particles, 7, K, KICK, 6);
			grid.update_copies_of_remote_neighbors();  // the accelerated records
			lost += grid.particles_step(particles, K, nullptr, DT)[4];

			if (cycle % 2 == 0) continue;
			// adapt: refine where the charge is, merge where it has left
			const std::vector<double> dens = rho.get(n);
			for (size_t i = 0; i < n; i++) {
				const int lvl = grid.get_refinement_level(cells[i]);
				if (lvl == 0 && dens[i] > 3 * mean) grid.refine_completely(cells[i]);
				if (lvl == 1 && dens[i] < 1.5 * mean) grid.unrefine_completely(cells[i]);
			}
			grid.update_copies_of_remote_neighbors();  // phi's remote copies, for the slopes
			const std::vector<FT> sums{FT{DCCRGX_REDUCE_SUM, nullptr, nullptr}};
			const double k0 = grid.field_reduce(sums, false, DCCRGX_REGION_ALL, true)[0];
			const double i0 = grid.field_reduce({FT{DCCRGX_REDUCE_SUM, &rho, nullptr}}, true, DCCRGX_REGION_ALL, true)[0];
			const double q0 = grid.field_reduce({FT{DCCRGX_REDUCE_SUM, &qcell, nullptr}}, false, DCCRGX_REGION_ALL, true)[0];
			const double c0 = grid.particles_reduce(particles, count_term, K, -1, true)[0];
			created += grid.stop_refining().size();
			removed += grid.get_removed_cells().size();
			lost += grid.particles_adapt_stats(particles)[2];
			n = grid.get_number_of_local_slots();
			slots = grid.get_slot_ids();
			cells.assign(slots.begin(), slots.begin() + ptrdiff_t(n));
			const double k1 = grid.field_reduce(sums, false, DCCRGX_REGION_ALL, true)[0];
			const double i1 = grid.field_reduce({FT{DCCRGX_REDUCE_SUM, &rho, nullptr}}, true, DCCRGX_REGION_ALL, true)[0];
			const double q1 = grid.field_reduce({FT{DCCRGX_REDUCE_SUM, &qcell, nullptr}}, false, DCCRGX_REGION_ALL, true)[0];
			const double c1 = grid.particles_reduce(particles, count_term, K, -1, true)[0];
			const double bi = gamma_bound(k0 + 17) * std::fabs(i0) + gamma_bound(k1 + 17) * std::fabs(i1);
			const double bq = gamma_bound(k0 + 17) * std::fabs(q0) + gamma_bound(k1 + 17) * std::fabs(q1);
			if (rank == 0) {
				std::printf("adapt %d cells %.0f -> %.0f integral of rho %.17g -> %.17g sum of qcell %.17g -> %.17g\n", cycle,
				            k0, k1, i0, i1, q0, q1);
				if (!(std::fabs(i1 - i0) <= bi)) off++;
				if (!(std::fabs(q1 - q0) <= bq)) off++;
				if (c0 != c1) off++;
			}
		}

		for (const auto& l : particles.download(n)) after += l.size() / K;
	}
	uint64_t mine[6] = {before, after, lost, created, removed, off}, all[6] = {0, 0, 0, 0, 0, 0};
	MPI_Reduce(mine, all, 6, MPI_UINT64_T, MPI_SUM, 0, MPI_COMM_WORLD);
	int status = 0;
	if (rank == 0) {
		std::printf("pic adaptive cycles %d records %llu %llu lost %llu created %llu removed %llu off %llu\n", CYCLES,
		            (unsigned long long)all[0], (unsigned long long)all[1], (unsigned long long)all[2],
		            (unsigned long long)all[3], (unsigned long long)all[4], (unsigned long long)all[5]);
		if (all[0] == all[1] && all[2] == 0 && all[5] == 0) {
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
