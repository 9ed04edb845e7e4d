// One electrostatic particle-in-cell cycle through the drop-in facade, every
// stage on the GPU: particles_deposit (cloud in cell, per volume) makes the
// charge density, the Poisson solver the potential of rhs = -(rho - mean rho),
// gradient with scale -1 the field E = -grad phi, particles_gather reads E
// back into the records, particles_accelerate adds (dt q) E to the velocities
// and particles_step pushes with them.  8 x 8 x 8 level-0 cells of length 1,
// fully periodic, one refinement level with the 2 x 2 x 2 block in the middle
// refined, neighborhood length 1.  Records of 10 doubles: position, velocity,
// charge q, E.  On this small grid the mean of rho is subtracted on the host.
//
// usage: mpiexec -n P pic_electrostatic
//   prints on rank 0 "pic cycles <n> records <before> <after> lost <l>" and
//   PASSED when its invariants hold (exit status 1 otherwise):
//   * E from phi = x^2 is -2 x on every cell whose two x-neighbors lie inside
//     the grid (the stencil is exact for a quadratic, across level jumps too);
//   * no record is lost and the record count is conserved.
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

int main(int argc, char* argv[])
{
	MPI_Init(&argc, &argv);
	constexpr int K = 10, CYCLES = 3;
	constexpr double LX = 8, DT = 0.05;
	int rank = 0;
	uint64_t before = 0, after = 0, lost = 0, bad_field = 0, checked = 0;
	{
		Grid grid;
		grid.set_initial_length({8, 8, 8}).set_neighborhood_length(1).set_maximum_refinement_level(1);
		grid.set_periodic(true, true, true).set_host_staging(false);
		grid.initialize(MPI_COMM_WORLD);
		rank = grid.get_rank();

		// the 2 x 2 x 2 block in the middle, refined
		const std::vector<uint64_t> level0 = grid.get_slot_ids();
		for (size_t i = 0; i < grid.get_number_of_local_slots(); i++) {
			const uint64_t id = level0[i];
			const auto c = grid.geometry.get_center(id);
			bool in = true;
			for (size_t d = 0; d < 3; d++) in = in && c[d] > 3 && c[d] < 5;
			if (in) grid.refine_completely(id);
		}
		grid.stop_refining();

		auto particles = grid.add_variable_field<double>("particles", true);
		const auto rho = grid.add_field<double>("rho", false);
		const auto rhs = grid.add_field<double>("rhs", false);
		const auto phi = grid.add_field<double>("phi", true);
		const auto ex = grid.add_field<double>("Ex", true);
		const auto ey = grid.add_field<double>("Ey", true);
		const auto ez = grid.add_field<double>("Ez", true);
		const std::array<const dccrg::Device_Field<double>*, 3> E{{&ex, &ey, &ez}};

		const size_t n = grid.get_number_of_local_slots();
		const std::vector<uint64_t> slots = grid.get_slot_ids();
		const std::vector<uint64_t> cells(slots.begin(), slots.begin() + ptrdiff_t(n));
		std::vector<double> volume(n);
		std::vector<std::array<double, 3>> center(n), lo(n), hi(n);
		for (size_t i = 0; i < n; i++) {
			const auto L = grid.geometry.get_length(cells[i]);
			center[i] = grid.geometry.get_center(cells[i]);
			lo[i] = grid.geometry.get_min(cells[i]);
			hi[i] = grid.geometry.get_max(cells[i]);
			volume[i] = L[0] * L[1] * L[2];
		}

		// invariant 1: E = -grad(x^2) = -2 x
		{
			std::vector<double> v(n);
			for (size_t i = 0; i < n; i++) v[i] = center[i][0] * center[i][0];
			phi.set(v);
			grid.update_copies_of_remote_neighbors();
			grid.gradient(phi, E, -1.0);
			const auto got = ex.get(n);
			for (size_t i = 0; i < n; i++) {
				if (lo[i][0] <= 0 || hi[i][0] >= LX) continue;  // a neighbor across the wrap is no sample of x^2
				checked++;
				if (!(std::fabs(got[i] + 2 * center[i][0]) <= 1e-12)) bad_field++;
			}
		}

		// two records in every local cell: a slow drift, charges 1 + 0.1 cos(2 pi x / Lx)
		std::vector<std::vector<double>> lists(n);
		for (size_t i = 0; i < n; i++) {
			Stream rnd{cells[i]};
			for (int k = 0; k < 2; k++) {
				double x[3];
				for (size_t d = 0; d < 3; d++) x[d] = lo[i][d] + (hi[i][d] - lo[i][d]) * rnd.next();
				for (size_t d = 0; d < 3; d++) lists[i].push_back(x[d]);
				for (size_t d = 0; d < 3; d++) lists[i].push_back(0.2 * (rnd.next() - 0.5));
				lists[i].push_back(1 + 0.1 * std::cos(2 * M_PI * x[0] / LX));
				for (size_t d = 0; d < 3; d++) lists[i].push_back(0);
			}
			before += 2;
		}
		particles.upload(lists);
		phi.set(std::vector<double>(n, 0.0));
		grid.poisson_cache(rhs, phi, cells);

		for (int cycle = 0; cycle < CYCLES; cycle++) {
			grid.update_copies_of_remote_neighbors();  // the neighbors' records
			grid.particles_deposit(particles, rho, K, 6, 1, true);
			// rhs = -(rho - mean rho): a periodic system is solvable for a zero-mean source
			std::vector<double> r = rho.get(n);
			double sums[2] = {0, 0}, all[2] = {0, 0};
			for (size_t i = 0; i < n; i++) {
				sums[0] += r[i] * volume[i];
				sums[1] += volume[i];
			}
			MPI_Allreduce(sums, all, 2, MPI_DOUBLE, MPI_SUM, MPI_COMM_WORLD);
			const double mean = all[0] / all[1];
			for (size_t i = 0; i < n; i++) r[i] = -(r[i] - mean);
			rhs.set(r);
			grid.poisson_solve(40, 0, 1e-10, 2, 10);
			grid.update_copies_of_remote_neighbors();  // phi
			grid.gradient(phi, E, -1.0);
			grid.update_copies_of_remote_neighbors();  // E
			grid.particles_gather(particles, {ex, ey, ez}, 7, K, 1);
			grid.particles_accelerate(particles, 7, K, DT, 6);
			grid.update_copies_of_remote_neighbors();  // the accelerated records
			lost += grid.particles_step(particles, K, nullptr, DT)[4];
		}

		const size_t n_end = grid.get_number_of_local_slots();
		for (const auto& l : particles.download(n_end)) after += l.size() / K;
	}
	uint64_t mine[5] = {before, after, lost, bad_field, checked}, all[5] = {0, 0, 0, 0, 0};
	MPI_Reduce(mine, all, 5, MPI_UINT64_T, MPI_SUM, 0, MPI_COMM_WORLD);
	int status = 0;
	if (rank == 0) {
		std::printf("pic cycles %d records %llu %llu lost %llu\n", CYCLES, (unsigned long long)all[0],
		            (unsigned long long)all[1], (unsigned long long)all[2]);
		std::printf("field of x^2 checked on %llu cells, %llu off\n", (unsigned long long)all[4],
		            (unsigned long long)all[3]);
		if (all[0] == all[1] && all[2] == 0 && all[3] == 0 && all[4] > 0) {
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
