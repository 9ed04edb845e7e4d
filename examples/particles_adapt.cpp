// Particles on an adaptive mesh through the drop-in facade: each cell's list
// of coordinates is a device variable field (3 doubles per particle) that
// follows the mesh (particles_follow_mesh).  Where user code of the reference
// would hand a refined parent's particles to its children from
// refined_cell_data and the removed children's to their parent from
// unrefined_cell_data, stop_refining here does it on the device.  A 4 x 4 x 4
// periodic grid, neighborhood length 1, one refinement level: every fifth
// cell is refined, a step, every family is merged again, a step.
//
// usage: mpiexec -n P particles_adapt
//   prints on rank 0: "particles <before> <after> outside <n> lost <n>"
#include <array>
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
	int rank = 0;
	uint64_t before = 0, after = 0, outside = 0, lost = 0;
	{
		Grid grid;
		grid.set_initial_length({4, 4, 4}).set_neighborhood_length(1).set_maximum_refinement_level(1);
		grid.set_periodic(true, true, true).set_host_staging(false);
		grid.initialize(MPI_COMM_WORLD);
		rank = grid.get_rank();
		auto particles = grid.add_variable_field<double>("particles", true);
		grid.particles_follow_mesh(particles, 3);

		// initial condition: 1..5 particles inside every local cell
		size_t n = grid.get_number_of_local_slots();
		std::vector<uint64_t> ids = grid.get_slot_ids();
		std::vector<std::vector<double>> lists(n);
		for (size_t i = 0; i < n; i++) {
			Stream rnd{ids[i]};
			const auto lo = grid.geometry.get_min(ids[i]), hi = grid.geometry.get_max(ids[i]);
			const unsigned count = 1 + unsigned(5 * rnd.next());
			for (unsigned k = 0; k < count; k++)
				for (size_t d = 0; d < 3; d++) lists[i].push_back(lo[d] + (hi[d] - lo[d]) * rnd.next());
			before += count;
		}
		particles.upload(lists);

		const std::array<double, 3> velocity{{0.1, 0.05, 0}};
		auto step = [&]() {
			grid.update_copies_of_remote_neighbors();
			lost += grid.particles_step(particles, 3, &velocity, 1.0)[4];
		};

		for (size_t i = 0; i < n; i++)
			if (ids[i] % 5 == 1) grid.refine_completely(ids[i]);
		grid.stop_refining();
		lost += grid.particles_adapt_stats(particles)[2];
		step();

		n = grid.get_number_of_local_slots();
		ids = grid.get_slot_ids();
		for (size_t i = 0; i < n; i++)
			if (grid.get_refinement_level(ids[i]) == 1) grid.unrefine_completely(ids[i]);
		grid.stop_refining();
		lost += grid.particles_adapt_stats(particles)[2];
		step();

		n = grid.get_number_of_local_slots();
		ids = grid.get_slot_ids();
		lists = particles.download(n);
		for (size_t i = 0; i < n; i++) {
			const auto lo = grid.geometry.get_min(ids[i]), hi = grid.geometry.get_max(ids[i]);
			after += lists[i].size() / 3;
			for (size_t k = 0; k + 2 < lists[i].size(); k += 3) {
				bool in = true;
				for (size_t d = 0; d < 3; d++) in = in && lists[i][k + d] >= lo[d] && lists[i][k + d] <= hi[d];
				const std::array<double, 3> x{{lists[i][k], lists[i][k + 1], lists[i][k + 2]}};
				if (!in || grid.get_existing_cell(x) != ids[i]) outside++;
			}
		}
	}
	uint64_t mine[4] = {before, after, outside, lost}, all[4] = {0, 0, 0, 0};
	MPI_Reduce(mine, all, 4, MPI_UINT64_T, MPI_SUM, 0, MPI_COMM_WORLD);
	if (rank == 0)
		std::printf("particles %llu %llu outside %llu lost %llu\n", (unsigned long long)all[0],
		            (unsigned long long)all[1], (unsigned long long)all[2], (unsigned long long)all[3]);
	MPI_Finalize();
	return 0;
}
