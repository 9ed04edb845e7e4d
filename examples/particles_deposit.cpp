// The two halves of a particle-in-cell transfer through the drop-in facade,
// with the particle lists and the cell fields on the GPU: particles_deposit
// sums every particle's charge into the cells its cloud overlaps (cloud in
// cell over leaves), particles_gather interpolates a cell field back to every
// particle with the same weights.  4 x 4 x 4 cells, fully periodic,
// neighborhood length 1, records of 5 doubles (position, charge q, gathered
// value).  All data are dyadic (positions on eighths of a cell, q on 2^-10,
// the cell field on sixteenths), so every sum is exact: the deposited total
// equals the particles' total charge to the bit, and the printed line is the
// same at every process count.
//
// usage: mpiexec -n P particles_deposit
//   prints on rank 0: "deposit <records> <sum of out> <sum of gathered>"
//   exit status 1 when the deposited total is not the total charge
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
	constexpr int K = 5;
	int rank = 0;
	uint64_t records = 0;
	double charge = 0, deposited = 0, gathered = 0;
	{
		Grid grid;
		grid.set_initial_length({4, 4, 4}).set_neighborhood_length(1).set_maximum_refinement_level(0);
		grid.set_periodic(true, true, true).set_host_staging(false);
		grid.initialize(MPI_COMM_WORLD);
		rank = grid.get_rank();
		auto particles = grid.add_variable_field<double>("particles", true);
		auto rho = grid.add_field<double>("rho", false);
		auto field = grid.add_field<double>("field", true);

		// 1..5 particles inside every local cell, and the cell field
		const size_t n = grid.get_number_of_local_slots();
		const std::vector<uint64_t> ids = grid.get_slot_ids();
		std::vector<std::vector<double>> lists(n);
		std::vector<double> values(n);
		for (size_t i = 0; i < n; i++) {
			Stream rnd{ids[i]};
			const auto lo = grid.geometry.get_min(ids[i]), hi = grid.geometry.get_max(ids[i]);
			const unsigned count = 1 + unsigned(5 * rnd.next());
			for (unsigned k = 0; k < count; k++) {
				for (size_t d = 0; d < 3; d++) {
					const double eighths = double(unsigned(8 * rnd.next()));
					lists[i].push_back(lo[d] + (hi[d] - lo[d]) * eighths / 8);
				}
				const double q = double(unsigned(1024 * rnd.next())) / 1024;
				lists[i].push_back(q);
				lists[i].push_back(0);
				charge += q;
			}
			records += count;
			values[i] = double(ids[i] % 16) / 16;
		}
		particles.upload(lists);
		field.set(values);

		// the neighbors' particles and field values, then the two transfers
		grid.update_copies_of_remote_neighbors();
		grid.particles_deposit(particles, rho, K, 3, 1, false);
		grid.particles_gather(particles, {field}, 4, K, 1);

		for (const double v : rho.get(n)) deposited += v;
		lists = particles.download(n);
		for (size_t i = 0; i < n; i++)
			for (size_t k = 0; k + K <= lists[i].size(); k += K) gathered += lists[i][k + 4];
	}
	uint64_t all_records = 0;
	double mine[3] = {charge, deposited, gathered}, all[3] = {0, 0, 0};
	MPI_Reduce(&records, &all_records, 1, MPI_UINT64_T, MPI_SUM, 0, MPI_COMM_WORLD);
	MPI_Reduce(mine, all, 3, MPI_DOUBLE, MPI_SUM, 0, MPI_COMM_WORLD);
	int status = 0;
	if (rank == 0) {
		std::printf("deposit %llu %.17g %.17g\n", (unsigned long long)all_records, all[1], all[2]);
		if (all[1] != all[0]) {
			std::printf("the particles' charge is %.17g\n", all[0]);
			status = 1;
		}
	}
	MPI_Bcast(&status, 1, MPI_INT, 0, MPI_COMM_WORLD);
	MPI_Finalize();
	return status;
}
