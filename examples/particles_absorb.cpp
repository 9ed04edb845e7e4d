// An absorbing body inside the domain: the sink that belongs to
// particles_create's source.  16 x 4 x 4 level-0 cells of length 1, periodic
// in every dimension; records of 7 doubles: position, velocity, weight.
//   body:   the cells 8 <= ix < 10, 1 <= iy < 3 (all iz) hold 1.0 in a mask
//           field, the others 0.0;
//   load:   4 records in every cell, weight 0.25 * density[c] with
//           density = 1 + 0.25 (ix mod 4), velocity normal with drift 0.3 in x
//           and thermal speed 0.1 (particles_create);
//   cycle:  the halo (the neighbors' lists as the last remove left them),
//           particles_step with dt = 0.5, then particles_remove: the mask
//           absorbs, a test drops the records faster than drift + 3 thermal
//           speeds in x, and a (-1, -1) tally adds every removed weight to the
//           cell's entry of the field `collected`: the body's surface charge.
// Every cycle prints the record count and the pool's charge
// (particles_reduce), the collected charge (field_reduce) and the four counts
// of the remove.  The weights are dyadic, so every partial sum is exact and
// the program asserts in every cycle
//   pool charge + collected charge == loaded charge,
// and, from an NGP count deposit times the mask, that no record is left in a
// masked cell.  Which records leave does not depend on the number of
// processes, so the count lines are the same at every process count.
//
// usage: mpiexec -n P particles_absorb
//   prints on rank 0 "loaded records <n> charge <q>", per cycle
//   "cycle <i> records <n> charge <q> collected <s> kept <k> mask <m> test <t>
//   chance <c>" (charges as hex floats), then PASSED when the assertions held
//   in all 20 cycles and the body absorbed something (exit status 1 otherwise).
#include <array>
#include <cstdint>
#include <cstdio>
#include <limits>
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

int main(int argc, char* argv[])
{
	MPI_Init(&argc, &argv);
	constexpr int K = 7, W = 6, CYCLES = 20;
	constexpr uint64_t NX = 16, NY = 4, LOADED = 4 * 16 * 4 * 4;
	constexpr double DT = 0.5, DRIFT = 0.3, THERMAL = 0.1;
	int rank = 0, status = 0;
	{
		Grid grid;
		grid.set_initial_length({NX, NY, 4}).set_neighborhood_length(1).set_maximum_refinement_level(0);
		grid.set_periodic(true, true, true).set_host_staging(false);
		grid.initialize(MPI_COMM_WORLD);
		rank = grid.get_rank();

		auto particles = grid.add_variable_field<double>("particles", true);
		const auto density = grid.add_field<double>("density", false);
		const auto mask = grid.add_field<double>("mask", false);
		const auto collected = grid.add_field<double>("collected", false);
		const auto occupancy = grid.add_field<double>("occupancy", false);
		const size_t n = grid.get_number_of_local_slots();
		const std::vector<uint64_t> slots = grid.get_slot_ids();
		std::vector<double> dens(n), body(n), zero(n, 0.0);
		for (size_t i = 0; i < n; i++) {
			const uint64_t ix = (slots[i] - 1) % NX, iy = ((slots[i] - 1) / NX) % NY;
			dens[i] = 1 + 0.25 * double(ix % 4);
			body[i] = ix >= 8 && ix < 10 && iy >= 1 && iy < 3 ? 1.0 : 0.0;
		}
		density.set(dens);
		mask.set(body);
		collected.set(zero);

		using CS = Grid::Create_Spec;
		const std::vector<CS> recipe = {{3, CS::NORMAL, DRIFT, THERMAL, nullptr, nullptr},
		                                {4, CS::NORMAL, 0.0, THERMAL, nullptr, nullptr},
		                                {5, CS::NORMAL, 0.0, THERMAL, nullptr, nullptr},
		                                {W, CS::CONSTANT, 0.25, 0.0, &density, nullptr}};
		const std::vector<Grid::Record_Term> pool_terms = {{DCCRGX_REDUCE_SUM, -1, -1}, {DCCRGX_REDUCE_SUM, W, -1}};
		const std::vector<Grid::Field_Term> field_terms = {{DCCRGX_REDUCE_SUM, &collected, nullptr},
		                                                   {DCCRGX_REDUCE_SUM, &mask, &occupancy}};
		const std::vector<Grid::Remove_Test> tests = {
		    {3, Grid::Remove_Test::KEEP, -std::numeric_limits<double>::infinity(), DRIFT + 3 * THERMAL}};
		const std::vector<Grid::Remove_Tally> tally = {{-1, -1, &collected}};
		auto total = [](uint64_t mine) {
			uint64_t all = 0;
			MPI_Allreduce(&mine, &all, 1, MPI_UINT64_T, MPI_SUM, MPI_COMM_WORLD);
			return all;
		};

		const uint64_t loaded = total(grid.particles_create(particles, K, 4.0, nullptr, false, recipe, 1));
		std::vector<double> r = grid.particles_reduce(particles, pool_terms, K, -1, true);
		const double charge0 = r[1];
		if (rank == 0) std::printf("loaded records %.0f charge %a\n", r[0], r[1]);
		bool ok = loaded == LOADED && r[0] == double(LOADED);
		uint64_t held = loaded, absorbed = 0;
		for (int cycle = 1; cycle <= CYCLES; cycle++) {
			grid.update_copies_of_remote_neighbors();  // the neighbors' records
			const uint64_t lost = total(grid.particles_step(particles, K, nullptr, DT)[4]);
			std::array<uint64_t, 4> st =
			    grid.particles_remove(particles, K, tests, &mask, 0.0, nullptr, 0, false, W, tally);
			for (auto& x : st) x = total(x);
			r = grid.particles_reduce(particles, pool_terms, K, -1, true);
			grid.particles_deposit(particles, occupancy, K, -1, 0, false);
			const std::vector<double> f = grid.field_reduce(field_terms, false, DCCRGX_REGION_ALL, true);
			if (rank == 0)
				std::printf("cycle %d records %.0f charge %a collected %a kept %llu mask %llu test %llu chance %llu\n",
				            cycle, r[0], r[1], f[0], (unsigned long long)st[0], (unsigned long long)st[1],
				            (unsigned long long)st[2], (unsigned long long)st[3]);
			ok = ok && lost == 0 && st[0] + st[1] + st[2] + st[3] == held && r[0] == double(st[0]);
			ok = ok && r[1] + f[0] == charge0;  // exact: dyadic weights
			ok = ok && f[1] == 0.0;             // no record is left in a masked cell
			held = st[0];
			absorbed += st[1];
		}
		ok = ok && absorbed > 0 && held > 0;
		if (rank == 0) std::printf(ok ? "PASSED\n" : "FAILED\n");
		status = ok ? 0 : 1;
	}
	MPI_Bcast(&status, 1, MPI_INT, 0, MPI_COMM_WORLD);
	MPI_Finalize();
	return status;
}
