// Particles are born on the device: a plasma is loaded and an inflow is kept
// up with particles_create, nothing is built on the host and no record is
// downloaded.  16 x 4 x 4 level-0 cells of length 1, open in x, periodic in y
// and z; records of 7 doubles: position, velocity, weight.
//   load:   4 records in every cell, weight 0.25 * density[c] with
//           density = 1 + 0.25 (ix mod 4), velocity normal with drift 0.3 in x
//           and thermal speed 0.1;
//   cycle:  particles_step with dt = 0.5 (records leave through the open
//           faces, counted lost), then particles_create into the inflow layer
//           ix = 0 alone: count_field is 1 there and 0 elsewhere, count = 0.6
//           with random rounding (the loss through the far face is about
//           4 * 0.3 * 0.5 = 0.6 a face cell and cycle), a new seed per cycle;
//   the record count and the charge of every cycle come from particles_reduce.
// The records a cell receives do not depend on the number of processes, so
// every line is the same at every process count.
//
// usage: mpiexec -n P particles_create
//   prints on rank 0 "loaded records <n> charge <q>", per cycle
//   "cycle <i> records <n> charge <q> created <c> lost <l>" (charges as hex
//   floats), then "band <lo> <hi> records min <m> max <M>" and PASSED when
//   the count stayed inside the band [1024 - 128, 1024 + 128] over the 20
//   cycles, the loaded count is 1024, every cycle's count is the previous one
//   plus created minus lost, and something was created and lost (exit status
//   1 otherwise).
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

int main(int argc, char* argv[])
{
	MPI_Init(&argc, &argv);
	constexpr int K = 7, W = 6, CYCLES = 20;
	constexpr uint64_t NX = 16, LOADED = 4 * 16 * 4 * 4, BAND = 128;
	constexpr double DT = 0.5, DRIFT = 0.3, THERMAL = 0.1, RATE = 0.6;
	int rank = 0, status = 0;
	{
		Grid grid;
		grid.set_initial_length({NX, 4, 4}).set_neighborhood_length(1).set_maximum_refinement_level(0);
		grid.set_periodic(false, true, true).set_host_staging(false);
		grid.initialize(MPI_COMM_WORLD);
		rank = grid.get_rank();

		auto particles = grid.add_variable_field<double>("particles", true);
		const auto density = grid.add_field<double>("density", false);
		const auto inflow = grid.add_field<double>("inflow", false);
		const size_t n = grid.get_number_of_local_slots();
		const std::vector<uint64_t> slots = grid.get_slot_ids();
		std::vector<double> dens(n), in(n);
		for (size_t i = 0; i < n; i++) {
			const uint64_t ix = (slots[i] - 1) % NX;
			dens[i] = 1 + 0.25 * double(ix % 4);
			in[i] = ix == 0 ? 1.0 : 0.0;
		}
		density.set(dens);
		inflow.set(in);

		using CS = Grid::Create_Spec;
		const std::vector<CS> recipe = {{3, CS::NORMAL, DRIFT, THERMAL, nullptr, nullptr},
		                                {4, CS::NORMAL, 0.0, THERMAL, nullptr, nullptr},
		                                {5, CS::NORMAL, 0.0, THERMAL, nullptr, nullptr},
		                                {W, CS::CONSTANT, 0.25, 0.0, &density, nullptr}};
		const std::vector<Grid::Record_Term> terms = {{DCCRGX_REDUCE_SUM, -1, -1}, {DCCRGX_REDUCE_SUM, W, -1}};
		auto total = [](uint64_t mine) {
			uint64_t all = 0;
			MPI_Allreduce(&mine, &all, 1, MPI_UINT64_T, MPI_SUM, MPI_COMM_WORLD);
			return all;
		};

		const uint64_t loaded = total(grid.particles_create(particles, K, 4.0, nullptr, false, recipe, 1));
		std::vector<double> r = grid.particles_reduce(particles, terms, K, -1, true);
		if (rank == 0) std::printf("loaded records %.0f charge %a\n", r[0], r[1]);
		bool ok = loaded == LOADED && r[0] == double(LOADED);
		uint64_t held = loaded, lo = held, hi = held, created_all = 0, lost_all = 0;
		for (int cycle = 1; cycle <= CYCLES; cycle++) {
			grid.update_copies_of_remote_neighbors();  // the neighbors' records
			const uint64_t lost = total(grid.particles_step(particles, K, nullptr, DT)[4]);
			const uint64_t created =
			    total(grid.particles_create(particles, K, RATE, &inflow, true, recipe, 100 + uint64_t(cycle)));
			r = grid.particles_reduce(particles, terms, K, -1, true);
			if (rank == 0)
				std::printf("cycle %d records %.0f charge %a created %llu lost %llu\n", cycle, r[0], r[1],
				            (unsigned long long)created, (unsigned long long)lost);
			ok = ok && r[0] == double(held + created - lost);
			held = held + created - lost;
			lo = held < lo ? held : lo;
			hi = held > hi ? held : hi;
			created_all += created;
			lost_all += lost;
		}
		ok = ok && lo >= LOADED - BAND && hi <= LOADED + BAND && created_all > 0 && lost_all > 0;
		if (rank == 0) {
			std::printf("band %llu %llu records min %llu max %llu\n", (unsigned long long)(LOADED - BAND),
			            (unsigned long long)(LOADED + BAND), (unsigned long long)lo, (unsigned long long)hi);
			std::printf(ok ? "PASSED\n" : "FAILED\n");
		}
		status = ok ? 0 : 1;
	}
	MPI_Bcast(&status, 1, MPI_INT, 0, MPI_COMM_WORLD);
	MPI_Finalize();
	return status;
}
