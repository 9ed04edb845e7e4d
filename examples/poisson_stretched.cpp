// Poisson's equation on unevenly spaced cells through the drop-in facade:
// the scenario of the reference's tests/poisson/poisson1d_stretched.cpp with
// the facade's device members.  For n = 8, 16, ... 1024 two grids of n x 1 x 1
// periodic cells cover [0, 2 pi] in x: one with a
// Stretched_Cartesian_Geometry whose cells shrink toward the places where the
// solution's gradient is largest (every cell of four equal ones is divided
// 1:3 again and again), one with evenly spaced cells.  On both the right-hand
// side is sin(center), the solver is Poisson_Solve(10, 0, 1e-5, 2, 10), and
// the solution is compared with -sin(center) in the 2-norm.  The stretched
// grid's factors come from its own cell lengths (dccrgx_poisson_cache follows
// the active stretched geometry).  Cells are dealt to the processes by
// id % comm_size, as the reference program does with pins.
//
// usage: mpiexec -n P poisson_stretched [largest n]
//   prints on rank 0, per size:
//   "cells <n> stretched <norm> <iterations> <residual> even <norm> <iterations> <residual>"
//   exits non-zero when the stretched norm is above the even one at 8 cells or
//   the even norm grows with n (the reference program's two conditions)
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <tuple>
#include <vector>

#include "mpi.h"

#include "dccrg.hpp"
#include "dccrg_stretched_cartesian_geometry.hpp"

struct Cell {  // unused on the device path
	double v = 0;
	std::tuple<void*, int, MPI_Datatype> get_mpi_datatype() const {
		return std::make_tuple((void*)&v, 1, MPI_DOUBLE);
	}
};

struct Outcome {
	double norm = 0;
	dccrg::Poisson_Result solve;
};

// n + 1 boundaries of n cells on [0, 2 pi]: the narrow part of every division
// lies toward 0 in the first and third quarter, toward 2 pi in the others
static std::vector<double> divided_boundaries(const uint64_t n) {
	std::vector<double> x{0, M_PI / 2, M_PI, 3 * M_PI / 2, 2 * M_PI};
	const double ratio = 3;
	while (x.size() < n) {
		std::vector<double> finer{x[0]};
		for (size_t i = 1; i < x.size(); i++) {
			const double lo = x[i - 1], hi = x[i], middle = (hi + lo) / 2;
			const bool toward_start = middle < M_PI / 2 || (middle >= M_PI && middle < 3 * M_PI / 2);
			finer.push_back(toward_start ? hi - (hi - lo) * ratio / (ratio + 1) : lo + (hi - lo) * ratio / (ratio + 1));
			finer.push_back(hi);
		}
		x.swap(finer);
	}
	return x;
}

// deal the cells out, set rhs = sin(center) and solution = 0 on the device,
// solve, and return the 2-norm of solution + sin(center) over all processes
template <class Grid> static Outcome solve_on(Grid& grid) {
	const int size = grid.get_comm_size();
	for (const uint64_t cell : grid.get_cells()) grid.pin(cell, int(cell % uint64_t(size)));
	grid.balance_load(false);
	grid.unpin_all_cells();

	const auto rhs = grid.template add_field<double>("rhs", false);
	const auto sol = grid.template add_field<double>("solution", true);
	const auto slots = grid.get_slot_ids();
	const size_t nl = grid.get_number_of_local_slots();
	const std::vector<uint64_t> cells(slots.begin(), slots.begin() + ptrdiff_t(nl));
	std::vector<double> center(nl), r(nl), zero(nl, 0.0);
	for (size_t s = 0; s < nl; s++) {
		center[s] = grid.geometry.get_center(cells[s])[0];
		r[s] = std::sin(center[s]);
	}
	rhs.set(r);
	sol.set(zero);

	Outcome out;
	grid.poisson_cache(rhs, sol, cells);
	out.solve = grid.poisson_solve(10, 0, 1e-5, 2, 10);
	const auto x = sol.get(nl);
	double local = 0, global = 0;
	for (size_t s = 0; s < nl; s++) local += std::pow(std::fabs(x[s] - (-std::sin(center[s]))), 2.0);
	MPI_Allreduce(&local, &global, 1, MPI_DOUBLE, MPI_SUM, MPI_COMM_WORLD);
	out.norm = std::pow(global, 1.0 / 2.0);
	return out;
}

int main(int argc, char* argv[]) {
	MPI_Init(&argc, &argv);
	int rank = 0;
	MPI_Comm_rank(MPI_COMM_WORLD, &rank);
	const uint64_t largest = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1024;
	int failed = 0;
	double even_before = std::numeric_limits<double>::max();
	for (uint64_t n = 8; n <= largest && !failed; n *= 2) {
		Outcome stretched, even;
		{
			dccrg::Dccrg<Cell, dccrg::Stretched_Cartesian_Geometry> grid;
			grid.set_initial_length({{n, 1, 1}}).set_neighborhood_length(0).set_maximum_refinement_level(0);
			grid.set_periodic(true, true, true).set_host_staging(false);
			dccrg::Stretched_Cartesian_Geometry::Parameters geom;
			geom.coordinates[0] = divided_boundaries(n);
			geom.coordinates[1] = {0, 1};
			geom.coordinates[2] = {0, 1};
			grid.set_geometry(geom);
			grid.initialize(MPI_COMM_WORLD);
			stretched = solve_on(grid);
		}
		{
			dccrg::Dccrg<Cell, dccrg::Cartesian_Geometry> grid;
			grid.set_initial_length({{n, 1, 1}}).set_neighborhood_length(0).set_maximum_refinement_level(0);
			grid.set_periodic(true, true, true).set_host_staging(false);
			grid.initialize(MPI_COMM_WORLD);
			dccrg::Cartesian_Geometry_Parameters geom;
			geom.level_0_cell_length = {{2 * M_PI / double(n), 1, 1}};
			grid.set_geometry(geom);
			even = solve_on(grid);
		}
		if (rank == 0) {
			std::printf("cells %llu stretched %.17g %u %.17g even %.17g %u %.17g\n", (unsigned long long)n,
			            stretched.norm, stretched.solve.iterations, stretched.solve.residual, even.norm,
			            even.solve.iterations, even.solve.residual);
			if (n == 8 && stretched.norm > even.norm) {
				std::fprintf(stderr, "the stretched grid's norm is above the even grid's at 8 cells\n");
				failed = 1;
			}
			if (even.norm > even_before) {
				std::fprintf(stderr, "the even grid's norm grew at %llu cells\n", (unsigned long long)n);
				failed = 1;
			}
			even_before = even.norm;
		}
		MPI_Bcast(&failed, 1, MPI_INT, 0, MPI_COMM_WORLD);
	}
	MPI_Finalize();
	return failed;
}
