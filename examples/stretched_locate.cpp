// Point location under a Stretched_Cartesian_Geometry through the drop-in
// facade: the geometry's unevenly spaced coordinates reach the library
// (dccrgx_set_stretched_geometry), so get_existing_cell(coordinate) is
// answered on the device.  Every level-0 boundary, every boundary of the
// finest cells (formed as c0 + k * li), each of those one step of the double
// grid below and above, and points outside the grid are located both ways:
// on the device, and on the host through geometry.get_real_coordinate,
// geometry.get_indices and get_existing_cell(indices).  4 x 3 x 2 cells,
// periodic in x and z, some cells refined twice.
//
// usage: mpiexec -n 1 stretched_locate
//   prints "located <points> inside <n> mismatches <n>"; exits non-zero on a mismatch
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

#include "mpi.h"

#include "dccrg.hpp"
#include "dccrg_stretched_cartesian_geometry.hpp"

struct Cell {
	double v = 0;
	std::tuple<void*, int, MPI_Datatype> get_mpi_datatype() const {
		return std::make_tuple((void*)&v, 1, MPI_DOUBLE);
	}
};

using Grid = dccrg::Dccrg<Cell, dccrg::Stretched_Cartesian_Geometry>;

int main(int argc, char* argv[]) {
	MPI_Init(&argc, &argv);
	uint64_t points = 0, inside = 0, mismatches = 0;
	{
		const int R = 2;
		dccrg::Stretched_Cartesian_Geometry::Parameters geom;
		geom.coordinates[0] = {0.0, 0.5, 1.5, 3.0, 5.0};
		geom.coordinates[1] = {0.1, 0.4, 1.1, 1.2};
		geom.coordinates[2] = {-0.6, -0.3, 0.4};
		Grid grid;
		grid.set_initial_length({{4, 3, 2}}).set_neighborhood_length(1).set_maximum_refinement_level(R);
		grid.set_periodic(true, false, true);
		grid.set_geometry(geom);
		grid.initialize(MPI_COMM_WORLD);
		for (const uint64_t c : {uint64_t(2), uint64_t(11), uint64_t(24)})
			if (grid.is_local(c)) grid.refine_completely(c);
		grid.stop_refining();
		for (const uint64_t c : {uint64_t(27), uint64_t(36)})  // children of cell 2
			if (grid.is_local(c)) grid.refine_completely(c);
		grid.stop_refining();

		// per dimension the telling values; the other two coordinates sit
		// inside the grid at a different place for every point
		std::vector<std::array<double, 3>> xs;
		const auto& c = grid.geometry.get().coordinates;
		const double inf = INFINITY;
		for (size_t d = 0; d < 3; d++) {
			std::vector<double> v;
			for (size_t i = 0; i < c[d].size(); i++) {
				v.push_back(c[d][i]);
				if (i + 1 == c[d].size()) break;
				const double li = (c[d][i + 1] - c[d][i]) / double(1 << R);
				for (int k = 0; k <= (1 << R); k++) v.push_back(c[d][i] + k * li);
			}
			const size_t n = v.size();
			for (size_t i = 0; i < n; i++) {
				v.push_back(std::nextafter(v[i], -inf));
				v.push_back(std::nextafter(v[i], inf));
			}
			const double len = c[d].back() - c[d].front();
			for (const double f : {1.0, 2.5}) {
				v.push_back(c[d].front() - f * len);
				v.push_back(c[d].back() + f * len);
			}
			for (size_t i = 0; i < v.size(); i++) {
				std::array<double, 3> x;
				for (size_t e = 0; e < 3; e++) {
					const double t = double((7 * i + 3 * e + 1) % 23) / 23.0;
					x[e] = c[e].front() + (c[e].back() - c[e].front()) * t;
				}
				x[d] = v[i];
				xs.push_back(x);
			}
		}
		for (const auto& x : xs) {
			const uint64_t device = grid.get_existing_cell(x);
			const auto r = grid.geometry.get_real_coordinate(x);
			const auto ind = grid.geometry.get_indices(r);
			uint64_t host = dccrg::error_cell;
			if (ind[0] != dccrg::error_index && ind[1] != dccrg::error_index && ind[2] != dccrg::error_index)
				host = grid.get_existing_cell(ind, 0, R);
			points++;
			if (host != dccrg::error_cell) inside++;
			if (device != host) {
				if (mismatches++ < 10)
					std::fprintf(stderr, "(%.17g, %.17g, %.17g): device %llu, host %llu\n", x[0], x[1], x[2],
					             (unsigned long long)device, (unsigned long long)host);
			}
		}
	}
	std::printf("located %llu inside %llu mismatches %llu\n", (unsigned long long)points, (unsigned long long)inside,
	            (unsigned long long)mismatches);
	MPI_Finalize();
	return mismatches ? 1 : 0;
}
