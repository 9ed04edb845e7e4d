// The particle half of a magnetised particle-in-cell cycle through the drop-in
// facade, every stage on the GPU: particles_deposit_moments makes the charge
// density and the three components of the current density in one walk of the
// records (cloud in cell, per volume), the Poisson solver the potential of
// rhs = -(rho - mean rho), gradient with scale -1 the field E = -grad phi,
// one particles_gather reads E and the cell-centred B back into the records,
// particles_boris kicks the velocities (half the electric kick, the rotation
// about B, the other half) and particles_step pushes with them.  8 x 8 x 8
// level-0 cells of length 1, fully periodic, one refinement level with the
// 2 x 2 x 2 block in the middle refined, neighborhood length 1.  Records of 13
// doubles: position, velocity, charge q, E, B.  B is a uniform B_0 along z
// plus a small perturbation, held in three cell fields.  The current is
// diagnostic here: a field solver for B would take it from these fields.
//
// usage: mpiexec -n P pic_magnetized
//   prints on rank 0 "pic_magnetized cycles <n> records <before> <after> lost
//   <l>", "moment sums checked <k>, <b> off" and PASSED when its invariants
//   hold in every cycle (exit status 1 otherwise):
//   * no record is lost and the record count is kept;
//   * sum_c rho_c V_c = sum_p q_p and sum_c J_c V_c = sum_p q_p v_p per
//     component: nothing leaves a periodic grid.  Each cell's sum is within
//     (m + 2) 2^-52 sum|term| of its exact value, m its number of terms (at
//     most the number of records N), and a record's shares add up to 1 within
//     64 2^-52 X / l_min (X the largest coordinate, l_min the finest cell's
//     length), so the two sides differ by at most
//     ((N + 2) 2^-52 + 64 2^-52 X / l_min + 4 2^-52) sum_p |q_p v_p|
//     with the host's sums kept in long double.
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
	constexpr int K = 13, Q = 6, E0 = 7, B0 = 10, CYCLES = 3;
	constexpr double LX = 8, DT = 0.05, MASS = 1.0, BZ = 1.0, EPS = 2.220446049250313e-16;
	int rank = 0;
	uint64_t before = 0, after = 0, lost = 0, count_off = 0, sums_off = 0, sums_checked = 0;
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
		const auto jx = grid.add_field<double>("Jx", false);
		const auto jy = grid.add_field<double>("Jy", false);
		const auto jz = grid.add_field<double>("Jz", false);
		const auto rhs = grid.add_field<double>("rhs", false);
		const auto phi = grid.add_field<double>("phi", true);
		const auto ex = grid.add_field<double>("Ex", true);
		const auto ey = grid.add_field<double>("Ey", true);
		const auto ez = grid.add_field<double>("Ez", true);
		const auto bx = grid.add_field<double>("Bx", true);
		const auto by = grid.add_field<double>("By", true);
		const auto bz = grid.add_field<double>("Bz", true);
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

		// B = B_0 z + a small divergence-free perturbation
		{
			std::vector<double> x(n), y(n), z(n);
			for (size_t i = 0; i < n; i++) {
				x[i] = 0.05 * std::sin(2 * M_PI * center[i][1] / LX);
				y[i] = 0.05 * std::sin(2 * M_PI * center[i][2] / LX);
				z[i] = BZ + 0.05 * std::sin(2 * M_PI * center[i][0] / LX);
			}
			bx.set(x);
			by.set(y);
			bz.set(z);
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
				for (size_t d = 0; d < 6; d++) lists[i].push_back(0);
			}
			before += 2;
		}
		particles.upload(lists);
		phi.set(std::vector<double>(n, 0.0));
		grid.poisson_cache(rhs, phi, cells);
		uint64_t total_before = 0;
		MPI_Allreduce(&before, &total_before, 1, MPI_UINT64_T, MPI_SUM, MPI_COMM_WORLD);

		for (int cycle = 0; cycle < CYCLES; cycle++) {
			grid.update_copies_of_remote_neighbors();  // the neighbors' records, B in the first cycle
			grid.particles_deposit_moments(particles, {rho, jx, jy, jz}, {{{-1, -1}}, {{3, -1}}, {{4, -1}}, {{5, -1}}}, K,
			                               Q, 1, true);
			// what the records hold against what the cells received
			long double sums[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, all[10];  // 4 of the records, 4 their magnitudes, ...
			uint64_t held = 0;
			for (const auto& l : particles.download(n)) {
				for (size_t p = 0; p + K <= l.size(); p += K) {
					const double q = l[p + Q];
					const double m[4] = {q, q * l[p + 3], q * l[p + 4], q * l[p + 5]};
					for (int j = 0; j < 4; j++) {
						sums[j] += m[j];
						sums[4 + j] += std::fabs(m[j]);
					}
					held++;
				}
			}
			const std::vector<double> r = rho.get(n);
			{
				const std::vector<double> c[4] = {r, jx.get(n), jy.get(n), jz.get(n)};
				long double cellsum[4] = {0, 0, 0, 0};
				for (int j = 0; j < 4; j++)
					for (size_t i = 0; i < n; i++) cellsum[j] += (long double)c[j][i] * volume[i];
				// ... the volume and rho V of the local cells, then the four cell sums
				for (size_t i = 0; i < n; i++) sums[8] += volume[i];
				sums[9] = cellsum[0];
				long double cs[4];
				MPI_Allreduce(cellsum, cs, 4, MPI_LONG_DOUBLE, MPI_SUM, MPI_COMM_WORLD);
				MPI_Allreduce(sums, all, 10, MPI_LONG_DOUBLE, MPI_SUM, MPI_COMM_WORLD);
				uint64_t held_all = 0;
				MPI_Allreduce(&held, &held_all, 1, MPI_UINT64_T, MPI_SUM, MPI_COMM_WORLD);
				if (held_all != total_before) count_off++;
				const long double rel = ((long double)held_all + 2) * EPS + 64 * EPS * LX / 0.5 + 4 * EPS;
				for (int j = 0; j < 4; j++) {
					sums_checked++;
					if (!(std::fabs((double)(cs[j] - all[j])) <= (double)(rel * all[4 + j]))) sums_off++;
				}
			}
			// rhs = -(rho - mean rho): a periodic system is solvable for a zero-mean source
			const double mean = double(all[9] / all[8]);
			std::vector<double> s(n);
			for (size_t i = 0; i < n; i++) s[i] = -(r[i] - mean);
			rhs.set(s);
			grid.poisson_solve(40, 0, 1e-10, 2, 10);
			grid.update_copies_of_remote_neighbors();  // phi
			grid.gradient(phi, E, -1.0);
			grid.update_copies_of_remote_neighbors();  // E
			grid.particles_gather(particles, {ex, ey, ez, bx, by, bz}, E0, K, 1);
			grid.particles_boris(particles, E0, B0, K, DT / (2 * MASS), Q);
			grid.update_copies_of_remote_neighbors();  // the kicked records
			lost += grid.particles_step(particles, K, nullptr, DT)[4];
		}

		const size_t n_end = grid.get_number_of_local_slots();
		for (const auto& l : particles.download(n_end)) after += l.size() / K;
	}
	uint64_t mine[3] = {before, after, lost}, all[3] = {0, 0, 0};
	MPI_Reduce(mine, all, 3, MPI_UINT64_T, MPI_SUM, 0, MPI_COMM_WORLD);
	int status = 0;
	if (rank == 0) {
		// (the sums and the count were reduced over all processes: every rank holds the same tallies)
		std::printf("pic_magnetized cycles %d records %llu %llu lost %llu\n", CYCLES, (unsigned long long)all[0],
		            (unsigned long long)all[1], (unsigned long long)all[2]);
		std::printf("moment sums checked %llu, %llu off\n", (unsigned long long)sums_checked,
		            (unsigned long long)sums_off);
		if (all[0] == all[1] && all[2] == 0 && count_off == 0 && sums_off == 0 && sums_checked == 4 * CYCLES) {
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
