// The diagnostics of a particle-in-cell cycle on the device: the
// electromagnetic cycle of pic_electromagnetic.cpp (8 x 8 x 8 level-0 cells of
// length 1, fully periodic, two records of 13 doubles in every cell: position,
// velocity, charge q, E, B; unit mass, c = eps_0 = 1), with every scalar of a
// cycle from one field_reduce_device and one particles_reduce_device call, both
// collective.  Their 19 doubles land in the first slots of a scratch cell
// field and are copied to the host once per cycle; no field and no record
// leaves the device for them.
//   field_reduce_device, by volume:  sum Ex^2 V .. sum Bz^2 V (the field energy
//     is half their sum), max |div B|, sum rho V (the deposited charge);
//   particles_reduce_device, weight -1:  the record count, the total charge
//     sum q, the momenta sum v_d, sum v_d^2 (the kinetic energy is half their
//     sum), max |v_d|, whose product with dt against the cell length decides
//     whether particles_step can lose a record.
//
// usage: mpiexec -n P pic_diagnostics
//   prints on rank 0 per cycle, as hex floats,
//     "cycle <i> field energy <e> kinetic energy <k> charge <q> momentum <x> <y> <z>"
//     "cycle <i> max |div B| <d> max |v| <x> <y> <z> records <n> max |v| dt <c>"
//   then "pic_diagnostics cycles <n> records <before> <after> lost <l>",
//   "sums checked <k>, <b> off; extrema checked <k>, <b> off" and PASSED when
//   every check holds in every cycle (exit status 1 otherwise).  The checks
//   are the one stated exception to "nothing is downloaded": the host way of
//   pic_electromagnetic.cpp (download every field and record list, loop, and
//   MPI_Allreduce) computes the same scalars, and
//   * the extrema are bitwise equal, the record count is equal;
//   * a sum of k terms is within gamma(k - 1) sum |t_i| of the host's,
//     gamma(m) = m u / (1 - m u), u = 2^-53, which holds for any order of
//     the additions; the host's own sum is kept in long double and adds
//     k 2^-63 sum |t_i|;
//   * the total charge of the records equals the deposited sum rho V within
//     the two sums' bounds and the deposit's own, pic_magnetized.cpp's
//     ((N + 2) 2^-52 + 64 2^-52 X / l_min + 4 2^-52) sum |q| (nothing leaves a
//     periodic grid);
//   * max |v_d| dt stays under the cell length and no record is lost.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// the host way: a sum of terms in long double with the sum of their magnitudes and their number
struct HostSum {
	long double sum = 0, mag = 0, k = 0;
	void add(const double t) {
		sum += t;
		mag += std::fabs(t);
		k += 1;
	}
};

static bool same_bits(const double a, const double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char* argv[])
{
	MPI_Init(&argc, &argv);
	constexpr int K = 13, Q = 6, E0 = 7, B0 = 10, CYCLES = 4, NF = 8, NP = 11;
	constexpr double LX = 8, DT = 0.05, MASS = 1.0, BZ = 1.0, C2 = 1.0, EPS0 = 1.0, CELL = 1.0;
	constexpr double U = 1.1102230246251565e-16, EPS = 2 * U;
	int rank = 0;
	uint64_t before = 0, after = 0, lost = 0;
	int sums_checked = 0, sums_off = 0, ext_checked = 0, ext_off = 0, other_off = 0;
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
		const auto diag = grid.add_field<double>("diagnostics", false);  // its first NF + NP slots hold the results
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

		using FT = Grid::Field_Term;
		using RT = Grid::Record_Term;
		const std::vector<FT> field_terms = {
		    {DCCRGX_REDUCE_SUM, &ex, &ex}, {DCCRGX_REDUCE_SUM, &ey, &ey},      {DCCRGX_REDUCE_SUM, &ez, &ez},
		    {DCCRGX_REDUCE_SUM, &bx, &bx}, {DCCRGX_REDUCE_SUM, &by, &by},      {DCCRGX_REDUCE_SUM, &bz, &bz},
		    {DCCRGX_REDUCE_MAX_ABS, &div, nullptr}, {DCCRGX_REDUCE_SUM, &rho, nullptr}};
		const std::vector<RT> record_terms = {
		    {DCCRGX_REDUCE_SUM, -1, -1}, {DCCRGX_REDUCE_SUM, Q, -1},     {DCCRGX_REDUCE_SUM, 3, -1},
		    {DCCRGX_REDUCE_SUM, 4, -1},  {DCCRGX_REDUCE_SUM, 5, -1},     {DCCRGX_REDUCE_SUM, 3, 3},
		    {DCCRGX_REDUCE_SUM, 4, 4},   {DCCRGX_REDUCE_SUM, 5, 5},      {DCCRGX_REDUCE_MAX_ABS, 3, -1},
		    {DCCRGX_REDUCE_MAX_ABS, 4, -1}, {DCCRGX_REDUCE_MAX_ABS, 5, -1}};
		if (field_terms.size() != NF || record_terms.size() != NP || n < NF + NP) return 2;

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

			// the diagnostics of the cycle: two calls, one copy of 19 doubles
			grid.divergence(B, div);
			double* const d_out = diag.data();
			grid.field_reduce_device(field_terms, d_out, true, DCCRGX_REGION_ALL, true);
			grid.particles_reduce_device(particles, record_terms, d_out + NF, K, -1, true);
			const std::vector<double> r = diag.get(NF + NP);
			const double* const fr = r.data();
			const double* const pr = r.data() + NF;
			const double field_energy = 0.5 * (((fr[0] + fr[1]) + fr[2]) + ((fr[3] + fr[4]) + fr[5]));
			const double kinetic = 0.5 * MASS * ((pr[5] + pr[6]) + pr[7]);
			const double cfl = std::max(std::max(pr[8], pr[9]), pr[10]) * DT;

			// the host way: download and loop
			HostSum hf[NF], hp[NP];
			double hmax[4] = {0, 0, 0, 0};  // |div B|, |v_d|
			{
				const std::vector<double> f[6] = {ex.get(n), ey.get(n), ez.get(n), bx.get(n), by.get(n), bz.get(n)};
				const std::vector<double> dv = div.get(n), rh = rho.get(n);
				const double V = (CELL * CELL) * CELL;
				for (size_t i = 0; i < n; i++) {
					for (int j = 0; j < 6; j++) hf[j].add((f[j][i] * f[j][i]) * V);
					hmax[0] = std::max(hmax[0], std::fabs(dv[i]));
					hf[7].add((rh[i] * 1.0) * V);
				}
				for (const auto& l : particles.download(n)) {
					for (size_t p = 0; p + K <= l.size(); p += K) {
						const double* rec = l.data() + p;
						hp[0].add(1.0);
						hp[1].add(rec[Q]);
						for (int d = 0; d < 3; d++) {
							hp[2 + d].add(rec[3 + d]);
							hp[5 + d].add(rec[3 + d] * rec[3 + d]);
							hmax[1 + d] = std::max(hmax[1 + d], std::fabs(rec[3 + d]));
						}
					}
				}
			}
			long double mine[3 * (NF + NP)], all[3 * (NF + NP)];
			for (int j = 0; j < NF + NP; j++) {
				const HostSum& h = j < NF ? hf[j] : hp[j - NF];
				mine[3 * j] = h.sum;
				mine[3 * j + 1] = h.mag;
				mine[3 * j + 2] = h.k;
			}
			MPI_Allreduce(mine, all, 3 * (NF + NP), MPI_LONG_DOUBLE, MPI_SUM, MPI_COMM_WORLD);
			double gmax[4];
			MPI_Allreduce(hmax, gmax, 4, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
			auto bound = [&](const int j) {  // of sum j against the host's
				const long double k = all[3 * j + 2], S = all[3 * j + 1];
				const long double m = k > 1 ? k - 1 : 0;
				return m * U / (1 - m * U) * S + k * 1.0842021724855044e-19L * S;  // gamma(k - 1) S + k 2^-63 S
			};
			for (int j = 0; j < NF + NP; j++) {
				const bool is_sum = j < NF ? j != 6 : j - NF < 8;
				if (!is_sum) continue;
				sums_checked++;
				if (!(std::fabs((double)(all[3 * j] - (long double)r[size_t(j)])) <= (double)bound(j))) sums_off++;
			}
			const double ext_dev[4] = {fr[6], pr[8], pr[9], pr[10]};
			for (int j = 0; j < 4; j++) {
				ext_checked++;
				if (!same_bits(ext_dev[j], gmax[j])) ext_off++;
			}
			// the record count; the records' charge against the deposited one
			const uint64_t held_all = uint64_t(all[3 * NF + 2]);
			if (pr[0] != double(held_all) || held_all != total_before) other_off++;
			const long double sum_q = all[3 * (NF + 1) + 1];
			const long double deposit = (((long double)held_all + 2) * EPS + 64 * EPS * LX / CELL + 4 * EPS) * sum_q;
			if (!(std::fabs(pr[1] - fr[7]) <= (double)(bound(NF + 1) + bound(7) + deposit))) other_off++;
			if (!(cfl < CELL)) other_off++;

			grid.update_copies_of_remote_neighbors();  // the kicked records
			lost += grid.particles_step(particles, K, nullptr, DT)[4];

			if (rank == 0) {
				std::printf("cycle %d field energy %a kinetic energy %a charge %a momentum %a %a %a\n", cycle, field_energy,
				            kinetic, pr[1], pr[2], pr[3], pr[4]);
				std::printf("cycle %d max |div B| %a max |v| %a %a %a records %.0f max |v| dt %a\n", cycle, fr[6], pr[8],
				            pr[9], pr[10], pr[0], cfl);
			}
		}

		const size_t n_end = grid.get_number_of_local_slots();
		for (const auto& l : particles.download(n_end)) after += l.size() / K;
	}
	uint64_t mine[3] = {before, after, lost}, all[3] = {0, 0, 0};
	MPI_Reduce(mine, all, 3, MPI_UINT64_T, MPI_SUM, 0, MPI_COMM_WORLD);
	int status = 0;
	if (rank == 0) {
		// (every scalar was reduced over all processes: every rank holds the same tallies)
		std::printf("pic_diagnostics cycles %d records %llu %llu lost %llu\n", CYCLES, (unsigned long long)all[0],
		            (unsigned long long)all[1], (unsigned long long)all[2]);
		std::printf("sums checked %d, %d off; extrema checked %d, %d off\n", sums_checked, sums_off, ext_checked, ext_off);
		if (all[0] == all[1] && all[2] == 0 && sums_off == 0 && ext_off == 0 && other_off == 0) {
			std::printf("PASSED\n");
		} else {
			std::printf("FAILED (%d other checks off)\n", other_off);
			status = 1;
		}
	}
	MPI_Bcast(&status, 1, MPI_INT, 0, MPI_COMM_WORLD);
	MPI_Finalize();
	return status;
}
