// Cell centers and lengths from the grid's geometry, on the device: one
// thread per slot (remote copies too, the sweeps read them as neighbors)
// takes the level and the indices of the slot's cell from its id and writes
// the fp64 center and / or length into fixed-size fp64 fields.
//
// Cartesian: the expressions of dccrgx_advection_initialize
// (dccrg_cartesian_geometry.hpp:282-362), so filled length fields are bitwise
// l0 * (1 / 2^level), the rows of the sweeps' length table.
// Stretched: Stretched_Cartesian_Geometry::get_length / get_center
// (dccrg_stretched_cartesian_geometry.hpp:298-403) in their operand order.
#include "dccrgx_grid.hpp"

// every product, quotient and sum is separately rounded in the reference
#pragma clang fp contract(off)

namespace dccrgx {

namespace {

struct FillGeo {
	double start[3], l0[3];  // Cartesian
	const double* c;         // stretched: packed coordinates (nullptr: Cartesian)
	uint32_t off[3];
	double* center[3];
	double* length[3];
};

__global__ void geometry_fill_kernel(const MapCtx m, const FillGeo G, const uint64_t* __restrict__ slot_ids,
                                     size_t n_slots) {
	const double nan = __longlong_as_double(0x7ff8000000000000ll);
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n_slots; s += size_t(gridDim.x) * blockDim.x) {
		uint64_t ind[3] = {0, 0, 0};
		const int lvl = map_indices(m, slot_ids[s], ind[0], ind[1], ind[2]);
#pragma unroll
		for (int d = 0; d < 3; d++) {
			double L = nan, c = nan;
			if (lvl >= 0) {
				if (G.c) {
					const uint64_t l0i = uint64_t(1) << m.R;
					const uint64_t i0 = ind[d] / l0i;
					const double c0 = G.c[G.off[d] + i0];
					const double extent = G.c[G.off[d] + i0 + 1] - c0;
					L = extent / double(uint64_t(1) << lvl);
					const double length_of_index = extent / double(l0i);
					const double in_cell = length_of_index * double(ind[d] - i0 * l0i);
					const double low = c0 + in_cell;
					c = low + L / 2;
				} else {
					const double sf = 1.0 / double(uint64_t(1) << lvl);
					L = G.l0[d] * sf;
					const double along = double(ind[d]) * G.l0[d];
					const double rel = along / double(uint64_t(1) << m.R);
					const double low = G.start[d] + rel;
					c = low + L / 2;
				}
			}
			if (G.length[d]) G.length[d][s] = L;
			if (G.center[d]) G.center[d][s] = c;
		}
	}
}

}  // namespace

void geometry_fill(Grid& g, const int center_fields[3], const int length_fields[3]) {
	DX_REQUIRE(g.initialized, "not initialized");
	DX_REQUIRE(g.str.active || g.geo_block.empty(),
	           "the grid holds a stretched geometry block (Cartesian geometry only)");
	FillGeo G{};
	Field* written[6];
	int nw = 0;
	for (int k = 0; k < 6; k++) {
		const int* ids = k < 3 ? center_fields : length_fields;
		const int fid = ids ? ids[k % 3] : -1;
		double** slot = k < 3 ? &G.center[k] : &G.length[k - 3];
		*slot = nullptr;
		if (fid < 0) continue;
		Field& F = fixed_field(g, fid);
		DX_REQUIRE(F.elem == 8, "geometry fields must be fp64");
		DX_REQUIRE(!F.external, "geometry_fill into a field whose device pointer was handed out");
		for (int j = 0; j < nw; j++) DX_REQUIRE(written[j] != &F, "geometry_fill: a field is given twice");
		written[nw++] = &F;
		*slot = reinterpret_cast<double*>(F.data.p);
	}
	if (!nw) return;
	if (g.str.active) {
		G.c = stretched_device(g);
		uint32_t at = 0;
		for (int d = 0; d < 3; d++) {
			G.off[d] = at;
			at += uint32_t(g.str.c[d].size());
		}
	} else {
		for (int d = 0; d < 3; d++) {
			G.start[d] = g.start[d];
			G.l0[d] = g.l0[d];
		}
	}
	for (int j = 0; j < nw; j++) field_written(*written[j]);
	if (!g.n_slots) return;
	geometry_fill_kernel<<<grid_for(g.n_slots, 256), 256, 0, g.s_comp>>>(g.m, G, g.slot_ids.p, g.n_slots);
	HIP_CHECK(hipGetLastError());
}

}  // namespace dccrgx
