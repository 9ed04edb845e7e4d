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
//
// Also here: the stretched geometry's setters, the one definition of its
// grid-file block, and the host-side batch query (dccrgx_geometry_batch).
#include <cmath>
#include <cstring>
#include <limits>
#include <string>

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

// ---- the grid file's Stretched_Cartesian_Geometry block ------------------------
// (write, dccrg_stretched_cartesian_geometry.hpp:652-715): int id 2, 3 x
// uint64 coordinate counts, then each dimension's coordinates as doubles
size_t stretched_block_bytes(const uint8_t* head) {
	int32_t id = 0;
	uint64_t cnt[3];
	std::memcpy(&id, head, 4);
	std::memcpy(cnt, head + 4, 24);
	if (id != kStretchedGeometryId) return 0;
	uint64_t tot = 0;
	for (int d = 0; d < 3; d++) {
		if (cnt[d] < 2 || cnt[d] > (uint64_t(1) << 40)) return 0;  // the reference's set() needs two per dimension
		tot += cnt[d];
	}
	return kStretchedBlockHead + size_t(8 * tot);
}

std::vector<uint8_t> stretched_block(const double* const coords[3], const size_t n[3]) {
	std::vector<uint8_t> b(kStretchedBlockHead + 8 * (n[0] + n[1] + n[2]));
	const int32_t gid = kStretchedGeometryId;
	std::memcpy(b.data(), &gid, 4);
	size_t at = kStretchedBlockHead;
	for (int d = 0; d < 3; d++) {
		const uint64_t cnt = n[d];
		std::memcpy(b.data() + 4 + 8 * d, &cnt, 8);
		std::memcpy(b.data() + at, coords[d], 8 * n[d]);
		at += 8 * n[d];
	}
	return b;
}

void stretched_block_coords(const std::vector<uint8_t>& block, std::vector<double> c[3]) {
	uint64_t cnt[3];
	std::memcpy(cnt, block.data() + 4, 24);
	size_t at = kStretchedBlockHead;
	for (int d = 0; d < 3; d++) {
		c[d].resize(size_t(cnt[d]));
		std::memcpy(c[d].data(), block.data() + at, 8 * c[d].size());
		at += 8 * c[d].size();
	}
}

// ---- the setters ----------------------------------------------------------------
void set_stretched_geometry(Grid& g, const double* const coords[3], const size_t n[3]) {
	// dccrg_stretched_cartesian_geometry.hpp:172-210
	for (int d = 0; d < 3; d++) {
		const std::string dim = " in dimension " + std::to_string(d);
		DX_REQUIRE(coords[d] != nullptr, "null coordinates" + dim);
		DX_REQUIRE(n[d] >= 2, "at least two coordinates are required" + dim);
		DX_REQUIRE(n[d] == g.len[d] + 1, "the number of coordinates" + dim + " must be the grid's length + 1 (" +
		                                     std::to_string(g.len[d] + 1) + ") but is " + std::to_string(n[d]));
		for (size_t i = 0; i < n[d]; i++)
			DX_REQUIRE(std::isfinite(coords[d][i]), "coordinates must be finite" + dim);
		for (size_t i = 0; i + 1 < n[d]; i++)
			DX_REQUIRE(coords[d][i] < coords[d][i + 1], "coordinates must be strictly increasing" + dim);
	}
	g.str.drop();
	g.str.active = true;
	g.geo_block = stretched_block(coords, n);
	for (int d = 0; d < 3; d++) {
		g.str.c[d].assign(coords[d], coords[d] + n[d]);
		// what the consumers that stay Cartesian see, as after load_grid_data:
		// the start and the first level-0 cell's length
		g.start[d] = coords[d][0];
		g.l0[d] = coords[d][1] - coords[d][0];
	}
}

void set_geometry_block(Grid& g, const void* bytes, size_t n) {
	if (n == 0) {
		g.geo_block.clear();
		g.str.drop();
		return;
	}
	DX_REQUIRE(bytes != nullptr && n >= kStretchedBlockHead, "geometry block too short");
	const uint8_t* b = static_cast<const uint8_t*>(bytes);
	DX_REQUIRE(stretched_block_bytes(b) == n, "not a Stretched_Cartesian_Geometry block (id 2, counts, coordinates)");
	g.geo_block.assign(b, b + n);
	g.str.drop();  // a file block only: no device geometry
}

// the host counterpart of geometry_fill_kernel for any ids: NaN for an id that
// is no cell of the grid
void geometry_batch(Grid& g, const uint64_t* ids, size_t n, double* center, double* length) {
	for (int d = 0; d < 3 && g.str.active; d++)
		DX_REQUIRE(g.str.c[d].size() == g.len[d] + 1, "the grid's length changed after set_stretched_geometry");
	MapCtx m;
	map_init(m, g.len, g.R, g.per);
	const double nan = std::numeric_limits<double>::quiet_NaN();
	for (size_t i = 0; i < n; i++) {
		uint64_t ind[3];
		const int lvl = map_indices(m, ids[i], ind[0], ind[1], ind[2]);
		for (int d = 0; d < 3; d++) {
			double L = nan, c = nan;
			if (lvl >= 0 && g.str.active) {  // dccrg_stretched_cartesian_geometry.hpp:298-337, 346-403
				const std::vector<double>& x = g.str.c[d];
				const uint64_t l0i = uint64_t(1) << g.R, i0 = ind[d] / l0i;
				L = (x[i0 + 1] - x[i0]) / double(uint64_t(1) << lvl);
				const double length_of_index = (x[i0 + 1] - x[i0]) / double(l0i);
				c = x[i0] + length_of_index * double(ind[d] - i0 * l0i) + L / 2;
			} else if (lvl >= 0) {  // dccrg_cartesian_geometry.hpp:299-303, 334-359
				L = g.l0[d] * (1.0 / double(uint64_t(1) << lvl));
				c = g.start[d] + double(ind[d]) * g.l0[d] / double(uint64_t(1) << g.R) + L / 2;
			}
			if (length) length[3 * i + d] = L;
			if (center) center[3 * i + d] = c;
		}
	}
}

}  // namespace dccrgx
