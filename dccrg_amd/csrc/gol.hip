// The uniform game of life (examples/game_of_life.cpp:54-79,
// tests/game_of_life/scalability3d.cpp:130-165 of the reference): the
// structured 26-point sweep over boxes of whole z planes, the walk over the
// iterator neighbor lists for every other mesh or partition, and their
// driver gol_step.  The refined game is gol_amr.hip.  Bandwidth-bound.
#include <algorithm>

#include "dccrgx_grid.hpp"

namespace dccrgx {

namespace {

// Game of life over the iterator neighbor list (deduplicated neighbors_of),
// for refined meshes and partitions the structured kernel cannot take.  One
// block per 256 consecutive rows: phase 1 reads the block's entries (one
// contiguous run of the CSR) coalesced, four per thread and word, and
// gathers their states eight in flight per thread into one LDS byte each;
// phase 2 sums each row from LDS (rows past the LDS window gather directly).
// Blocks are dealt XCD-contiguously (block b runs on XCD b % 8), so the rows
// whose states a block gathers were loaded into the same L2.
constexpr int kGolRows = 256;
__global__ __launch_bounds__(kGolRows) void gol_csr_kernel(const uint32_t* __restrict__ state,
                                                         uint32_t* __restrict__ out, const uint32_t* __restrict__ ptr,
                                                         const int32_t* __restrict__ nb, size_t s0, size_t s1) {
	constexpr uint32_t cap = 8192;  // entry bytes staged per block
	__shared__ uint32_t sp32[cap / 4];
	const uint32_t tid = threadIdx.x;
	const uint32_t lb = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
	const size_t r0 = s0 + size_t(lb) * kGolRows;
	if (r0 >= s1) return;  // block-uniform
	const size_t r1 = r0 + kGolRows < s1 ? r0 + kGolRows : s1;
	const uint32_t E0 = ptr[r0] & ~3u, E1 = ptr[r1];
	const uint32_t nB = E1 - E0 < cap ? E1 - E0 : cap;
	const uint32_t nw = (nB + 3) / 4;
	for (uint32_t w = tid; w < nw; w += 2 * kGolRows) {
		int32_t q[8];
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const uint32_t e = E0 + 4 * (w + (k >> 2) * kGolRows) + (k & 3);
			q[k] = e >= E0 + 4 * nw || e >= E1 ? -1 : nb[e];
		}
		uint32_t v[8];
#pragma unroll
		for (int k = 0; k < 8; k++) v[k] = q[k] >= 0 && state[q[k]] > 0 ? 1u : 0u;
		sp32[w] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
		if (w + kGolRows < nw) sp32[w + kGolRows] = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
	}
	__syncthreads();
	const size_t s = r0 + tid;
	if (s >= r1) return;
	const uint8_t* sp8 = reinterpret_cast<const uint8_t*>(sp32);
	uint32_t cnt = 0;
	for (uint32_t j = ptr[s], e = ptr[s + 1]; j < e; j++)
		cnt += j - E0 < nB ? sp8[j - E0] : (state[nb[j]] > 0 ? 1u : 0u);
	const uint32_t cur = state[s];
	out[s] = cnt == 3 ? 1u : (cnt == 2 ? cur : 0u);
}

// Uniform 26-point game of life (nx a multiple of 256): a lane owns 4
// consecutive x (16-B loads and stores), a wave one 256-x segment of YR
// consecutive y rows, a block G3_ROWS such waves of the same segment; each
// wave marches a chunk of zc planes with the raw loads of the next DEPTH
// planes in flight while the current one is summed (8 B per
// cell-update, the y+-1 rows and the segment-edge columns are re-reads served
// by L2).  Blocks are dealt to XCDs in contiguous runs of the (x segment, y,
// z chunk) order, so the rows shared by vertically adjacent blocks stay in
// one XCD's L2.
#ifndef DCCRGX_G3_ROWS
#define DCCRGX_G3_ROWS 4
#endif
constexpr int G3_ROWS = DCCRGX_G3_ROWS;

// A plane's YR + 2 rows are loaded once per wave for YR output rows, so the
// L2 reads of the y+-1 rows are 4 (YR + 2) / YR B per cell instead of the 12 B
// of one row per wave (gol_structured_v3, removed with the <3, 2>, <1, 4> and
// <2, 4> forms after their A/B, profiles/r06ze_gol_yr_ab.txt: 0.1118 ->
// 0.1083 ms per sweep for <2, 2>; four rows: 185 VGPRs, slower).  The store
// is streaming: the next state is not read again in this sweep, so keeping
// it out of L2 leaves room for the planes in flight (paired A/B on config 2:
// 0.113 -> 0.108 ms per sweep).
template <int DEPTH, int YR>
__global__ __launch_bounds__(64 * G3_ROWS) void gol_structured_yr(const uint32_t* __restrict__ st,
                                                                 uint32_t* __restrict__ out, int nx, int ny, int nz,
                                                                 int px, int py, int pz, int zc, unsigned nbx,
                                                                 unsigned nby, unsigned nb,
                                                                 const uint32_t* __restrict__ lo,
                                                                 const uint32_t* __restrict__ hi) {
	constexpr int NR = YR + 2;
	const unsigned per_xcd = gridDim.x >> 3;
	const unsigned L = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
	if (L >= nb) return;  // block-uniform
	const unsigned bx = L % nbx, r = L / nbx, by = r % nby, bz = r / nby;
	const int lane = threadIdx.x & 63;
	const int y0 = (int(by) * G3_ROWS + int(threadIdx.x >> 6)) * YR;
	if (y0 >= ny) return;  // wave-uniform
	const int x0 = int(bx) * 256;
	const int x = x0 + 4 * lane;
	// row i of a plane is y0 - 1 + i, wrapped or absent (-1)
	size_t orow[NR];
	bool rin[NR];
#pragma unroll
	for (int i = 0; i < NR; i++) {
		int y = y0 - 1 + i;
		bool in = true;
		if (y < 0) {
			if (py) y += ny;
			else in = false;
		} else if (y >= ny) {
			if (py) y -= ny;
			else in = false;
		}
		// row i feeds the output rows max(0, i - 2) .. min(i, YR - 1): absent
		// when the first of them is (the one subtraction above leaves y >= ny
		// for ny == 1: a row past the plane)
		if (y0 + max(0, i - 2) >= ny) in = false;
		rin[i] = in;
		orow[i] = in ? size_t(y) * nx : 0;
	}
	int xe = -1;
	if (lane == 0) xe = x0 > 0 ? x0 - 1 : (px ? nx - 1 : -1);
	if (lane == 63) xe = x0 + 256 < nx ? x0 + 256 : (px ? 0 : -1);
	const size_t plane = size_t(nx) * ny;
	struct P {
		uint4 v[NR];
		uint32_t e[NR];
	};
	auto load = [&](int z, P& Q) {
#pragma unroll
		for (int i = 0; i < NR; i++) {
			Q.v[i] = make_uint4(0, 0, 0, 0);
			Q.e[i] = 0;
		}
		const uint32_t* p;
		if (z < 0) p = lo ? lo : (pz ? st + size_t(z + nz) * plane : nullptr);
		else if (z >= nz) p = hi ? hi : (pz ? st + size_t(z - nz) * plane : nullptr);
		else p = st + size_t(z) * plane;
		if (!p) return;
#pragma unroll
		for (int i = 0; i < NR; i++)
			if (rin[i]) Q.v[i] = *reinterpret_cast<const uint4*>(p + orow[i] + x);
		if (xe >= 0) {
#pragma unroll
			for (int i = 0; i < NR; i++)
				if (rin[i]) Q.e[i] = p[orow[i] + xe];
		}
	};
	// per output row k the in-plane 3x3 sums at this lane's 4 x
	auto psum = [&](const P& Q, uint32_t s[YR][4]) {
		uint32_t c[NR][4], ce[NR];
#pragma unroll
		for (int i = 0; i < NR; i++) {
			c[i][0] = Q.v[i].x > 0;
			c[i][1] = Q.v[i].y > 0;
			c[i][2] = Q.v[i].z > 0;
			c[i][3] = Q.v[i].w > 0;
			ce[i] = Q.e[i] > 0;
		}
#pragma unroll
		for (int k = 0; k < YR; k++) {
			const uint32_t c0 = c[k][0] + c[k + 1][0] + c[k + 2][0], c1 = c[k][1] + c[k + 1][1] + c[k + 2][1],
			               c2 = c[k][2] + c[k + 1][2] + c[k + 2][2], c3 = c[k][3] + c[k + 1][3] + c[k + 2][3];
			const uint32_t cee = ce[k] + ce[k + 1] + ce[k + 2];
			uint32_t l = __shfl_up(c3, 1, 64), rr = __shfl_down(c0, 1, 64);
			if (lane == 0) l = cee;
			if (lane == 63) rr = cee;
			s[k][0] = l + c0 + c1;
			s[k][1] = c0 + c1 + c2;
			s[k][2] = c1 + c2 + c3;
			s[k][3] = c2 + c3 + rr;
		}
	};
	const int z0 = int(bz) * zc;
	const int z1 = min(z0 + zc, nz);
	P A, Q[DEPTH];
	uint32_t sp[YR][4], sc[YR][4], sn[YR][4];
	uint4 cur[YR];
	load(z0 - 1, A);
	psum(A, sp);
	load(z0, A);
	psum(A, sc);
#pragma unroll
	for (int k = 0; k < YR; k++) cur[k] = A.v[k + 1];
#pragma unroll
	for (int i = 0; i < DEPTH; i++)
		if (z0 + 1 + i <= z1) load(z0 + 1 + i, Q[i]);
	for (int z = z0; z < z1; z++) {
		P E = Q[DEPTH - 1];
		if (z + 1 + DEPTH <= z1) load(z + 1 + DEPTH, E);
		psum(Q[0], sn);
#pragma unroll
		for (int k = 0; k < YR; k++) {
			if (y0 + k >= ny) continue;
			uint4 o;
			uint32_t cnt;
			cnt = sp[k][0] + sc[k][0] + sn[k][0] - (cur[k].x > 0);
			o.x = cnt == 3 ? 1u : (cnt == 2 ? cur[k].x : 0u);
			cnt = sp[k][1] + sc[k][1] + sn[k][1] - (cur[k].y > 0);
			o.y = cnt == 3 ? 1u : (cnt == 2 ? cur[k].y : 0u);
			cnt = sp[k][2] + sc[k][2] + sn[k][2] - (cur[k].z > 0);
			o.z = cnt == 3 ? 1u : (cnt == 2 ? cur[k].z : 0u);
			cnt = sp[k][3] + sc[k][3] + sn[k][3] - (cur[k].w > 0);
			o.w = cnt == 3 ? 1u : (cnt == 2 ? cur[k].w : 0u);
			typedef unsigned int u4v __attribute__((ext_vector_type(4)));
			u4v ov = {o.x, o.y, o.z, o.w};
			__builtin_nontemporal_store(ov, reinterpret_cast<u4v*>(out + size_t(z) * plane + size_t(y0 + k) * nx + x));
		}
#pragma unroll
		for (int k = 0; k < YR; k++) {
#pragma unroll
			for (int i = 0; i < 4; i++) {
				sp[k][i] = sc[k][i];
				sc[k][i] = sn[k][i];
			}
			cur[k] = Q[0].v[k + 1];
		}
#pragma unroll
		for (int i = 0; i + 1 < DEPTH; i++) Q[i] = Q[i + 1];
		Q[DEPTH - 1] = E;
	}
}

}  // namespace

static void k_gol_csr(const uint32_t* state, uint32_t* out, const uint32_t* it_ptr, const int32_t* it_slot, size_t s0,
                      size_t s1, hipStream_t s) {
	if (s1 <= s0) return;
	const size_t nb = (s1 - s0 + kGolRows - 1) / kGolRows;
	gol_csr_kernel<<<unsigned((nb + 7) / 8 * 8), kGolRows, 0, s>>>(state, out, it_ptr, it_slot, s0, s1);
	HIP_CHECK(hipGetLastError());
}

// uniform 26-point game of life on a box of nx x ny x nz cells stored in
// raster order; planes z = -1 and z = nz come from lo / hi (nullptr: outside);
// false when the box does not fit the structured kernel (nx % 256 != 0)
static bool k_gol_structured(const uint32_t* state, uint32_t* out, const uint64_t n[3], const int per[3],
                             const uint32_t* lo, const uint32_t* hi, hipStream_t s) {
	if (n[0] % 256 != 0 || n[0] * n[1] * n[2] >= (uint64_t(1) << 32) || n[2] == 0) return false;
	// 64 planes per z chunk, two rows per wave and two planes of loads in
	// flight (r01g/r01j sweeps over zc and the depth on config 2)
	const int zc = int(std::min<uint64_t>(n[2], 64));
	const unsigned rows = unsigned(G3_ROWS * 2);
	const unsigned nbx = unsigned(n[0] / 256), nby = unsigned((n[1] + rows - 1) / rows),
	               nbz = unsigned((n[2] + zc - 1) / zc);
	const size_t nb = size_t(nbx) * nby * nbz;
	const unsigned grid = unsigned((nb + 7) / 8 * 8);
	gol_structured_yr<2, 2><<<grid, 64 * G3_ROWS, 0, s>>>(state, out, int(n[0]), int(n[1]), int(n[2]), per[0], per[1],
	                                                      per[2], zc, nbx, nby, unsigned(nb), lo, hi);
	HIP_CHECK(hipGetLastError());
	return true;
}

// --------------------------------------------------------------------------- slab planes
// The structured 26-point sweep needs the cells of a box in raster order.
// On a uniform level-0 grid whose ranks hold whole z-planes (the block
// partition, or any repartition into z-planes) a rank holds its planes in
// slot order [inner planes | outer planes] and receives each neighbor plane as
// one contiguous run of halo slots, so every region is a set of boxes whose
// z-1 / z+1 planes are other runs.
static int64_t plane_slot(Grid& g, int64_t z) {
	const int64_t nz = int64_t(g.len[2]);
	if (z < 0 || z >= nz) {
		if (!g.per[2]) return -2;  // outside the grid
		z = (z % nz + nz) % nz;
	}
	const uint64_t plane = g.len[0] * g.len[1];
	const uint64_t first = 1 + uint64_t(z) * plane, last = first + plane - 1;
	const int64_t a = lookup_slot(g, first), b = lookup_slot(g, last);
	if (a < 0 || b != a + int64_t(plane) - 1) return -1;  // not one contiguous run
	return a;
}

static bool gol_slab_plan(Grid& g, std::vector<GolBox>& inner, std::vector<GolBox>& outer) {
	inner.clear();
	outer.clear();
	if (g.R != 0 || g.hood_len != 1 || g.len[0] % 256 != 0) return false;
	const uint64_t plane = g.len[0] * g.len[1];
	const int64_t nz = int64_t(g.len[2]);
	if (!g.n_local || g.n_local % plane != 0) return false;
	if (g.size == 1 && g.n_outer == 0 && g.n_slots == g.n_local && g.n_local == plane * uint64_t(nz)) {
		inner.push_back(GolBox{0, uint64_t(nz), -3, -3});  // -3: the kernel's own periodic wrap
		return true;
	}
	// the own cells must be whole planes, each one run of local slots of one
	// class (inner or outer); any number of z runs (e.g. a rank holding two
	// slabs after a repartition)
	std::vector<int64_t> own(size_t(nz), -1);
	uint64_t owned = 0;
	for (int64_t z = 0; z < nz; z++) {
		const int64_t s0 = plane_slot(g, z);
		if (s0 < 0 || uint64_t(s0) + plane > g.n_local) continue;
		if ((uint64_t(s0) < g.n_inner) != (uint64_t(s0) + plane - 1 < g.n_inner)) return false;
		own[size_t(z)] = s0;
		owned++;
	}
	if (owned * plane != g.n_local) return false;
	auto slot = [&](int64_t z) -> int64_t {
		return (z >= 0 && z < nz && own[size_t(z)] >= 0) ? own[size_t(z)] : plane_slot(g, z);
	};
	// boxes: runs of inner planes consecutive in z and in slots; every outer
	// plane alone; z-1 / z+1 of a box: another run (local or halo) or nothing
	for (int64_t z = 0; z < nz;) {
		if (own[size_t(z)] < 0) {
			z++;
			continue;
		}
		const bool in = uint64_t(own[size_t(z)]) < g.n_inner;
		int64_t e = z + 1;
		while (in && e < nz && own[size_t(e)] >= 0 && uint64_t(own[size_t(e)]) < g.n_inner &&
		       own[size_t(e)] == own[size_t(e - 1)] + int64_t(plane))
			e++;
		const int64_t lo = slot(z - 1), hi = slot(e);
		if (lo == -1 || hi == -1) return false;  // a neighbor plane not held as one run
		(in ? inner : outer).push_back(GolBox{uint64_t(own[size_t(z)]), uint64_t(e - z), lo, hi});
		z = e;
	}
	return true;
}

// one step of the uniform game over a region into the field's scratch
// (dccrgx_gol_step): the structured sweep over the slab plan's boxes, else the
// CSR walk
void gol_step(Grid& g, int sf, int region) {
	Field& f = field(g, sf);
	DX_REQUIRE(f.elem == 4, "game of life state must be a 4-byte field");
	ensure_scratch(g, f);
	size_t s0, s1;
	region_range(g, region, s0, s1);
	if (s1 <= s0) return;
	if (!g.gol_plan_valid) {
		g.gol_plan_ok = gol_slab_plan(g, g.gol_inner, g.gol_outer);
		g.gol_plan_valid = true;
	}
	const uint32_t* st = (const uint32_t*)f.data.p;
	uint32_t* out = (uint32_t*)f.scratch.p;
	k_time_begin(g);
	bool done = false;
	if (g.gol_plan_ok) {
		done = true;
		for (int r = 0; r < 2 && done; r++) {
			if (r == 0 && region == DCCRGX_REGION_OUTER) continue;
			if (r == 1 && region == DCCRGX_REGION_INNER) continue;
			for (const GolBox& b : r == 0 ? g.gol_inner : g.gol_outer) {
				const uint64_t n[3] = {g.len[0], g.len[1], b.nz};
				const int per[3] = {g.per[0], g.per[1], b.lo == -3 ? g.per[2] : 0};
				const uint32_t* lo = b.lo >= 0 ? st + uint64_t(b.lo) : nullptr;
				const uint32_t* hi = b.hi >= 0 ? st + uint64_t(b.hi) : nullptr;
				if (!k_gol_structured(st + b.slot0, out + b.slot0, n, per, lo, hi, g.s_comp)) {
					done = false;
					break;
				}
			}
		}
	}
	if (!done) {
		ensure_csr(g);
		k_gol_csr(st, out, g.it_ptr.p, g.it_slot.p, s0, s1, g.s_comp);
	}
	k_time_end(g);
}

}  // namespace dccrgx
