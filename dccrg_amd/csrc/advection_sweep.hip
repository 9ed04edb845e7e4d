// The advection sweeps (tests/advection/solve.hpp:44-279 of the reference,
// calculate_fluxes + apply_fluxes fused: every cell gathers its own faces, so
// the reference's scatter into two cells becomes a race-free gather with no
// atomics): the flux functions, the untiled sweep over the face CSR, the
// face-table sweep of a mesh that has just changed, and the two persistent
// tile sweeps (regular boxes, any other tile) with the neighbor records, the
// length-table and uniform-velocity checks, and their launchers.  The driver
// and the choice of what a sweep runs with (adv_sweep_plan) are advection.hip,
// the time step and the adaptation kernels advection_adapt.hip.
// All bandwidth-bound; no MFMA.
#include <algorithm>
#include <type_traits>

#include "dccrgx_internal.hpp"

namespace dccrgx {

namespace {

// ---------------------------------------------------------------------------
// Face flux without the division by the cell volume (applied once per cell):
// the face velocity and the upwind flux keep the reference's expression
// (solve.hpp:169-225), so only the per-cell rounding of the sum differs.
__device__ __forceinline__ double adv_face_flux(int dir, double cd, double cl_a, double cl_b, double cl_c,
                                                double cvel, double nd, double nl_a, double nl_b, double nl_c,
                                                double nv, double dt) {
#pragma clang fp contract(off)
	// cl_a = the cell's length along the face normal, cl_b/cl_c transverse
	const double min_area = fmin(cl_b * cl_c, nl_b * nl_c);
	const double v = (cl_a * nv + nl_a * cvel) / (cl_a + nl_a);
	if (dir & 1) return -((v >= 0 ? cd : nd) * dt * v * min_area);
	return (v >= 0 ? nd : cd) * dt * v * min_area;
}

// The same flux through a face between two cells of one level, whose lengths
// are then the same bits (the length table's row): cl_a + nl_a = 2 cl_a is a
// power of two and rinv its reciprocal (Grid::LenTable::pow2), so the product
// is bitwise the quotient, and fmin of the two equal areas is the area.
__device__ __forceinline__ double adv_face_flux_same(int dir, double cd, double cl_a, double cl_b, double cl_c,
                                                     double cvel, double nd, double nv, double rinv, double dt) {
#pragma clang fp contract(off)
	const double min_area = cl_b * cl_c;
	const double v = (cl_a * nv + cl_a * cvel) * rinv;
	if (dir & 1) return -((v >= 0 ? cd : nd) * dt * v * min_area);
	return (v >= 0 ? nd : cd) * dt * v * min_area;
}

struct AdvNb {
	double d, lx, ly, lz, v;
};

__device__ __forceinline__ double adv_face_flux_d(int d, double cd, double clx, double cly, double clz, double cvx,
                                                  double cvy, double cvz, const AdvNb& n, double dt) {
	if (d < 2) return adv_face_flux(d, cd, clx, cly, clz, cvx, n.d, n.lx, n.ly, n.lz, n.v, dt);
	if (d < 4) return adv_face_flux(d, cd, cly, clx, clz, cvy, n.d, n.ly, n.lx, n.lz, n.v, dt);
	return adv_face_flux(d, cd, clz, clx, cly, cvz, n.d, n.lz, n.lx, n.ly, n.v, dt);
}

// Advection (tests/advection/solve.hpp:44-279), fp64, fused flux + apply,
// for runs the tile sweeps cannot take (tiles beyond the LDS capacity).
// Face entry = neighbor slot * 8 + dir (0..5 = -x,+x,-y,+y,-z,+z).  Every
// face flux is the tile sweeps' (the reference's expression and operand
// order, contraction off) and they are summed in the same face order and
// divided once by the cell volume, so a cell's new density is bitwise the
// same whichever sweep computes it.
__global__ void advection_kernel(const double* __restrict__ rho, const double* __restrict__ vx,
                                 const double* __restrict__ vy, const double* __restrict__ vz,
                                 const double* __restrict__ lx, const double* __restrict__ ly,
                                 const double* __restrict__ lz, double* __restrict__ rho_out,
                                 const uint32_t* __restrict__ ptr, const int32_t* __restrict__ ent, size_t s0, size_t s1,
                                 double dt) {
#pragma clang fp contract(off)
	for (size_t s = s0 + blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < s1; s += size_t(gridDim.x) * blockDim.x) {
		const double cd = rho[s];
		const double clx = lx[s], cly = ly[s], clz = lz[s];
		const double cvx = vx[s], cvy = vy[s], cvz = vz[s];
		double acc = 0;
		const uint32_t e0 = ptr[s], e1 = ptr[s + 1];
		for (uint32_t e = e0; e < e1; e++) {
			const int32_t en = ent[e];
			const int32_t n = en >> 3;
			const int dir = en & 7;
			const double nv = dir < 2 ? vx[n] : (dir < 4 ? vy[n] : vz[n]);
			acc += adv_face_flux_d(dir, cd, clx, cly, clz, cvx, cvy, cvz, AdvNb{rho[n], lx[n], ly[n], lz[n], nv}, dt);
		}
		rho_out[s] = cd + acc / (clx * cly * clz);
	}
}

// The same sweep over the fixed-width face table of ensure_face
// (face_table_kernel: ell[6 r + d] = the neighbor's slot, -1 none, -2 - f the
// four finer neighbors fine[4 f ..] in the reference's order): the sweep of a
// mesh that has just changed, before (and instead of) building its tiles.
// One thread per cell, the row's six codes as three 8-B loads, the same face
// fluxes summed in the same face order as advection_kernel and the tile
// sweeps, so the new density is bitwise theirs.  A block sweeps 256
// consecutive slots (Morton order: a compact box, where about five in six
// face neighbors are cells of the same block), reads its cells' seven values
// once, coalesced, into LDS and takes every neighbor inside the block from
// there; the others are gathered from the fields (profiles/r05_ell_lds_ab.txt:
// 0.326 -> 0.278 ms against the gather-only form, since removed).
// BANDS: check_for_adaptation's band of every swept cell as well (the
// densities it compares are the ones the sweep reads): adv_max_diff's
// comparisons in its order - a coarser single neighbor only from the corner
// of its face, of a finer face only the first cell - and adv_bands_kernel's
// thresholds, so the bytes are that kernel's.
template <bool BANDS>
__global__ __launch_bounds__(256) void advection_ell_lds_kernel(
    const double* __restrict__ rho, const double* __restrict__ vx, const double* __restrict__ vy,
    const double* __restrict__ vz, const double* __restrict__ lx, const double* __restrict__ ly,
    const double* __restrict__ lz, double* __restrict__ rho_out, const int32_t* __restrict__ ell,
    const int32_t* __restrict__ fine, size_t s0, size_t s1, double dt, BandArgs B) {
#pragma clang fp contract(off)
	typedef int i2v __attribute__((ext_vector_type(2)));
	typedef int i4v __attribute__((ext_vector_type(4)));
	__shared__ double sd[256], svx[256], svy[256], svz[256], slx[256], sly[256], slz[256];
	__shared__ uint8_t slv[BANDS ? 256 : 1];
	const unsigned t = threadIdx.x;
	for (size_t b0 = s0 + blockIdx.x * size_t(256); b0 < s1; b0 += size_t(gridDim.x) * 256) {
		const size_t s = b0 + t;
		const bool live = s < s1;
		const uint32_t nb_in = uint32_t(min(size_t(256), s1 - b0));
		double cd = 0, clx = 1, cly = 1, clz = 1, cvx = 0, cvy = 0, cvz = 0;
		int32_t e6[6] = {-1, -1, -1, -1, -1, -1};
		int lvl = 0;
		unsigned oct = 0;
		if (live) {
			cd = rho[s];
			clx = lx[s];
			cly = ly[s];
			clz = lz[s];
			cvx = vx[s];
			cvy = vy[s];
			cvz = vz[s];
			if (BANDS) {
				const unsigned v = B.lvl8[s];
				lvl = int(v & 31u);
				oct = v >> 5;
			}
			const i2v* ev = reinterpret_cast<const i2v*>(ell + 6 * s);
#pragma unroll
			for (int j = 0; j < 3; j++) {
				const i2v v = ev[j];
				e6[2 * j] = v.x;
				e6[2 * j + 1] = v.y;
			}
		}
		__syncthreads();  // the previous chunk's readers are done with LDS
		sd[t] = cd;
		svx[t] = cvx;
		svy[t] = cvy;
		svz[t] = cvz;
		slx[t] = clx;
		sly[t] = cly;
		slz[t] = clz;
		if (BANDS) slv[t] = uint8_t(lvl);
		__syncthreads();
		if (!live) continue;
		auto nb = [&](int32_t n, int dir) {
			const uint32_t k = uint32_t(int64_t(n) - int64_t(b0));
			if (k < nb_in) {
				const double nv = dir < 2 ? svx[k] : (dir < 4 ? svy[k] : svz[k]);
				return AdvNb{sd[k], slx[k], sly[k], slz[k], nv};
			}
			const double nv = dir < 2 ? vx[n] : (dir < 4 ? vy[n] : vz[n]);
			return AdvNb{rho[n], lx[n], ly[n], lz[n], nv};
		};
		double acc = 0, md = 0;
		auto band_cmp = [&](double b) {
			const double diff = fabs(cd - b) / (fmin(cd, b) + B.thr);
			md = fmax(diff, md);
		};
#pragma unroll
		for (int dir = 0; dir < 6; dir++) {
			const int32_t c = e6[dir];
			if (c == -1) continue;
			if (c >= 0) {
				const AdvNb q = nb(c, dir);
				acc += adv_face_flux_d(dir, cd, clx, cly, clz, cvx, cvy, cvz, q, dt);
				if (BANDS) {
					const uint32_t k = uint32_t(int64_t(c) - int64_t(b0));
					const int nl = k < nb_in ? int(slv[k]) : int(B.lvl8[c] & 31u);
					// coarser: only from the corner of its face, i.e. the
					// cell's octant bits across the face axis are zero
					if (nl >= lvl || (oct & ~(1u << (dir >> 1))) == 0) band_cmp(q.d);
				}
			} else {
				const i4v q = *reinterpret_cast<const i4v*>(fine + 4 * size_t(-2 - c));
				const AdvNb first = nb(q.x, dir);
				acc += adv_face_flux_d(dir, cd, clx, cly, clz, cvx, cvy, cvz, first, dt);
				acc += adv_face_flux_d(dir, cd, clx, cly, clz, cvx, cvy, cvz, nb(q.y, dir), dt);
				acc += adv_face_flux_d(dir, cd, clx, cly, clz, cvx, cvy, cvz, nb(q.z, dir), dt);
				acc += adv_face_flux_d(dir, cd, clx, cly, clz, cvx, cvy, cvz, nb(q.w, dir), dt);
				if (BANDS) band_cmp(first.d);
			}
		}
		rho_out[s] = cd + acc / (clx * cly * clz);
		if (BANDS) {
			const double refine_diff = (lvl + 1) * B.inc, unrefine_diff = B.uns * refine_diff;
			B.band[s] = md > refine_diff ? 2 : (md >= unrefine_diff ? 1 : 0);
		}
	}
}

// 32-bit byte offsets from a uniform base: global_load v, voff, s[base]
// (halves the address registers of a gather; slots < 2^29, checked on the host)
__device__ __forceinline__ double ldo(const double* __restrict__ p, uint32_t off) {
	return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(p) + off);
}

// density store of the tile sweeps: non-temporal (a streaming write that
// should not allocate over the face lines neighboring tiles re-read from
// L2; measured on config 3: 0.1960 -> 0.1945 ms per sweep.  The same hint on
// the own-field loads cost 12 %: those lines ARE the re-read face lines)
__device__ __forceinline__ void st_nt(double* __restrict__ p, uint32_t i, double v) {
	__builtin_nontemporal_store(v, p + i);
}

// Regular tiles (tile_build.hip classify_tiles_kernel): an aligned 8x8x8 box
// of same-level cells, slots ts..ts+511 in Morton order, whose face
// neighbors across each side are the same-level cells of one neighbor box
// starting at slot tnb[6 gt + d] (-1: no neighbor on that side).  Thread t
// owns the cell with local Morton index t.  Own fields are staged in LDS for
// the in-tile faces; the (at most three) out-of-tile face neighbors of a
// cell are each used by that cell alone, so they are read straight into
// registers, issued before the barrier.  No per-cell face rows are read.
__device__ __forceinline__ uint32_t m9(uint32_t x, uint32_t y, uint32_t z) {
	return (x & 1u) | ((y & 1u) << 1) | ((z & 1u) << 2) | ((x & 2u) << 2) | ((y & 2u) << 3) | ((z & 2u) << 4) |
	       ((x & 4u) << 4) | ((y & 4u) << 5) | ((z & 4u) << 6);
}

// the out-of-tile neighbors of a regular tile, flattened: k = (side * 5 +
// value) * 64 + face cell (value 0 rho, 1 lx, 2 ly, 3 lz, 4 the velocity
// along the side's axis): 30 (side, value) rows of 64, wave w loads rows w,
// w + 8, w + 16, w + 24, so side and value are wave-uniform (scalar pointer
// and neighbor-box start, no private-memory lookup tables)
struct AdvPtrs {
	const double* p[7];  // rho, lx, ly, lz, vx, vy, vz
};

// The upwind flux through one face with the cell `c` on its minus side and
// `n` on its plus side, along axis a (solve.hpp:136-225 for direction +a):
// the reference's expression and operand order.  The minus-side cell adds
// -G, the plus-side cell +G; evaluated from the plus side the reference
// computes the same products in swapped (commutative) order, so one
// evaluation per face is bitwise what each side would get.
// P2: ca + na is a power of two and rinv its reciprocal, a normal double
// (Grid::LenTable::pow2): the product rounds the real number the quotient
// rounds, so v has the same bits for every numerator.
template <bool P2 = false>
__device__ __forceinline__ double adv_face_g(int a, double cd, double clx, double cly, double clz, double cv_a,
                                             const AdvNb& n, double dt, double rinv = 0) {
#pragma clang fp contract(off)
	double ca, cb, cc, na, nb, nc;
	if (a == 0) { ca = clx; cb = cly; cc = clz; na = n.lx; nb = n.ly; nc = n.lz; }
	else if (a == 1) { ca = cly; cb = clx; cc = clz; na = n.ly; nb = n.lx; nc = n.lz; }
	else { ca = clz; cb = clx; cc = cly; na = n.lz; nb = n.lx; nc = n.ly; }
	const double min_area = fmin(cb * cc, nb * nc);
	const double num = ca * n.v + na * cv_a;
	const double v = P2 ? num * rinv : num / (ca + na);
	return (v >= 0 ? cd : n.d) * dt * v * min_area;
}

// Tile records (32 B) are read one tile ahead of their use by a vector load
// (lanes 0..7 one word each) and made uniform with readlane.  A scalar load
// issued that early would not help: the next LDS wait (lgkmcnt counts LDS and
// scalar memory alike) would wait for it, exposing its latency once per tile;
// the vector counter is in order, so waiting for the previous tile's fields
// does not wait for the record loaded after them.
__device__ __forceinline__ uint32_t tile_record_word(const void* meta, uint32_t tt, uint32_t lane) {
	return lane < 8u ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(meta) + 8u * tt + lane) : 0u;
}

__device__ __forceinline__ uint32_t word_of(uint32_t v, int k) {
	return uint32_t(__builtin_amdgcn_readlane(int(v), k));
}

// Static persistent schedule of the tile sweeps: block b runs on XCD b % 8
// (measured: scripts/microbench/xcd_map.hip); XCD x sweeps the x-th eighth
// of the tile list, its B blocks side by side (block j: tiles j, j + B, ...),
// so the tiles an XCD has in flight are Morton neighbors sharing L2 lines.
struct StaticTiles {
	uint32_t t0, t1, B;
	__device__ __forceinline__ explicit StaticTiles(uint32_t ntiles) {
		const uint32_t x = blockIdx.x & 7u;
		B = gridDim.x >> 3;
		t0 = uint32_t((uint64_t(x) * ntiles) >> 3);
		t1 = uint32_t((uint64_t(x + 1) * ntiles) >> 3);
	}
	__device__ __forceinline__ uint32_t first() const { return t0 + (blockIdx.x >> 3); }
	__device__ __forceinline__ uint32_t next(uint32_t t) const { return t + B; }
};

// Neighbor records (Grid::NbRecords): per axis a and slot s the 24-B record
// {l_a, l_b * l_c, v_a} at r[3 a n + 3 s], b < c the two other axes, the
// product formed as the reference forms a face's area (solve.hpp:142-161).
// An out-of-tile face neighbor across an a-face then costs its density and
// this record (one line or two) instead of its density, three lengths and
// v_a from five arrays.  The sweeps stage such a neighbor into LDS with its
// length along a in row l_a, the area in the row of the first transverse
// length (nb_area_row) and 1.0 in the other (nb_one_row): every flux
// expression then forms nb * nc = area * 1.0 = area exactly, so the fluxes
// are bitwise those from the fields.
__global__ void nbrec_kernel(const double* __restrict__ lx, const double* __restrict__ ly,
                             const double* __restrict__ lz, const double* __restrict__ vx,
                             const double* __restrict__ vy, const double* __restrict__ vz, size_t n,
                             double* __restrict__ r) {
#pragma clang fp contract(off)
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x) {
		const double x = lx[s], y = ly[s], z = lz[s];
		double* r0 = r + 3 * s;
		double* r1 = r + 3 * n + 3 * s;
		double* r2 = r + 6 * n + 3 * s;
		r0[0] = x;
		r0[1] = y * z;
		r0[2] = vx[s];
		r1[0] = y;
		r1[1] = x * z;
		r1[2] = vy[s];
		r2[0] = z;
		r2[1] = x * y;
		r2[2] = vz[s];
	}
}

// LDS / register rows (4 lx, 5 ly, 6 lz) of a record-staged neighbor across
// an a-face: the area in the row of nb, 1.0 in the row of nc, where
// adv_face_g / adv_face_flux take (nb, nc) = (ly, lz), (lx, lz), (lx, ly)
__device__ __forceinline__ uint32_t nb_area_row(uint32_t a) { return a == 0 ? 5u : 4u; }
__device__ __forceinline__ uint32_t nb_one_row(uint32_t a) { return a == 2 ? 5u : 6u; }

//
// LEN: the grid's length fields are bitwise l0[d] * 2^-level (ensure_len_table
// verified it), LT its per-level table (32 rows of lx, ly, lz, copied to LDS).
// A regular tile and its neighbor boxes are one level, the record's last
// word, so the tile's three lengths are block-uniform values from the table:
// the out-of-tile rows shrink from 30 to 12 (per side the density and the
// velocity along the side's axis) and (DCCRGX_LEN_OWN) the own loads from
// seven to four.  The lengths never enter LDS (LREG): shd keeps the four rows
// rho, vx, vy, vz, and every length a face reads - the own cell's, the +a
// neighbor's, the -a boundary faces' - is the tile's uniform tl[], the same
// bits in the same operands, so the densities are bitwise the field-reading
// kernel's.  That is a third fewer LDS instructions per tile and 42.3 KB of
// LDS instead of 64 KB; at 76 VGPRs the kernel is compiled for, and
// launched with, three blocks per CU (DCCRGX_REG_BLOCKS;
// profiles/len_lds_ab.md).  DCCRGX_LEN_LDS=1 or DCCRGX_LEN_OWN=0 keep the
// seven rows, staged from the table, and two blocks.
//
// UM (ensure_vel_uniform verified it): bit a set - velocity component a holds
// one 64-bit pattern in every slot, uv.v[a].  Such a component is neither
// loaded nor staged: shd keeps the density and the other components' rows
// (vel_row), the out-of-tile rows are six density rows and two velocity rows
// per other axis, and every operand that was the component - the own cell's,
// a neighbor's, a boundary face's two - is uv.v[a], the same bits, so the
// densities are bitwise the UM = 0 kernel's.  No arithmetic is skipped.
//
// P2 (Grid::LenTable::pow2 verified it on the host): every level's 2 l_a and
// volume are powers of two whose reciprocals are normal doubles, and LT
// carries them behind the lengths (kLenTabP2 doubles: 96 lengths, 96 times
// 1 / (2 l_a), 32 times 1 / volume).  A face between two cells of one level
// divides by l_a + l_a = 2 l_a and a cell by its volume: both multiply by the
// table's reciprocal instead, which rounds the same real number, so the bits
// are the quotient's for every numerator (inf, NaN payloads and subnormals
// included).  A face between two levels (3 l_a: not a power of two) divides.
struct AdvUV {
	double v[3];
};
// LDS row of velocity component a when the components of mask um have none
__host__ __device__ constexpr uint32_t vel_row(int um, uint32_t a) {
	return 1u + a - uint32_t(__builtin_popcount(unsigned(um) & ((1u << a) - 1u)));
}
// the k-th axis (ascending) that is not in mask um
__host__ __device__ constexpr uint32_t vel_live_axis(int um, uint32_t k) {
	uint32_t a = 0;
	for (; a < 3; a++) {
		if ((um >> a) & 1) continue;
		if (k == 0) break;
		k--;
	}
	return a;
}

// a block-uniform double out of the vector registers
__device__ __forceinline__ double uniform_f64(double x) {
	const long long b = __double_as_longlong(x);
	const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(b)), hi = __builtin_amdgcn_readfirstlane(uint32_t(b >> 32));
	return __longlong_as_double((long long)((uint64_t(hi) << 32) | lo));
}

template <int MINW, bool REC, bool LEN, int UM = 0, bool P2 = false>
__global__ __launch_bounds__(512, MINW) void advection_regular_pp_kernel(AdvPtrs P, double* __restrict__ rho_out,
                                                                         const RegTileMeta* __restrict__ meta,
                                                                         uint32_t ntiles, double dt,
                                                                         const double* __restrict__ R, size_t nrec,
                                                                         const double* __restrict__ LT, AdvUV uv) {
#pragma clang fp contract(off)
	static_assert(!(REC && LEN), "the length table is for the default kernels only");
	constexpr bool LOWN = LEN && DCCRGX_LEN_OWN;
	constexpr bool LREG = LOWN && !DCCRGX_LEN_LDS;  // the lengths stay in registers
	static_assert(UM == 0 || (LREG && UM > 0 && UM < 8), "uniform components: the register-length kernel only");
	static_assert(!P2 || LREG, "reciprocals: the register-length kernel only");
	constexpr uint32_t NLT = P2 ? kLenTabP2 : 96u;
	constexpr int NV = 3 - __builtin_popcount(unsigned(UM));  // velocity components with a row
	// rows rho, vx, vy, vz, lx, ly, lz; columns 0..511 the tile's own cells,
	// 512 + 64 d + (face cell) the out-of-tile neighbor across side d (only
	// rows rho, lx, ly, lz and the velocity along d's axis are filled), so
	// every face reads its neighbor through one LDS index, whichever side.
	// LREG: no length rows, every length a face reads is the tile's tl[]
	constexpr uint32_t W = 512 + 6 * 64;
	constexpr int NROW = LREG ? 1 + NV : 7;
	__shared__ double shd[NROW][W];
	__shared__ double shg[3][512];  // flux through each cell's +x, +y, +z face
	__shared__ double shm[3][64];   // flux through the tile's -x, -y, -z boundary faces
	__shared__ double lt[LEN ? NLT : 1];  // LEN: the per-level lengths (P2: and reciprocals)
	const StaticTiles tk(ntiles);
	const uint32_t t1 = tk.t1;
	uint32_t t = tk.first();
	if (t >= t1) return;  // block-uniform
	const uint32_t tid = threadIdx.x;
	if (LEN && tid < NLT) lt[tid] = LT[tid];  // (read after the first tile's first barrier)
	const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63u;
	const uint32_t l[3] = {(tid & 1u) | ((tid >> 2) & 2u) | ((tid >> 4) & 4u),
	                       ((tid >> 1) & 1u) | ((tid >> 3) & 2u) | ((tid >> 5) & 4u),
	                       ((tid >> 2) & 1u) | ((tid >> 4) & 2u) | ((tid >> 6) & 4u)};
	// index of this cell within a side of each axis (the two other coordinates)
	const uint32_t fi[3] = {l[1] + 8 * l[2], l[0] + 8 * l[2], l[0] + 8 * l[1]};
	// LDS column of the +a neighbor of this cell (inside the tile or across side 2a+1)
	uint32_t lp[3];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		uint32_t q[3] = {l[0], l[1], l[2]};
		q[a] += 1;
		lp[a] = l[a] < 7 ? m9(q[0], q[1], q[2]) : 512u + 64u * uint32_t(2 * a + 1) + fi[a];
	}
	// boundary-face duty of waves 0..2: wave a evaluates the -a side face of
	// the cell at l[a] = 0 whose face index is the lane
	const uint32_t bu = lane & 7u, bv = lane >> 3;
	const uint32_t bcell = w == 0 ? m9(0, bu, bv) : (w == 1 ? m9(bu, 0, bv) : m9(bu, bv, 0));
	const double* __restrict__ rho = P.p[0];
	const double* __restrict__ lx = P.p[1];
	const double* __restrict__ ly = P.p[2];
	const double* __restrict__ lz = P.p[3];
	const double* __restrict__ vx = P.p[4];
	const double* __restrict__ vy = P.p[5];
	const double* __restrict__ vz = P.p[6];
	// LDS row of value `val` (0 rho, 1 lx, 2 ly, 3 lz, 4 velocity along a)
	auto vrow = [](uint32_t val, uint32_t a) -> uint32_t { return val == 0 ? 0u : (val == 4 ? 1u + a : val + 3u); };
	// LEN: the out-of-tile rows (side, value 0 rho | 4 the velocity along the
	// side's axis) as the waves enumerate them, side and value wave-uniform.
	// UM = 0: 12 rows, (side, value) interleaved; else the six density rows,
	// then two velocity rows per axis that is not uniform
	constexpr uint32_t ext_rows = UM == 0 ? 12u : 6u + 2u * uint32_t(NV);
	auto ext_side = [](uint32_t row) -> uint32_t {
		if (UM == 0) return row >> 1;
		if (row < 6u) return row;
		const uint32_t k = row - 6u;
		return 2u * ((k >> 1) == 0 ? vel_live_axis(UM, 0) : vel_live_axis(UM, 1)) + (k & 1u);
	};
	auto ext_val = [](uint32_t row) -> uint32_t { return UM == 0 ? 4u * (row & 1u) : (row < 6u ? 0u : 4u); };
	// a register set: a tile being loaded
	struct RegSet {
		double c[7], e[4];
	};
	// a tile record: its first slot, and the raw record words (lanes 0..7)
	// whose neighbor-box starts are read with a wave-uniform readlane (a
	// register array indexed by a run-time side would live in scratch)
	struct RM {
		uint32_t ts, rec;
		__device__ __forceinline__ int32_t nst(uint32_t d) const { return int32_t(word_of(rec, int(1 + d))); }
		__device__ __forceinline__ uint32_t lvl() const { return word_of(rec, 7) & 31u; }
	};
	auto unpack = [&](uint32_t v) { return RM{word_of(v, 0), v}; };
	auto load = [&](const RM& mt, RegSet& r) {
		const uint32_t ts = mt.ts;
		const uint32_t o = (ts + tid) << 3;
		r.c[0] = ldo(rho, o);
		if (!(UM & 1)) r.c[1] = ldo(vx, o);
		if (!(UM & 2)) r.c[2] = ldo(vy, o);
		if (!(UM & 4)) r.c[3] = ldo(vz, o);
		if (!LOWN) {
			r.c[4] = ldo(lx, o); r.c[5] = ldo(ly, o);
			r.c[6] = ldo(lz, o);
		}
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const uint32_t row = w + 8u * uint32_t(i);  // wave-uniform
			r.e[i] = 0;
			// LEN: 12 rows (side, 0 rho | 1 the velocity along the side's axis)
			if (LEN && i >= 2) continue;
			if (row >= (REC ? 24u : (LEN ? ext_rows : 30u))) continue;
			const uint32_t d = REC ? row >> 2 : (LEN ? ext_side(row) : row / 5u);
			const uint32_t val = REC ? row & 3u : (LEN ? ext_val(row) : row - 5u * d), a = d >> 1;
			const int32_t st = mt.nst(d);
			if (st < 0) continue;
			const uint32_t u = lane & 7u, v = lane >> 3, side = (d & 1u) ? 0u : 7u;
			const uint32_t q0 = a == 0 ? side : u, q1 = a == 1 ? side : (a == 0 ? u : v), q2 = a == 2 ? side : v;
			const uint32_t sl = uint32_t(st) + m9(q0, q1, q2);
			if (REC) {
				// rows (side, 0 rho | 1 l_a | 2 area | 3 v_a): the density from
				// its field, the rest from the side's axis record
				r.e[i] = val == 0 ? ldo(rho, sl << 3) : R[size_t(a) * 3 * nrec + 3 * size_t(sl) + (val - 1)];
			} else {
				r.e[i] = ldo(P.p[val == 4 ? 4 + a : val], sl << 3);
			}
		}
	};
	// LEN: a tile's lengths, block-uniform (lt: after the first barrier)
	// (P2: and 1 / (2 l_a), 1 / volume, kept in scalar registers)
	struct TL {
		double v[3], r[3], rv;
	};
	auto lengths = [&](const RM& m) {
		TL tl{{0, 0, 0}, {0, 0, 0}, 0};
		if (LEN) {
			const uint32_t lv = 3u * m.lvl();
			tl.v[0] = lt[lv]; tl.v[1] = lt[lv + 1]; tl.v[2] = lt[lv + 2];
			if (P2) {
#pragma unroll
				for (int a = 0; a < 3; a++) tl.r[a] = uniform_f64(lt[96u + lv + uint32_t(a)]);
				tl.rv = uniform_f64(lt[192u + m.lvl()]);
			}
		}
		return tl;
	};
	// a loaded tile into LDS (after the barrier that ends the previous tile's reads)
	auto stage = [&](const RegSet& r, const TL& tlv) {
		const double (&tl)[3] = tlv.v;
#pragma unroll
		for (int k = 0; k < (UM ? 4 : NROW); k++) {
			if (UM == 0) shd[k][tid] = LOWN && k >= 4 ? tl[k - 4] : r.c[k];
			else if (k == 0 || !((UM >> (k - 1)) & 1)) shd[k == 0 ? 0u : vel_row(UM, uint32_t(k - 1))][tid] = r.c[k];
		}
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const uint32_t row = w + 8u * uint32_t(i);
			if (LEN) {
				if (i < 2 && row < ext_rows) {
					const uint32_t d = ext_side(row), col = 512u + 64u * d + lane;
					if (ext_val(row)) {
						shd[vel_row(UM, d >> 1)][col] = r.e[i];
					} else {
						shd[0][col] = r.e[i];
						if (!LREG) {
							shd[4 % NROW][col] = tl[0]; shd[5 % NROW][col] = tl[1]; shd[6 % NROW][col] = tl[2];
						}
					}
				}
			} else if (REC) {
				if (row < 24u) {
					const uint32_t d = row >> 2, val = row & 3u, a = d >> 1, col = 512u + 64u * d + lane;
					const uint32_t k = val == 0 ? 0u : (val == 1 ? 4u + a : (val == 2 ? nb_area_row(a) : 1u + a));
					shd[k % NROW][col] = r.e[i];
					if (val == 2) shd[nb_one_row(a) % NROW][col] = 1.0;
				}
			} else if (row < 30u) {
				const uint32_t d = row / 5u, val = row - 5u * d;
				shd[vrow(val, d >> 1) % NROW][512u + 64u * d + lane] = r.e[i];
			}
		}
	};
	// column i of LDS row k (LREG: a length row is the tile's length)
	auto lrow = [&](const TL& tl, int k, uint32_t i) -> double {
		return LREG && k >= 4 ? tl.v[k - 4] : shd[k % NROW][i];
	};
	// velocity component a of LDS column i (a uniform component has no row)
	auto vel = [&](uint32_t a, uint32_t i) -> double { return ((UM >> a) & 1) ? uv.v[a] : shd[vel_row(UM, a)][i]; };
	// the staged tile tc from LDS
	auto compute = [&](const RM& mc, const TL& tl) {
		const uint32_t ts = mc.ts;
		const double cd = shd[0][tid], clx = lrow(tl, 4, tid), cly = lrow(tl, 5, tid), clz = lrow(tl, 6, tid);
		const double cva[3] = {vel(0, tid), vel(1, tid), vel(2, tid)};
		// pass 1: the +x, +y, +z face of every cell, once per face, branch-free
		// (a missing face beyond a non-periodic boundary evaluates zeros and
		// is masked by a select)
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const uint32_t li = lp[a];
			const double g = adv_face_g<P2>(a, cd, clx, cly, clz, cva[a],
			                                AdvNb{shd[0][li], lrow(tl, 4, li), lrow(tl, 5, li), lrow(tl, 6, li), vel(a, li)}, dt,
			                                tl.r[a]);
			const bool has = l[a] < 7 || mc.nst(2 * a + 1) >= 0;
			shg[a][tid] = has ? g : 0.0;
		}
		// the tile's -a boundary faces (minus cell outside): 192 faces on
		// waves 0..2, wave-uniform
		if (w < 3 && mc.nst(2 * w) >= 0) {
			const uint32_t k = 512u + 64u * (2u * w) + lane;
			const double sv = UM == 0 ? shd[1 + w][bcell] : (w == 0 ? vel(0, bcell) : (w == 1 ? vel(1, bcell) : vel(2, bcell)));
			const AdvNb self{shd[0][bcell], lrow(tl, 4, bcell), lrow(tl, 5, bcell), lrow(tl, 6, bcell), sv};
			const double kx = lrow(tl, 4, k), ky = lrow(tl, 5, k), kz = lrow(tl, 6, k);
			double gmv;
			if (w == 0) gmv = adv_face_g<P2>(0, shd[0][k], kx, ky, kz, vel(0, k), self, dt, tl.r[0]);
			else if (w == 1) gmv = adv_face_g<P2>(1, shd[0][k], kx, ky, kz, vel(1, k), self, dt, tl.r[1]);
			else gmv = adv_face_g<P2>(2, shd[0][k], kx, ky, kz, vel(2, k), self, dt, tl.r[2]);
			shm[w][lane] = gmv;
		}
		__syncthreads();
		// pass 2: sum in the reference's face order -x, +x, -y, +y, -z, +z
		double acc = 0;
#pragma unroll
		for (int a = 0; a < 3; a++) {
			uint32_t q[3] = {l[0], l[1], l[2]};
			q[a] -= 1;
			double gm = 0;
			if (l[a] > 0) gm = shg[a][m9(q[0] & 7u, q[1] & 7u, q[2] & 7u)];
			else if (mc.nst(2 * a) >= 0) gm = shm[a][fi[a]];
			acc += gm;
			acc += -shg[a][tid];
		}
		st_nt(rho_out, ts + tid, cd + (P2 ? acc * tl.rv : acc / (clx * cly * clz)));
	};
	RegSet ra;
	RM cur = unpack(tile_record_word(meta, t, lane));
	uint32_t tn = tk.next(t);
	load(cur, ra);
	uint32_t rec = tn < t1 ? tile_record_word(meta, tn, lane) : 0u;  // tile tn's record
	for (;;) {
		__syncthreads();  // the previous tile's faces have been read from LDS
		const TL tl = lengths(cur);
		stage(ra, tl);
		__syncthreads();
		const bool more = tn < t1;
		RM nxt = cur;
		if (more) {
			// the next tile's loads fly while this one is computed, then the
			// record of the tile after it
			nxt = unpack(rec);
			load(nxt, ra);
			const uint32_t tnn = tk.next(tn);
			rec = tnn < t1 ? tile_record_word(meta, tnn, lane) : 0u;
		}
		compute(cur, tl);
		if (!more) break;
		cur = nxt;
		tn = tk.next(tn);
	}
}

// Persistent, software-pipelined form of advection_tiles_kernel for any tile
// (the tables of tile_build.hip): the same XCD-contiguous persistent schedule
// as advection_regular_pp_kernel; per tile one 32-B record; while a tile is
// computed from LDS, the next tile's own fields, face rows, ext cells (at
// most two per thread) and finer-face index pairs are in flight into
// registers, so the compute phase issues no global load.
struct TileMeta {
	uint32_t ts, n, e0, ne, fb, nf, pad0, pad1;
};

// Every face is evaluated by each of its two cells (a form that evaluated
// the in-tile same-level faces once, into LDS, lost its paired A/B to the
// extra barrier, profiles/r06i_face_once_ab.txt, and was removed).
//
// LEN (see advection_regular_pp_kernel): an ext cell's three lengths come
// from the per-level table LT (in LDS) by its level byte extl[k], an array
// parallel to ext read coalesced with the ext code; (DCCRGX_LEN_OWN) an own
// cell's by slvl[slot], a coalesced 1-B load instead of three 8-B ones.
// The lengths are not staged (LLVL): LDS keeps the rows rho, vx, vy, vz and
// one level byte per column, and a face takes its neighbor's lengths from
// the table row of that byte (one 1-B LDS read more per neighbor, three 8-B
// rows of T + ecap less; a level bit in the 16-bit face code would save the
// read, but the codes have no spare bit: 0xffff, 0x8000 | k and indices up to
// T + ecap use all of them).  39 KB of LDS at config 3's ecap of 523 instead
// of 62.8 KB and 77 VGPRs: three blocks per CU (DCCRGX_GEN_BLOCKS), as many
// as the runtime reports for the mesh's ecap - two at the capacity of 1024.
// The registers come from two things: the second ext set is gone (the ext
// cells beyond the first T, in few tiles, are loaded at staging), and the
// per-tile addresses are recomputed per tile (`ti`).  The same length bits
// reach the same operands, so the densities are bitwise the fields'.
// DCCRGX_LEN_LDS_GEN=1 or DCCRGX_LEN_OWN=0 keep the seven rows and two blocks.
//
// P2 (see advection_regular_pp_kernel): a face whose neighbor column's level
// byte is the cell's own takes the neighbor's lengths from the own registers
// (the same row, the same bits) and multiplies by the own level's
// 1 / (2 l_a); a face to another level and the four fluxes of a finer face
// divide as before, under a branch a wave skips when none of its lanes has
// one.  The faces are still summed in the order -x .. +z, and the cell
// multiplies by its level's 1 / volume.
template <int MINW, bool REC, bool LEN, int UM = 0, bool P2 = false>
__global__ __launch_bounds__(512, MINW) void advection_tiles_pp_kernel(
    AdvPtrs P, double* __restrict__ rho_out, const uint32_t* __restrict__ tell, uint32_t tplane,
    const uint32_t* __restrict__ ext, const uint32_t* __restrict__ tfine, const TileMeta* __restrict__ meta,
    uint32_t ntiles, uint32_t ecap, double dt, const double* __restrict__ R, size_t nrec,
    const uint8_t* __restrict__ slvl, const uint8_t* __restrict__ extl, const double* __restrict__ LT, AdvUV uv) {
#pragma clang fp contract(off)
	static_assert(!(LEN && REC), "the length table is for the default kernels only");
	constexpr bool LOWN = LEN && DCCRGX_LEN_OWN;
	constexpr bool LLVL = LOWN && !DCCRGX_LEN_LDS_GEN;  // no length rows: a level byte per column
	static_assert(UM == 0 || (LLVL && UM > 0 && UM < 8), "uniform components: the level-row kernel only");
	static_assert(!P2 || LLVL, "reciprocals: the level-row kernel only");
	constexpr uint32_t NLT = P2 ? kLenTabP2 : 96u;
	constexpr uint32_t T = 512;
	// UM (see advection_regular_pp_kernel): a uniform component has no row
	// (the launch still sizes the LDS for four, adv_tiles_lds)
	constexpr uint32_t NROW = LLVL ? 4u - uint32_t(__builtin_popcount(unsigned(UM))) : 7;
	// [NROW][T + ecap] doubles (rho vx vy vz lx ly lz); 2 x T u32 finer-face
	// pairs; LEN: 96 doubles, the per-level lengths (P2: kLenTabP2, with the
	// reciprocals); LLVL: T + ecap level bytes
	// (adv_tiles_lds restates the size)
	extern __shared__ double shd[];
	const uint32_t W = T + ecap;
	uint32_t* shf = reinterpret_cast<uint32_t*>(shd + NROW * W);
	double* lt = reinterpret_cast<double*>(shf + 2 * T);  // (LEN)
	uint8_t* shl = reinterpret_cast<uint8_t*>(lt + NLT);  // (LLVL)
	const StaticTiles tk(ntiles);
	const uint32_t t1 = tk.t1;
	uint32_t t = tk.first();
	if (t >= t1) return;  // block-uniform
	const uint32_t tid = threadIdx.x;
	// the thread index the per-tile addresses are formed from.  LLVL: made
	// opaque once per tile, so that the LDS and global addresses derived from
	// it are recomputed (a few adds) and not held in registers across the
	// loop: they are the registers between this kernel and 80
	uint32_t ti = tid;
	const double* const rho = P.p[0];
	const double* const lx = P.p[1];
	const double* const ly = P.p[2];
	const double* const lz = P.p[3];
	const double* const vx = P.p[4];
	const double* const vy = P.p[5];
	const double* const vz = P.p[6];
	// the register set of the tile being loaded (field order rho vx vy vz lx ly lz)
	// (LLVL: entries 0..3 only, and no second ext set: the ext cells beyond
	// the first T, in few tiles, are loaded at staging)
	double c[7], xa[7], xb[7];
	uint32_t row[3], fq[2];
	uint32_t lvc = 0, lva = 0, lvb = 0;  // LEN: the level bytes of c, xa, xb
	if (LEN && tid < NLT) lt[tid] = LT[tid];  // (read after the first tile's first barrier)
	auto load7 = [&](uint32_t slot, double (&v)[7]) {
		const uint32_t o = slot << 3;
		v[0] = ldo(rho, o);
		if (!(UM & 1)) v[1] = ldo(vx, o);
		if (!(UM & 2)) v[2] = ldo(vy, o);
		if (!(UM & 4)) v[3] = ldo(vz, o);
		if (LOWN) {
			lvc = __builtin_nontemporal_load(slvl + slot);
			return;
		}
		v[4] = ldo(lx, o); v[5] = ldo(ly, o); v[6] = ldo(lz, o);
	};
	// a cell's lengths from the table by its level byte (at staging time)
	auto lengths = [&](uint32_t lv, double (&v)[7]) {
		const uint32_t k = 3u * (lv & 31u);
		v[4] = lt[k]; v[5] = lt[k + 1]; v[6] = lt[k + 2];
	};
	// ext = slot | axis mask << 29: density and lengths, and only the
	// velocity components along the axes its faces cross
	auto load5 = [&](uint32_t q, double (&v)[7]) {
		const uint32_t sl = q & 0x1fffffffu, o = sl << 3, ax = q >> 29;
		v[0] = ldo(rho, o);
		if (LEN) {
			if (!(UM & 1)) v[1] = (ax & 1u) ? ldo(vx, o) : 0.0;
			if (!(UM & 2)) v[2] = (ax & 2u) ? ldo(vy, o) : 0.0;
			if (!(UM & 4)) v[3] = (ax & 4u) ? ldo(vz, o) : 0.0;
			return;
		}
		if (REC && (ax == 1u || ax == 2u || ax == 4u)) {
			// reached through faces of one axis (all but ~0.3 % on config 3):
			// its density and that axis' record, staged in the rows of
			// nb_area_row / nb_one_row (bitwise the same fluxes)
			const uint32_t a = ax >> 1;
			const double* r = R + size_t(a) * 3 * nrec + 3 * size_t(sl);
			const double la = r[0], ar = r[1], vv = r[2];
			v[4] = a == 0 ? la : ar;
			v[5] = a == 0 ? ar : (a == 1 ? la : 1.0);
			v[6] = a == 2 ? la : 1.0;
			v[1] = a == 0 ? vv : 0.0;
			v[2] = a == 1 ? vv : 0.0;
			v[3] = a == 2 ? vv : 0.0;
			return;
		}
		v[4] = ldo(lx, o); v[5] = ldo(ly, o); v[6] = ldo(lz, o);
		v[1] = (ax & 1u) ? ldo(vx, o) : 0.0;
		v[2] = (ax & 2u) ? ldo(vy, o) : 0.0;
		v[3] = (ax & 4u) ? ldo(vz, o) : 0.0;
	};
	const uint32_t lane = tid & 63u;
	struct GM {
		uint32_t ts, n, e0, ne, fb, nf;
	};
	auto unpack = [&](uint32_t v) { return GM{word_of(v, 0), word_of(v, 1), word_of(v, 2), word_of(v, 3), word_of(v, 4),
	                                          word_of(v, 5)}; };
	auto load = [&](const GM& mt) {
		const uint32_t ts = mt.ts, n = mt.n, e0 = mt.e0, ne = mt.ne, fb = mt.fb, nf = mt.nf;
		if (tid < n) {
			load7(ts + ti, c);
			// the tile's face codes, ext list and finer pairs are read once per
			// sweep: non-temporal, so they do not evict the field lines other
			// tiles re-read (paired A/B on config 3: 0.1915 -> 0.1865 ms/sweep)
			// (three planes of codes: one coalesced 4-B load per plane; the
			// interleaved 12-B records cost ~20 us per sweep on config 3)
			row[0] = __builtin_nontemporal_load(tell + (ts + ti));
			row[1] = __builtin_nontemporal_load(tell + tplane + (ts + ti));
			row[2] = __builtin_nontemporal_load(tell + 2 * tplane + (ts + ti));
		}
		if (tid < ne) {
			load5(__builtin_nontemporal_load(ext + e0 + ti), xa);
			if (LEN) lva = __builtin_nontemporal_load(extl + e0 + ti);
		}
		if (!LLVL && tid + T < ne) {
			load5(__builtin_nontemporal_load(ext + e0 + tid + T), xb);
			if (LEN) lvb = __builtin_nontemporal_load(extl + e0 + tid + T);
		}
		if (tid < nf) {
			typedef unsigned int u2v __attribute__((ext_vector_type(2)));
			const u2v q = __builtin_nontemporal_load(reinterpret_cast<const u2v*>(tfine) + (fb + ti));
			fq[0] = q.x;
			fq[1] = q.y;
		}
	};
	// UM: a register set into LDS column col, the density and the live components
	auto stage = [&](uint32_t col, const double (&v)[7]) {
		shd[col] = v[0];
#pragma unroll
		for (uint32_t a = 0; a < 3; a++)
			if (!((UM >> a) & 1)) shd[vel_row(UM, a) * W + col] = v[1 + a];
	};
	GM cur = unpack(tile_record_word(meta, t, lane));
	uint32_t tn = tk.next(t);
	load(cur);
	uint32_t rec = tn < t1 ? tile_record_word(meta, tn, lane) : 0u;  // tile tn's record
	for (;;) {
		const uint32_t n = cur.n, ne = cur.ne, nf = cur.nf, ts = cur.ts;
		if (LLVL) asm volatile("" : "+v"(ti));
		__syncthreads();  // the previous tile's faces have been read from LDS
		if (tid < n) {
			if (LOWN && !LLVL) lengths(lvc, c);
			if (UM) {
				stage(ti, c);
			} else {
#pragma unroll
				for (uint32_t k = 0; k < NROW; k++) shd[k * W + ti] = c[k];
			}
			if (LLVL) shl[ti] = uint8_t(lvc);
		}
		if (tid < ne) {
			if (LEN && !LLVL) lengths(lva, xa);
			if (UM) {
				stage(T + ti, xa);
			} else {
#pragma unroll
				for (uint32_t k = 0; k < NROW; k++) shd[k * W + T + ti] = xa[k];
			}
			if (LLVL) shl[T + ti] = uint8_t(lva);
		}
		if (tid + T < ne) {
			if (LLVL) {
				load5(__builtin_nontemporal_load(ext + cur.e0 + ti + T), xb);
				lvb = __builtin_nontemporal_load(extl + cur.e0 + ti + T);
				shl[2 * T + ti] = uint8_t(lvb);
			} else if (LEN) {
				lengths(lvb, xb);
			}
			if (UM) {
				stage(2 * T + ti, xb);
			} else {
#pragma unroll
				for (uint32_t k = 0; k < NROW; k++) shd[k * W + 2 * T + ti] = xb[k];
			}
		}
		if (tid < nf) {
			shf[2 * ti] = fq[0];
			shf[2 * ti + 1] = fq[1];
		}
		const uint32_t r0 = row[0], r1 = row[1], r2 = row[2];
		__syncthreads();
		const bool more = tn < t1;
		GM nxt = cur;
		if (more) {
			// the next tile's loads fly while this one is computed, then the
			// record of the tile after it
			nxt = unpack(rec);
			load(nxt);
			const uint32_t tnn = tk.next(tn);
			rec = tnn < t1 ? tile_record_word(meta, tnn, lane) : 0u;
		}
		const bool own = tid < n;
		double cd = 0, cvx = 0, cvy = 0, cvz = 0, clx = 1, cly = 1, clz = 1;
		uint32_t olv = 0;  // P2: the own level
		if (own) {
			cd = shd[ti];
			cvx = (UM & 1) ? uv.v[0] : shd[vel_row(UM, 0) * W + ti];
			cvy = (UM & 2) ? uv.v[1] : shd[vel_row(UM, 1) * W + ti];
			cvz = (UM & 4) ? uv.v[2] : shd[vel_row(UM, 2) * W + ti];
			if (LLVL) {
				// own lengths: the table row of the cell's level byte, kept in
				// registers across the compute phase
				olv = uint32_t(shl[ti]) & 31u;
				const uint32_t k = 3u * olv;
				clx = lt[k]; cly = lt[k + 1]; clz = lt[k + 2];
			} else {
				clx = shd[(4 % NROW) * W + ti];
				cly = shd[(5 % NROW) * W + ti];
				clz = shd[(6 % NROW) * W + ti];
			}
		}
		auto fetch = [&](uint32_t li, int d) -> AdvNb {
			if (LLVL) {
				// a neighbor's lengths: the table row of its column's level byte
				const uint32_t k = 3u * (uint32_t(shl[li]) & 31u);
				const uint32_t a = uint32_t(d >> 1);
				return AdvNb{shd[li], lt[k], lt[k + 1], lt[k + 2], ((UM >> a) & 1) ? uv.v[a] : shd[vel_row(UM, a) * W + li]};
			}
			return AdvNb{shd[li], shd[(4 % NROW) * W + li], shd[(5 % NROW) * W + li], shd[(6 % NROW) * W + li],
			             shd[(1 + (d >> 1)) * W + li]};
		};
		const uint32_t rr[3] = {r0, r1, r2};
		if (own) {
			double acc = 0;
#pragma unroll
			for (int d = 0; d < 6; d++) {
				const uint32_t code = (rr[d >> 1] >> (16 * (d & 1))) & 0xffffu;
				if (code == 0xffffu) continue;
				if (P2 && !(code & 0x8000u) && (uint32_t(shl[code]) & 31u) == olv) {
					// a same-level neighbor: its lengths are the own ones
					const uint32_t a = uint32_t(d >> 1);
					const double nv = ((UM >> a) & 1) ? uv.v[a] : shd[vel_row(UM, a) * W + code];
					const double ri = lt[96u + 3u * olv + a];
					if (a == 0) acc += adv_face_flux_same(d, cd, clx, cly, clz, cvx, shd[code], nv, ri, dt);
					else if (a == 1) acc += adv_face_flux_same(d, cd, cly, clx, clz, cvy, shd[code], nv, ri, dt);
					else acc += adv_face_flux_same(d, cd, clz, clx, cly, cvz, shd[code], nv, ri, dt);
				} else if (code & 0x8000u) {
					const uint32_t fk = code & 0x7fffu;
					const uint32_t q0 = shf[2 * fk], q1 = shf[2 * fk + 1];
					const uint32_t li[4] = {q0 & 0xffffu, q0 >> 16, q1 & 0xffffu, q1 >> 16};
#pragma unroll
					for (int k = 0; k < 4; k++)
						acc += adv_face_flux_d(d, cd, clx, cly, clz, cvx, cvy, cvz, fetch(li[k], d), dt);
				} else {
					acc += adv_face_flux_d(d, cd, clx, cly, clz, cvx, cvy, cvz, fetch(code, d), dt);
				}
			}
			st_nt(rho_out, ts + ti, cd + (P2 ? acc * lt[192u + olv] : acc / (clx * cly * clz)));
		}
		if (!more) break;
		cur = nxt;
		tn = tk.next(tn);
	}
}

}  // namespace

// ===========================================================================
static void k_advection(const double* const f[7], double* rho_out, const uint32_t* face_ptr, const int32_t* face_ent,
                        size_t s0, size_t s1, double dt, hipStream_t s) {
	// the untiled gather over the face CSR: runs whose tiles exceed the
	// pipelined tile kernel's capacities
	if (s1 <= s0) return;
	advection_kernel<<<grid_for(s1 - s0, 256, 256u * 64u), 256, 0, s>>>(f[0], f[1], f[2], f[3], f[4], f[5], f[6],
	                                                                    rho_out, face_ptr, face_ent, s0, s1, dt);
	HIP_CHECK(hipGetLastError());
}

// the face-table sweep of slots [s0, s1); bands: their bands as well
void k_advection_ell(const double* const f[7], double* rho_out, const int32_t* ell, const int32_t* fine, size_t s0,
                     size_t s1, double dt, hipStream_t s, const BandArgs* bands) {
	if (s1 <= s0) return;
	if (bands)
		advection_ell_lds_kernel<true><<<grid_for(s1 - s0, 256, 256u * 64u), 256, 0, s>>>(
		    f[0], f[1], f[2], f[3], f[4], f[5], f[6], rho_out, ell, fine, s0, s1, dt, *bands);
	else
		advection_ell_lds_kernel<false><<<grid_for(s1 - s0, 256, 256u * 64u), 256, 0, s>>>(
		    f[0], f[1], f[2], f[3], f[4], f[5], f[6], rho_out, ell, fine, s0, s1, dt, BandArgs{});
	HIP_CHECK(hipGetLastError());
}

// The two persistent kernels of k_advection_tiles and how they are launched.
// The length-table kernels are compiled for DCCRGX_REG_BLOCKS /
// DCCRGX_GEN_BLOCKS blocks per CU; the grid is sized by the blocks per CU the
// runtime reports for the kernel and its LDS (registers, LDS and a large
// ecap all enter there), never by a constant.  Should more blocks fit than
// the kernel is compiled for (an A/B build with fewer), its dynamic LDS is
// grown until they do not: a persistent grid smaller than the machine's
// capacity would otherwise be spread unevenly over the CUs.
constexpr int kRegWaves = 2 * DCCRGX_REG_BLOCKS, kGenWaves = 2 * DCCRGX_GEN_BLOCKS;
constexpr bool kLvlRow = DCCRGX_LEN_OWN && !DCCRGX_LEN_LDS_GEN;

// dynamic LDS of advection_tiles_pp_kernel (restates the kernel's layout)
static size_t adv_tiles_lds(uint32_t ecap, bool len, bool pow2) {
	const size_t W = size_t(512) + ecap;
	const bool lvl_row = len && kLvlRow;
	return (lvl_row ? 4 : 7) * W * sizeof(double) + size_t(2) * 512 * sizeof(uint32_t) +
	       (len ? (pow2 ? kLenTabP2 : 96) * sizeof(double) : 0) + (lvl_row ? (W + 7) / 8 * 8 : 0);
}

// The length-table kernels' instantiation for the mask of uniform velocity
// components (ensure_vel_uniform): f(std::integral_constant<int, UM>)
template <class F>
static auto with_vel_mask(int um, F&& f) {
	switch (um & 7) {
		case 1: return f(std::integral_constant<int, 1>{});
		case 2: return f(std::integral_constant<int, 2>{});
		case 3: return f(std::integral_constant<int, 3>{});
		case 4: return f(std::integral_constant<int, 4>{});
		case 5: return f(std::integral_constant<int, 5>{});
		case 6: return f(std::integral_constant<int, 6>{});
		case 7: return f(std::integral_constant<int, 7>{});
		default: return f(std::integral_constant<int, 0>{});
	}
}
// From the plan to the kernel, once per kind.  All instantiations of a
// template share their parameter list (an instantiation ignores the pointers
// it has no use for), so the occupancy query of adv_sweep_launch and the
// launch of k_advection_tiles go through one typed pointer.
using RegKernel = void (*)(AdvPtrs, double*, const RegTileMeta*, uint32_t, double, const double*, size_t, const double*,
                           AdvUV);
using GenKernel = void (*)(AdvPtrs, double*, const uint32_t*, uint32_t, const uint32_t*, const uint32_t*, const TileMeta*,
                           uint32_t, uint32_t, double, const double*, size_t, const uint8_t*, const uint8_t*,
                           const double*, AdvUV);

static RegKernel adv_regular_kernel(const AdvSweepPlan& p) {
	if (p.rec) return advection_regular_pp_kernel<4, true, false>;
	if (p.len)
		return with_vel_mask(p.um[0], [&](auto M) -> RegKernel {
			constexpr int um = kRegMasks ? decltype(M)::value : 0;
			return p.pow2 ? advection_regular_pp_kernel<kRegWaves, false, true, um, kRegMasks>
			              : advection_regular_pp_kernel<kRegWaves, false, true, um>;
		});
	return advection_regular_pp_kernel<4, false, false>;
}

static GenKernel adv_general_kernel(const AdvSweepPlan& p) {
	if (p.rec) return advection_tiles_pp_kernel<4, true, false>;
	if (p.len)
		return with_vel_mask(p.um[1], [&](auto M) -> GenKernel {
			constexpr int um = kGenMasks ? decltype(M)::value : 0;
			// the dividing kernels of the masks with vy or vz uniform come out
			// at seven waves per SIMD in the three-block build; left to the
			// bound of six the reciprocal ones take 73-77 registers, so they
			// are compiled for seven (no scratch) and none has fewer waves
			// than the dividing kernel of its mask
			constexpr int w = kGenWaves + (kGenWaves == 6 && um >= 2 ? 1 : 0);
			return p.pow2 ? advection_tiles_pp_kernel<w, false, true, um, kGenMasks>
			              : advection_tiles_pp_kernel<kGenWaves, false, true, um>;
		});
	return advection_tiles_pp_kernel<4, false, false>;
}

const Grid::SweepLaunch& adv_sweep_launch(Grid& g, int kind, const AdvSweepPlan& plan) {
	void* fn;  // (SweepLaunch::fn: the typed pointer is taken back from it for the launch)
	size_t lds_min = 0;
	int cap = 2;
	bool table;  // a length-table kernel (the others keep their fixed two blocks per CU)
	if (kind == 0) {
		fn = reinterpret_cast<void*>(adv_regular_kernel(plan));
		table = plan.len != nullptr;
		if (table) cap = DCCRGX_REG_BLOCKS;
	} else {
		fn = reinterpret_cast<void*>(adv_general_kernel(plan));
		table = plan.len != nullptr;
		lds_min = adv_tiles_lds(uint32_t(g.max_ext), table, table && plan.pow2);
		if (table) cap = DCCRGX_GEN_BLOCKS;
	}
	Grid::SweepLaunch& L = g.adv_launch[kind];
	if (L.fn == fn && L.lds_min == lds_min && L.blocks_per_cu > 0) return L;
	int k = 2;
	size_t lds = lds_min;
	if (table) {
		HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&k, fn, 512, lds));
		if (k > cap) {
			hipFuncAttributes fa;
			HIP_CHECK(hipFuncGetAttributes(&fa, fn));
			int dev = 0, cu_lds = 0;
			HIP_CHECK(hipGetDevice(&dev));
			HIP_CHECK(hipDeviceGetAttribute(&cu_lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev));
			// just over a (cap + 1)-th of the CU's LDS per block
			const size_t per = (size_t(cu_lds) / size_t(cap + 1) + 512) / 512 * 512;
			if (per > fa.sharedSizeBytes + lds) lds = per - fa.sharedSizeBytes;
			HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&k, fn, 512, lds));
		}
		DX_REQUIRE(k >= 1, "the tile sweep kernel does not fit a CU");
	}
	L.fn = fn;
	L.lds_min = lds_min;
	L.lds = lds;
	L.blocks_per_cu = k;
	return L;
}

// Tiled advection sweep of one run (0 inner, 1 outer): the regular tiles with
// advection_regular_pp_kernel, every other tile with advection_tiles_pp_kernel,
// both persistent: the field-reading and the record kernels with two blocks
// per CU (r01k: one / two tiles in flight per block, dynamic tickets and a
// second stream for the general sweep all tie or lose against this schedule),
// the length-table kernels with the blocks per CU the runtime reports for
// them, three on config 3 (adv_sweep_launch).
void k_advection_tiles(const double* const f[7], double* rho_out, Grid& g, int run, double dt, hipStream_t s,
                       const AdvSweepPlan& plan) {
	const size_t n_reg = g.tcount[run], n_irr = g.tcount[2 + run];
	const AdvUV uv{{plan.uv[0], plan.uv[1], plan.uv[2]}};
	const AdvPtrs P{{f[0], f[4], f[5], f[6], f[1], f[2], f[3]}};
	if (n_irr && !g.tmeta.n) {
		// a tile beyond the pipelined kernel's capacities: the whole run untiled
		const size_t s0 = run == 0 ? 0 : g.n_inner, s1 = run == 0 ? g.n_inner : g.n_local;
		k_advection(f, rho_out, g.face_ptr.p, g.face_ent.p, s0, s1, dt, s);
		return;
	}
	if (n_reg) {
		const RegTileMeta* meta = g.tregmeta.p + (run == 0 ? 0 : g.tcount[0]);
		const Grid::SweepLaunch& L = adv_sweep_launch(g, 0, plan);
		const unsigned nblk = unsigned(std::min<size_t>(size_t(256) * L.blocks_per_cu, (n_reg + 7) / 8 * 8));
		reinterpret_cast<RegKernel>(L.fn)<<<nblk, 512, L.lds, s>>>(P, rho_out, meta, uint32_t(n_reg), dt, plan.rec, g.n_slots,
		                                                        plan.len, uv);
		HIP_CHECK(hipGetLastError());
	}
	if (n_irr) {
		const TileMeta* meta = reinterpret_cast<const TileMeta*>(g.tmeta.p) + (run == 0 ? 0 : g.tcount[2]);
		const uint32_t ecap = uint32_t(g.max_ext);
		const Grid::SweepLaunch& L = adv_sweep_launch(g, 1, plan);
		const unsigned nblk = unsigned(std::min<size_t>(size_t(256) * L.blocks_per_cu, (n_irr + 7) / 8 * 8));
		reinterpret_cast<GenKernel>(L.fn)<<<nblk, 512, L.lds, s>>>(
		    P, rho_out, g.tell.p, uint32_t(g.n_local + 1), g.ext_pk.p, g.tfine.p, meta, uint32_t(n_irr), ecap, dt, plan.rec,
		    g.n_slots, g.slot_lvl.p, g.ext_lvl.p, plan.len, uv);
		HIP_CHECK(hipGetLastError());
	}
}

// ensure_len_table's check: flag = 1 when a slot's three lengths are not
// bitwise its level's row of the table
__global__ void len_check_kernel(const double* __restrict__ lx, const double* __restrict__ ly,
                                 const double* __restrict__ lz, const uint8_t* __restrict__ lvl, size_t n,
                                 const double* __restrict__ tab, int* __restrict__ flag) {
	bool bad = false;
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x) {
		const double* r = tab + 3u * (lvl[s] & 31u);
		bad |= __double_as_longlong(lx[s]) != __double_as_longlong(r[0]) ||
		       __double_as_longlong(ly[s]) != __double_as_longlong(r[1]) ||
		       __double_as_longlong(lz[s]) != __double_as_longlong(r[2]);
	}
	if (bad) atomicOr(flag, 1);
}

void k_len_check(const double* const f[7], const uint8_t* slot_lvl, size_t n, const double* tab, int* flag,
                 hipStream_t s) {
	HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), s));
	if (!n) return;
	len_check_kernel<<<grid_for(n, 256, 256u * 16u), 256, 0, s>>>(f[4], f[5], f[6], slot_lvl, n, tab, flag);
	HIP_CHECK(hipGetLastError());
}

// ensure_vel_uniform's check: out[0] bit a = 1 when some slot's velocity
// component a is not the 64-bit pattern of slot 0; out[1 + a] that pattern
__global__ void vel_check_kernel(const uint64_t* __restrict__ vx, const uint64_t* __restrict__ vy,
                                 const uint64_t* __restrict__ vz, size_t n, uint64_t* __restrict__ out) {
	const uint64_t x0 = vx[0], y0 = vy[0], z0 = vz[0];
	unsigned diff = 0;
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x)
		diff |= (vx[s] != x0 ? 1u : 0u) | (vy[s] != y0 ? 2u : 0u) | (vz[s] != z0 ? 4u : 0u);
	if (diff) atomicOr(reinterpret_cast<unsigned long long*>(out), (unsigned long long)diff);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		out[1] = x0;
		out[2] = y0;
		out[3] = z0;
	}
}

void k_vel_check(const double* const f[7], size_t n, uint64_t* out, hipStream_t s) {
	HIP_CHECK(hipMemsetAsync(out, 0, 4 * sizeof(uint64_t), s));
	if (!n) return;
	vel_check_kernel<<<grid_for(n, 256, 256u * 16u), 256, 0, s>>>(
	    reinterpret_cast<const uint64_t*>(f[1]), reinterpret_cast<const uint64_t*>(f[2]),
	    reinterpret_cast<const uint64_t*>(f[3]), n, out);
	HIP_CHECK(hipGetLastError());
}

// the out-of-tile neighbor entries of the general tiles (ntiles records of
// 8 x u32: word 2 the first entry, word 3 their count) by axis-bit pattern:
// cnt[ax] entries of ext_pk hold the bits ax
__global__ __launch_bounds__(256) void ext_axis_count_kernel(const uint32_t* __restrict__ tmeta, size_t ntiles,
                                                             const uint32_t* __restrict__ ext_pk,
                                                             unsigned long long* __restrict__ cnt) {
	__shared__ unsigned sh[8];
	if (threadIdx.x < 8) sh[threadIdx.x] = 0;
	__syncthreads();
	for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const uint32_t e0 = tmeta[8 * t + 2], ne = tmeta[8 * t + 3];
		for (uint32_t k = threadIdx.x; k < ne; k += blockDim.x) atomicAdd(&sh[ext_pk[e0 + k] >> 29], 1u);
	}
	__syncthreads();
	if (threadIdx.x < 8 && sh[threadIdx.x]) atomicAdd(cnt + threadIdx.x, (unsigned long long)sh[threadIdx.x]);
}

void k_ext_axis_count(const uint32_t* tmeta, size_t ntiles, const uint32_t* ext_pk, uint64_t* cnt, hipStream_t s) {
	HIP_CHECK(hipMemsetAsync(cnt, 0, 8 * sizeof(uint64_t), s));
	if (!ntiles) return;
	ext_axis_count_kernel<<<unsigned(std::min<size_t>(ntiles, 1024)), 256, 0, s>>>(
	    tmeta, ntiles, ext_pk, reinterpret_cast<unsigned long long*>(cnt));
	HIP_CHECK(hipGetLastError());
}

void k_nbrec(const double* const f[7], size_t n, double* r, hipStream_t s) {
	launch_per_item(nbrec_kernel, n, s, f[4], f[5], f[6], f[1], f[2], f[3], n, r);
}


}  // namespace dccrgx
