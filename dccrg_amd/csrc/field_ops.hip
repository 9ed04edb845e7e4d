// Operators on fp64 cell fields, kernels and drivers together: gradient, curl
// and divergence over the face table (one stencil, dccrgx_stencil.hpp), axpy,
// and the field reductions (dccrgx_reduce.hpp; the second stage also folds the
// particle reductions of particles.hip).  Bandwidth-bound; no MFMA.  Per-cell
// arithmetic is written expression by expression with contraction off.
#include <algorithm>

#include "dccrgx_grid.hpp"
#include "dccrgx_reduce.hpp"
#include "dccrgx_stencil.hpp"

namespace dccrgx {

namespace {

// the first-derivative stencil over the face table (face_row, face_value,
// face_level, stencil_lengths, stencil_dim, stencil_derivative): dccrgx_stencil.hpp

// dccrgx_gradient (dccrgx.h): the cell-centred gradient of `in` over the
// unfiltered face table for the local slots [s0, s1), the first-derivative
// counterpart of set_scaling_factor's second derivative: the same centre
// distances (own half length + the neighbor's), the same three-point stencil
// per dimension.  The Poisson classification is not consulted.
// A neighbor's length along the face's dimension needs its level only
// (slot_lvl, one byte per slot, made with the face table): neighbors differ by
// at most one level, the four finer cells of a face are one level up, and
// under a stretched geometry the neighbor's level-0 cell along d follows from
// this cell's own indices (the index just past its upper face or just below
// its lower one, wrapped), so no neighbor id is decoded.
template <bool STRETCHED>
__global__ __launch_bounds__(BS) void gradient_kernel(MapCtx m, double l0x, double l0y, double l0z, StretchedView G,
                                                      const uint64_t* __restrict__ slot_ids,
                                                      const uint8_t* __restrict__ slot_lvl,
                                                      const int32_t* __restrict__ face_ell,
                                                      const int32_t* __restrict__ face_fine,
                                                      const double* __restrict__ in, double* __restrict__ ox,
                                                      double* __restrict__ oy, double* __restrict__ oz, double scale,
                                                      size_t s0, size_t s1) {
#pragma clang fp contract(off)
	const size_t s = s0 + size_t(xcd_block()) * BS + threadIdx.x;
	if (s >= s1) return;
	int32_t ev[6];
	face_row(face_ell, s, ev);
	const int lvl = slot_lvl[s] & 31;
	const double vc = in[s];
	// the six neighbor values and levels, gathered before the ordered arithmetic
	double v[6];
	int nl[6];
#pragma unroll
	for (int dir = 0; dir < 6; dir++) {
		v[dir] = face_value(in, face_fine, ev[dir]);
		nl[dir] = face_level(slot_lvl, ev[dir], lvl);
	}
	double lc[3], ln[6];
	stencil_lengths<STRETCHED>(m, l0x, l0y, l0z, G, slot_ids, s, lvl, nl, lc, ln);
	double* const out[3] = {ox, oy, oz};
#pragma unroll
	for (int d = 0; d < 3; d++) {
		if (!out[d]) continue;
		const StencilDim k = stencil_dim(lc[d], ln[2 * d], ln[2 * d + 1], ev[2 * d], ev[2 * d + 1]);
		out[d][s] = scale * stencil_derivative(k, v[2 * d], vc, v[2 * d + 1]);
	}
}

// dccrgx_curl / dccrgx_divergence (dccrgx.h) of the three fields f0, f1, f2 for
// the local slots [s0, s1).  The face row, the seven levels, the lengths and
// the three dimensions' coefficients are formed once per cell and serve all
// three fields.  The field pointers are kernel arguments and every array of
// them is indexed by unrolled constants only, so they stay in SGPRs.
// The value of field j across the faces of dimension d is wanted by the curl
// component 3 - j - d alone (d != j): 12 gathered values when all three
// components are wanted; the divergence takes the 6 with d == j.
template <bool STRETCHED, bool ACCUMULATE>
__global__ __launch_bounds__(BS) void curl_kernel(MapCtx m, double l0x, double l0y, double l0z, StretchedView G,
                                                  const uint64_t* __restrict__ slot_ids,
                                                  const uint8_t* __restrict__ slot_lvl,
                                                  const int32_t* __restrict__ face_ell,
                                                  const int32_t* __restrict__ face_fine, const double* f0,
                                                  const double* f1, const double* f2, double* ox, double* oy,
                                                  double* oz, double scale, size_t s0, size_t s1) {
#pragma clang fp contract(off)
	const size_t s = s0 + size_t(xcd_block()) * BS + threadIdx.x;
	if (s >= s1) return;
	int32_t ev[6];
	face_row(face_ell, s, ev);
	const int lvl = slot_lvl[s] & 31;
	const double* const F[3] = {f0, f1, f2};
	double* const out[3] = {ox, oy, oz};
	// the gathers first: the levels, then per wanted component its four values
	int nl[6];
#pragma unroll
	for (int dir = 0; dir < 6; dir++) nl[dir] = face_level(slot_lvl, ev[dir], lvl);
	double vc[3], v[3][6], prev[3] = {0.0, 0.0, 0.0};
#pragma unroll
	for (int j = 0; j < 3; j++) {
		vc[j] = F[j][s];
		if constexpr (ACCUMULATE)
			if (out[j]) prev[j] = out[j][s];
#pragma unroll
		for (int d = 0; d < 3; d++) {
			if (d == j) continue;
			if (!out[3 - j - d]) continue;
			v[j][2 * d] = face_value(F[j], face_fine, ev[2 * d]);
			v[j][2 * d + 1] = face_value(F[j], face_fine, ev[2 * d + 1]);
		}
	}
	double lc[3], ln[6];
	stencil_lengths<STRETCHED>(m, l0x, l0y, l0z, G, slot_ids, s, lvl, nl, lc, ln);
	StencilDim k[3];
#pragma unroll
	for (int d = 0; d < 3; d++) k[d] = stencil_dim(lc[d], ln[2 * d], ln[2 * d + 1], ev[2 * d], ev[2 * d + 1]);
#pragma unroll
	for (int c = 0; c < 3; c++) {
		if (!out[c]) continue;
		constexpr int nxt[3] = {1, 2, 0};
		const int d1 = nxt[c], d2 = nxt[d1];  // r_c = D_d1(F_d2) - D_d2(F_d1)
		const double p = stencil_derivative(k[d1], v[d2][2 * d1], vc[d2], v[d2][2 * d1 + 1]);
		const double q = stencil_derivative(k[d2], v[d1][2 * d2], vc[d1], v[d1][2 * d2 + 1]);
		const double r = p - q;
		const double t = scale * r;
		if constexpr (ACCUMULATE) out[c][s] = prev[c] + t;
		else out[c][s] = t;
	}
}

template <bool STRETCHED, bool ACCUMULATE>
__global__ __launch_bounds__(BS) void divergence_kernel(MapCtx m, double l0x, double l0y, double l0z, StretchedView G,
                                                        const uint64_t* __restrict__ slot_ids,
                                                        const uint8_t* __restrict__ slot_lvl,
                                                        const int32_t* __restrict__ face_ell,
                                                        const int32_t* __restrict__ face_fine, const double* f0,
                                                        const double* f1, const double* f2, double* out, double scale,
                                                        size_t s0, size_t s1) {
#pragma clang fp contract(off)
	const size_t s = s0 + size_t(xcd_block()) * BS + threadIdx.x;
	if (s >= s1) return;
	int32_t ev[6];
	face_row(face_ell, s, ev);
	const int lvl = slot_lvl[s] & 31;
	const double* const F[3] = {f0, f1, f2};
	int nl[6];
	double vc[3], v[6];
#pragma unroll
	for (int d = 0; d < 3; d++) {
		nl[2 * d] = face_level(slot_lvl, ev[2 * d], lvl);
		nl[2 * d + 1] = face_level(slot_lvl, ev[2 * d + 1], lvl);
		vc[d] = F[d][s];
		v[2 * d] = face_value(F[d], face_fine, ev[2 * d]);
		v[2 * d + 1] = face_value(F[d], face_fine, ev[2 * d + 1]);
	}
	double lc[3], ln[6];
	stencil_lengths<STRETCHED>(m, l0x, l0y, l0z, G, slot_ids, s, lvl, nl, lc, ln);
	double D[3];
#pragma unroll
	for (int d = 0; d < 3; d++) {
		const StencilDim k = stencil_dim(lc[d], ln[2 * d], ln[2 * d + 1], ev[2 * d], ev[2 * d + 1]);
		D[d] = stencil_derivative(k, v[2 * d], vc[d], v[2 * d + 1]);
	}
	const double r = (D[0] + D[1]) + D[2];
	const double t = scale * r;
	if constexpr (ACCUMULATE) out[s] = out[s] + t;
	else out[s] = t;
}

// dccrgx_field_axpy: y = y + (a * x) over the slots [s0, s1), the product
// rounded before the sum.  A field's array starts 256-byte aligned (DBuf), so
// pairs from the first even slot on go as 16-byte loads and stores, a leading
// odd slot and a trailing single one on their own.
__global__ __launch_bounds__(BS) void field_axpy_kernel(double* __restrict__ y, const double* __restrict__ x, double a,
                                                        size_t s0, size_t s1) {
#pragma clang fp contract(off)
	const size_t t = size_t(blockIdx.x) * BS + threadIdx.x;
	const size_t b = (s0 + 1) & ~size_t(1);
	const size_t i = b + 2 * t;
	if (i + 1 < s1) {
		double2 yv = *reinterpret_cast<const double2*>(y + i);
		const double2 xv = *reinterpret_cast<const double2*>(x + i);
		const double p0 = a * xv.x, p1 = a * xv.y;
		yv.x = yv.x + p0;
		yv.y = yv.y + p1;
		*reinterpret_cast<double2*>(y + i) = yv;
	} else if (i < s1) {
		const double p = a * x[i];
		y[i] = y[i] + p;
	}
	if (t == 0 && b != s0) {  // (s0 < s1: the launcher starts nothing for an empty range)
		const double p = a * x[s0];
		y[s0] = y[s0] + p;
	}
}

// dccrgx_field_reduce, first stage: one streaming pass over the slots
// [s0, s1) for all terms.  A thread takes W cells a pass and stages every
// distinct field's value of them in its LDS columns (dccrgx_reduce.hpp), each
// field loaded once per cell, eight loads in flight.  W == 2: pairs from the
// first even slot on as 16-byte loads (a field's array starts 256-byte
// aligned), a leading odd slot by the first thread and a trailing single one
// on their own, as field_axpy_kernel has them; 2 KB of LDS per field and
// cell of the pair, so up to 16 fields.  W == 1 takes the 17 to 32 fields
// that 16 terms can name.
constexpr int kRB = 256;
constexpr int kRedFields = 32;

struct RedFields {
	const double* f[kRedFields];
};

// V_c of slot c (RedVolume)
__device__ __forceinline__ double red_cell_volume(const MapCtx& m, const RedVolume& V, size_t c) {
#pragma clang fp contract(off)
	if (V.mode == 2) return cell_volume(m, V.G, V.slot_ids[c]);
	if (V.mode != 1) return 1.0;
	if (!V.slot_lvl) return V.vol0;
	const int lvl = V.slot_lvl[c] & 31;  // (the byte's upper bits hold the octant)
	const double sf3 = __longlong_as_double((1023ll - 3ll * lvl) << 52);  // 2^(-3 level)
	return V.vol0 * sf3;
}

template <int W>
__global__ __launch_bounds__(kRB) void field_reduce_kernel(const MapCtx m, const RedArgs T, const RedFields F,
                                                           const RedVolume V, size_t s0, size_t s1,
                                                           double* __restrict__ part) {
#pragma clang fp contract(off)
	extern __shared__ double red_sh[];
	constexpr int STRIDE = kRB * W;
	double acc[kRedTerms];
	red_init(T, acc);
	const int col = int(threadIdx.x);
	auto single = [&](size_t c) {
		for (int f0 = 0; f0 < T.nv; f0 += 8) {
			double v[8];
#pragma unroll
			for (int k = 0; k < 8; k++)
				if (f0 + k < T.nv) v[k] = F.f[f0 + k][c];
#pragma unroll
			for (int k = 0; k < 8; k++)
				if (f0 + k < T.nv) red_sh[(f0 + k) * STRIDE + col] = v[k];
		}
		red_accumulate(T, red_sh, STRIDE, col, red_cell_volume(m, V, c), acc);
	};
	if constexpr (W == 1) {
		for (size_t c = s0 + blockIdx.x * size_t(kRB) + threadIdx.x; c < s1; c += size_t(gridDim.x) * kRB) single(c);
	} else {
		const size_t b = (s0 + 1) & ~size_t(1);
		if (b != s0 && blockIdx.x == 0 && threadIdx.x == 0) single(s0);  // (s0 < s1: no launch for an empty range)
		for (size_t i = b + 2 * (blockIdx.x * size_t(kRB) + threadIdx.x); i < s1; i += 2 * size_t(gridDim.x) * kRB) {
			if (i + 1 < s1) {
				for (int f0 = 0; f0 < T.nv; f0 += 8) {
					double2 v[8];
#pragma unroll
					for (int k = 0; k < 8; k++)
						if (f0 + k < T.nv) v[k] = *reinterpret_cast<const double2*>(F.f[f0 + k] + i);
#pragma unroll
					for (int k = 0; k < 8; k++)
						if (f0 + k < T.nv) {
							red_sh[(f0 + k) * STRIDE + col] = v[k].x;
							red_sh[(f0 + k) * STRIDE + kRB + col] = v[k].y;
						}
				}
				red_accumulate(T, red_sh, STRIDE, col, red_cell_volume(m, V, i), acc);
				red_accumulate(T, red_sh, STRIDE, kRB + col, red_cell_volume(m, V, i + 1), acc);
			} else {
				single(i);
			}
		}
	}
	const double r = red_block<kRB>(T, red_sh, acc);
	if (int(threadIdx.x) < T.n) part[size_t(blockIdx.x) * kRedTerms + threadIdx.x] = r;
}

// second stage of dccrgx_field_reduce and dccrgx_particles_reduce: block j
// folds the nb partials of term j, thread t the partials t, t + kRB, .. in
// that order, then the block as in the first stage; nb == 0 leaves the
// operation's identity
__global__ __launch_bounds__(kRB) void reduce_fold_kernel(const RedArgs T, const double* __restrict__ part, unsigned nb,
                                                          double* __restrict__ out) {
#pragma clang fp contract(off)
	__shared__ double sh[kRB / 64];
	const int j = int(blockIdx.x);
	const int cop = red_combine_op(T.op[j]);
	double v = red_identity(T.op[j]);
	for (unsigned i = threadIdx.x; i < nb; i += kRB) v = red_combine(cop, v, part[size_t(i) * kRedTerms + j]);
	for (int o = 32; o > 0; o >>= 1) v = red_combine(cop, v, __shfl_down(v, o, 64));
	if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
	__syncthreads();
	if (threadIdx.x == 0) {
		double r = sh[0];
		for (int i = 1; i < kRB / 64; i++) r = red_combine(cop, r, sh[i]);
		out[j] = r;
	}
}

}  // namespace

unsigned k_field_reduce_blocks(size_t n, int nv) {
	if (!n) return 0;
	const size_t per = size_t(kRB) * (nv <= kRedFields / 2 ? 2 : 1);
	return grid_for(n + 1, unsigned(per), 2048);  // (+ 1: the pairs start at the first even slot)
}

void k_field_reduce(const MapCtx& m, const RedArgs& T, const double* const* fields, const RedVolume& V, size_t s0,
                    size_t s1, unsigned nb, double* part, hipStream_t s) {
	if (s1 <= s0 || !nb) return;
	DX_REQUIRE(T.nv <= kRedFields, "more distinct fields than a reduction stages");
	RedFields F{};
	for (int f = 0; f < T.nv; f++) F.f[f] = fields[f];
	const int W = T.nv <= kRedFields / 2 ? 2 : 1;
	const size_t lds = std::max(size_t(T.nv) * kRB * W, size_t(kRedTerms) * (kRB / 64)) * sizeof(double);
	if (W == 2)
		field_reduce_kernel<2><<<nb, kRB, lds, s>>>(m, T, F, V, s0, s1, part);
	else
		field_reduce_kernel<1><<<nb, kRB, lds, s>>>(m, T, F, V, s0, s1, part);
	HIP_CHECK(hipGetLastError());
}

void k_reduce_fold(const RedArgs& T, const double* part, unsigned nb, double* out, hipStream_t s) {
	reduce_fold_kernel<<<unsigned(T.n), kRB, 0, s>>>(T, part, nb, out);
	HIP_CHECK(hipGetLastError());
}

void k_gradient(const FaceStencil& F, const double* in, double* const out[3], double scale, size_t s0, size_t s1,
                hipStream_t s) {
	if (s1 <= s0) return;
	const unsigned nb = xcd_blocks(s1 - s0);
	if (F.G.c)
		gradient_kernel<true><<<nb, BS, 0, s>>>(F.m, F.l0[0], F.l0[1], F.l0[2], F.G, F.slot_ids, F.slot_lvl, F.face_ell,
		                                        F.face_fine, in, out[0], out[1], out[2], scale, s0, s1);
	else
		gradient_kernel<false><<<nb, BS, 0, s>>>(F.m, F.l0[0], F.l0[1], F.l0[2], F.G, F.slot_ids, F.slot_lvl, F.face_ell,
		                                         F.face_fine, in, out[0], out[1], out[2], scale, s0, s1);
	HIP_CHECK(hipGetLastError());
}

namespace {
// launch(std::bool_constant<STRETCHED>, std::bool_constant<ACCUMULATE>) for the
// run-time pair of curl and divergence
template <class L>
void stretched_accumulate(bool stretched, bool accumulate, L&& launch) {
	if (stretched) {
		if (accumulate) launch(std::true_type{}, std::true_type{});
		else launch(std::true_type{}, std::false_type{});
	} else {
		if (accumulate) launch(std::false_type{}, std::true_type{});
		else launch(std::false_type{}, std::false_type{});
	}
	HIP_CHECK(hipGetLastError());
}
}  // namespace

void k_curl(const FaceStencil& F, const double* const in[3], double* const out[3], double scale, bool accumulate,
            size_t s0, size_t s1, hipStream_t s) {
	if (s1 <= s0) return;
	stretched_accumulate(F.G.c != nullptr, accumulate, [&](auto S, auto A) {
		curl_kernel<decltype(S)::value, decltype(A)::value><<<xcd_blocks(s1 - s0), BS, 0, s>>>(
			F.m, F.l0[0], F.l0[1], F.l0[2], F.G, F.slot_ids, F.slot_lvl, F.face_ell, F.face_fine, in[0], in[1], in[2],
			out[0], out[1], out[2], scale, s0, s1);
	});
}

void k_divergence(const FaceStencil& F, const double* const in[3], double* out, double scale, bool accumulate,
                  size_t s0, size_t s1, hipStream_t s) {
	if (s1 <= s0) return;
	stretched_accumulate(F.G.c != nullptr, accumulate, [&](auto S, auto A) {
		divergence_kernel<decltype(S)::value, decltype(A)::value><<<xcd_blocks(s1 - s0), BS, 0, s>>>(
			F.m, F.l0[0], F.l0[1], F.l0[2], F.G, F.slot_ids, F.slot_lvl, F.face_ell, F.face_fine, in[0], in[1], in[2],
			out, scale, s0, s1);
	});
}

void k_field_axpy(double* y, double a, const double* x, size_t s0, size_t s1, hipStream_t s) {
	if (s1 <= s0) return;
	const size_t pairs = (s1 - s0) / 2 + 1;  // from the first even slot on, a trailing single one included
	field_axpy_kernel<<<unsigned((pairs + BS - 1) / BS), BS, 0, s>>>(y, x, a, s0, s1);
	HIP_CHECK(hipGetLastError());
}

// ---- the host side ------------------------------------------------------------
namespace {
const char* const VC_FP64 ="the fields of a curl, divergence or axpy must be fixed-size fields of 8-byte elements (fp64)";

// the three inputs of a curl or divergence (they need not be distinct)
void vector_inputs(Grid& g, const int in_fields[3], const double* in[3]) {
	for (int j = 0; j < 3; j++) {
		DX_REQUIRE(fixed_field(g, in_fields[j]).elem == 8, VC_FP64);
		in[j] = reinterpret_cast<const double*>(field(g, in_fields[j]).data.p);
	}
}

// the optional output triple of gradient and curl (-1: not wanted), with the
// operator's own messages: every output a fixed fp64 field, none of them an
// input, all distinct, at least one wanted; then the region; then - every
// check has passed - the outputs marked written and their arrays
struct OutputTexts {
	const char *fp64, *is_input, *twice, *none;
};
void wanted_outputs(Grid& g, const int out_fields[3], const int* in_fields, int n_in, const OutputTexts& t, int region,
                    size_t& s0, size_t& s1, double* out[3]) {
	int wanted = 0;
	for (int k = 0; k < 3; k++) {
		if (out_fields[k] == -1) continue;
		DX_REQUIRE(fixed_field(g, out_fields[k]).elem == 8, t.fp64);
		for (int j = 0; j < n_in; j++) DX_REQUIRE(out_fields[k] != in_fields[j], t.is_input);
		for (int e = 0; e < k; e++) DX_REQUIRE(out_fields[e] != out_fields[k], t.twice);
		wanted++;
	}
	DX_REQUIRE(wanted, t.none);
	region_range(g, region, s0, s1);
	for (int k = 0; k < 3; k++) {
		out[k] = nullptr;
		if (out_fields[k] == -1) continue;
		Field& F = field(g, out_fields[k]);
		field_written(F);
		out[k] = reinterpret_cast<double*>(F.data.p);
	}
}
}  // namespace

void field_gradient(Grid& g, int in_field, const int out_fields[3], double scale, int region) {
	DX_REQUIRE(g.initialized, "grid not initialized");
	DX_REQUIRE(out_fields, "null pointer");
	static const OutputTexts texts{
		"the gradient's input and outputs must be fixed-size fields of 8-byte elements (fp64)",
		"a gradient output is the input field", "two gradient outputs are one field",
		"no gradient output wanted (all three are -1)"};
	DX_REQUIRE(fixed_field(g, in_field).elem == 8, texts.fp64);
	size_t s0, s1;
	double* out[3];
	wanted_outputs(g, out_fields, &in_field, 1, texts, region, s0, s1, out);
	const FaceStencil F = face_stencil(g);
	k_time_begin(g);
	k_gradient(F, reinterpret_cast<const double*>(field(g, in_field).data.p), out, scale, s0, s1, g.s_comp);
	k_time_end(g);
}

void field_curl(Grid& g, const int in_fields[3], const int out_fields[3], double scale, bool accumulate, int region) {
	DX_REQUIRE(g.initialized, "grid not initialized");
	DX_REQUIRE(in_fields && out_fields, "null pointer");
	const double* in[3];
	vector_inputs(g, in_fields, in);
	static const OutputTexts texts{VC_FP64, "a curl output is an input field", "two curl outputs are one field",
	                               "no curl output wanted (all three are -1)"};
	size_t s0, s1;
	double* out[3];
	wanted_outputs(g, out_fields, in_fields, 3, texts, region, s0, s1, out);
	const FaceStencil F = face_stencil(g);
	k_time_begin(g);
	k_curl(F, in, out, scale, accumulate, s0, s1, g.s_comp);
	k_time_end(g);
}

void field_divergence(Grid& g, const int in_fields[3], int out_field, double scale, bool accumulate, int region) {
	DX_REQUIRE(g.initialized, "grid not initialized");
	DX_REQUIRE(in_fields, "null pointer");
	const double* in[3];
	vector_inputs(g, in_fields, in);
	DX_REQUIRE(fixed_field(g, out_field).elem == 8, VC_FP64);
	for (int j = 0; j < 3; j++) DX_REQUIRE(out_field != in_fields[j], "the divergence's output is an input field");
	size_t s0, s1;
	region_range(g, region, s0, s1);
	const FaceStencil F = face_stencil(g);
	Field& out = field(g, out_field);
	field_written(out);
	k_time_begin(g);
	k_divergence(F, in, reinterpret_cast<double*>(out.data.p), scale, accumulate, s0, s1, g.s_comp);
	k_time_end(g);
}

void field_axpy(Grid& g, int y_field, double a, int x_field, int region) {
	DX_REQUIRE(g.initialized, "grid not initialized");
	DX_REQUIRE(fixed_field(g, y_field).elem == 8 && fixed_field(g, x_field).elem == 8, VC_FP64);
	DX_REQUIRE(x_field != y_field, "the axpy's x and y are one field");
	size_t s0, s1;
	region_range(g, region, s0, s1);
	Field& Y = field(g, y_field);
	field_written(Y);
	k_time_begin(g);
	k_field_axpy(reinterpret_cast<double*>(Y.data.p), a, reinterpret_cast<const double*>(field(g, x_field).data.p),
	             s0, s1, g.s_comp);
	k_time_end(g);
}

// dccrgx_field_reduce into the device doubles d_out, everything queued on the
// compute stream: the first stage over the region's slots (field_reduce_kernel),
// the fold of the blocks' partials, and with `collective` the rank-ordered
// combine.  Every check precedes the first write.
void field_reduce_device(Grid& g, const int* terms, int n, int by_volume, int region, int collective, double* d_out) {
	DX_REQUIRE(g.initialized, "grid not initialized");
	DX_REQUIRE(n >= 1 && n <= kRedTerms, "the number of terms must be 1 .. 16");
	DX_REQUIRE(terms && d_out, "null pointer");
	RedArgs T;
	T.n = n;
	int ids[2 * kRedTerms], cops[kRedTerms];
	const double* fields[2 * kRedTerms];
	auto staged = [&](int fid) {  // the column of a field's value
		if (fid == -1) return kRedOne;
		for (int i = 0; i < T.nv; i++)
			if (ids[i] == fid) return i;
		DX_REQUIRE(fixed_field(g, fid).elem == 8,
		           "the fields of a reduction must be fixed-size fields of 8-byte elements (fp64)");
		ids[T.nv] = fid;
		fields[T.nv] = reinterpret_cast<const double*>(field(g, fid).data.p);
		return T.nv++;
	};
	for (int j = 0; j < n; j++) {
		const int op = terms[3 * j];
		DX_REQUIRE(op >= DCCRGX_REDUCE_SUM && op <= DCCRGX_REDUCE_MAX_ABS, "unknown reduction (DCCRGX_REDUCE_*)");
		T.op[j] = int8_t(op);
		T.x0[j] = int8_t(staged(terms[3 * j + 1]));
		T.x1[j] = int8_t(staged(terms[3 * j + 2]));
		T.x2[j] = int8_t(by_volume && op == DCCRGX_REDUCE_SUM ? kRedExtra : kRedOne);
		cops[j] = red_combine_op(op);
	}
	size_t s0, s1;
	region_range(g, region, s0, s1);
	if (collective && g.size > 1) comm_require(g, "a collective reduction");
	const RedVolume V = reduce_volume(g, by_volume != 0);
	hipStream_t s = g.s_comp;
	const unsigned nb = s1 > s0 ? k_field_reduce_blocks(s1 - s0, T.nv) : 0;
	k_time_begin(g);
	if (nb) {
		g.red_part.reserve(size_t(nb) * kRedTerms);
		k_field_reduce(g.m, T, fields, V, s0, s1, nb, g.red_part.p, s);
	}
	k_reduce_fold(T, g.red_part.p, nb, d_out, s);
	k_time_end(g);
	if (collective) comm_allreduce_f64_ops_dev(g, d_out, d_out, n, cops, s);
}

}  // namespace dccrgx

