// The first-derivative stencil over the face table, shared by the kernels of
// field_ops.hip (gradient, curl, divergence) and field_adapt.hip (the
// slopes of a limited linear prolongation): one definition, so one set of bits.
#pragma once

#include "dccrgx_internal.hpp"

namespace dccrgx {

// ---- the first-derivative stencil over the face table ------------------------
// What gradient_kernel, curl_kernel and divergence_kernel share, so that the
// derivative of a field along a dimension has the same bits in all three
// (dccrgx.h: D_d(F)[c]): the face row, a side's value and level, the lengths,
// a dimension's coefficients and the three-point derivative.

// the six face entries of row s (24 bytes, 8-byte aligned) together
__device__ __forceinline__ void face_row(const int32_t* __restrict__ face_ell, size_t s, int32_t (&ev)[6]) {
	const int2* row = reinterpret_cast<const int2*>(face_ell + 6 * s);
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const int2 r = row[k];
		ev[2 * k] = r.x;
		ev[2 * k + 1] = r.y;
	}
}

// the value of `in` across the face entry e: the neighbor's, the mean of the
// four finer cells' in face_fine order, or 0.0 without a neighbor
__device__ __forceinline__ double face_value(const double* __restrict__ in, const int32_t* __restrict__ face_fine,
                                             int32_t e) {
#pragma clang fp contract(off)
	double v = 0.0;
	if (e >= 0) {
		v = in[e];
	} else if (e < -1) {
		const int32_t* f = face_fine + 4 * size_t(-2 - e);
		const double a0 = in[f[0]], a1 = in[f[1]], a2 = in[f[2]], a3 = in[f[3]];
		v = ((a0 + a1) + (a2 + a3)) / 4.0;
	}
	return v;
}

// the level of the cell(s) across the face entry e of a cell of level lvl
__device__ __forceinline__ int face_level(const uint8_t* __restrict__ slot_lvl, int32_t e, int lvl) {
	if (e >= 0) return slot_lvl[e] & 31;
	return e < -1 ? lvl + 1 : lvl;
}

// lengths along d of the cell of slot s (lc) and of its two neighbors (ln),
// whose levels are nl
template <bool STRETCHED>
__device__ __forceinline__ void stencil_lengths(const MapCtx& m, double l0x, double l0y, double l0z,
                                                const StretchedView& G, const uint64_t* __restrict__ slot_ids,
                                                size_t s, int lvl, const int (&nl)[6], double (&lc)[3],
                                                double (&ln)[6]) {
#pragma clang fp contract(off)
	if constexpr (STRETCHED) {
		uint64_t ind[3] = {0, 0, 0};
		map_indices(m, slot_ids[s], ind[0], ind[1], ind[2]);
		const uint64_t size = uint64_t(1) << (m.R - lvl);
#pragma unroll
		for (int d = 0; d < 3; d++) {
			const double* c = G.c + G.off[d];
			const uint64_t i0 = ind[d] >> m.R;
			lc[d] = (c[i0 + 1] - c[i0]) / double(uint64_t(1) << lvl);
			const uint64_t lo = ind[d] == 0 ? m.glen[d] - 1 : ind[d] - 1;
			const uint64_t hi = ind[d] + size >= m.glen[d] ? 0 : ind[d] + size;
			const uint64_t in_ = lo >> m.R, ip = hi >> m.R;
			ln[2 * d] = (c[in_ + 1] - c[in_]) / double(uint64_t(1) << nl[2 * d]);
			ln[2 * d + 1] = (c[ip + 1] - c[ip]) / double(uint64_t(1) << nl[2 * d + 1]);
		}
	} else {
		const double l0[3] = {l0x, l0y, l0z};
#pragma unroll
		for (int d = 0; d < 3; d++) {
			lc[d] = l0[d] * (1.0 / double(uint64_t(1) << lvl));  // Cartesian get_length
			ln[2 * d] = l0[d] * (1.0 / double(uint64_t(1) << nl[2 * d]));
			ln[2 * d + 1] = l0[d] * (1.0 / double(uint64_t(1) << nl[2 * d + 1]));
		}
	}
}

// a dimension's coefficients: with both sides a and b of the three-point
// stencil; with one side the centre distance h in `a` (the contract divides by
// it, so the divisor is kept and not its reciprocal)
constexpr int ST_NONE = 0, ST_BOTH = 1, ST_POS = 2, ST_NEG = 3;
struct StencilDim {
	int sides;
	double a, b;
};
__device__ __forceinline__ StencilDim stencil_dim(double lc, double ln_neg, double ln_pos, int32_t e_neg,
                                                  int32_t e_pos) {
#pragma clang fp contract(off)
	const double hc = lc / 2.0;
	const bool has_neg = e_neg != -1, has_pos = e_pos != -1;
	const double h_neg = hc + ln_neg / 2.0, h_pos = hc + ln_pos / 2.0;
	StencilDim k{ST_NONE, 0.0, 0.0};
	if (has_neg && has_pos) {
		const double tot = h_pos + h_neg;
		k.sides = ST_BOTH;
		k.a = h_neg / (h_pos * tot);
		k.b = h_pos / (h_neg * tot);
	} else if (has_pos) {
		k.sides = ST_POS;
		k.a = h_pos;
	} else if (has_neg) {
		k.sides = ST_NEG;
		k.a = h_neg;
	}
	return k;
}

// the derivative along the dimension of k from the values on its two sides
// and the cell's own: `grad` of dccrgx_gradient's contract, before the scaling
__device__ __forceinline__ double stencil_derivative(const StencilDim& k, double v_neg, double vc, double v_pos) {
#pragma clang fp contract(off)
	const double dp = v_pos - vc, dn = vc - v_neg;
	double grad = 0.0;
	if (k.sides == ST_BOTH) grad = k.a * dp + k.b * dn;
	else if (k.sides == ST_POS) grad = dp / k.a;
	else if (k.sides == ST_NEG) grad = dn / k.a;
	return grad;
}

}  // namespace dccrgx
