// Up to 16 reductions over the elements of one walk (dccrgx_field_reduce over
// cells, dccrgx_particles_reduce over records): the device routines both
// kernels share and the second stage that folds the blocks' partials.
//
// A thread stages the values of its element in LDS, one column per thread
// (value f of the column `col` at sh[f * stride + col]): every distinct value
// is loaded from memory once, and a term picks its factors from the column by
// an index that is uniform over the wave, which registers cannot be indexed
// by.  Term j of the element is (x0 * x1) * x2, two IEEE products; a factor
// index of kRedOne stands for 1.0 (the product with it is exact), kRedExtra
// for the element's extra value (the cell volume).  The thread folds the term
// into its accumulator j; the block's threads are folded by a shuffle tree
// and through LDS in wave order; block b stores its partial of term j at
// part[b * kRedTerms + j] with a plain store.  reduce_fold_kernel folds the
// partials of a term in the same way.  No atomic takes part and the grid
// size is a function of the problem, so the order of every sum is fixed.
#pragma once

#include "dccrgx_internal.hpp"

namespace dccrgx {

constexpr int kRedOne = -1;    // factor 1.0
constexpr int kRedExtra = -2;  // the element's extra value

// the identity of an operation: the result over no elements
DX_HD double red_identity(int op) {
	if (op == DCCRGX_REDUCE_MIN) return __builtin_huge_val();
	if (op == DCCRGX_REDUCE_MAX) return -__builtin_huge_val();
	return 0.0;
}

// how two partial results of `op` combine (MAX_ABS: as MAX, the absolute
// value was taken of the term); the comparisons keep the first operand on NaN
DX_HD int red_combine_op(int op) { return op == DCCRGX_REDUCE_MAX_ABS ? DCCRGX_REDUCE_MAX : op; }

#ifdef __HIPCC__

__device__ __forceinline__ double red_combine(int cop, double acc, double x) {
#pragma clang fp contract(off)
	if (cop == DCCRGX_REDUCE_SUM) return acc + x;
	if (cop == DCCRGX_REDUCE_MIN) return (x < acc) ? x : acc;
	return (acc < x) ? x : acc;
}

__device__ __forceinline__ void red_init(const RedArgs& T, double (&acc)[kRedTerms]) {
#pragma unroll
	for (int j = 0; j < kRedTerms; j++) acc[j] = red_identity(j < T.n ? T.op[j] : 0);
}

// the terms of the element whose values stand in column `col` of sh
__device__ __forceinline__ void red_accumulate(const RedArgs& T, const double* sh, int stride, int col, double extra,
                                               double (&acc)[kRedTerms]) {
#pragma clang fp contract(off)
#pragma unroll
	for (int j = 0; j < kRedTerms; j++) {
		if (j < T.n) {
			const int i0 = T.x0[j], i1 = T.x1[j], i2 = T.x2[j];
			const double x0 = i0 < 0 ? 1.0 : sh[i0 * stride + col];
			const double x1 = i1 < 0 ? 1.0 : sh[i1 * stride + col];
			const double x2 = i2 == kRedExtra ? extra : (i2 < 0 ? 1.0 : sh[i2 * stride + col]);
			const double p = x0 * x1;
			const double t = p * x2;
			const int op = T.op[j];
			acc[j] = red_combine(red_combine_op(op), acc[j], op == DCCRGX_REDUCE_MAX_ABS ? fabs(t) : t);
		}
	}
}

// the block's accumulators folded: lanes by a shuffle tree, waves in order
// through sh (at least kRedTerms * B / 64 doubles, free to overwrite once
// every thread is here); thread j < n holds term j's result on return
template <int B>
__device__ __forceinline__ double red_block(const RedArgs& T, double* sh, double (&acc)[kRedTerms]) {
#pragma clang fp contract(off)
	constexpr int W = B / 64;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	__syncthreads();  // the columns are read no more
#pragma unroll
	for (int j = 0; j < kRedTerms; j++) {
		if (j < T.n) {
			const int cop = red_combine_op(T.op[j]);
			double v = acc[j];
			for (int o = 32; o > 0; o >>= 1) v = red_combine(cop, v, __shfl_down(v, o, 64));
			if (lane == 0) sh[j * W + w] = v;
		}
	}
	__syncthreads();
	double r = 0.0;
	if (int(threadIdx.x) < T.n) {
		const int j = int(threadIdx.x);
		const int cop = red_combine_op(T.op[j]);
		r = sh[j * W];
		for (int i = 1; i < W; i++) r = red_combine(cop, r, sh[j * W + i]);
	}
	return r;
}

#endif  // __HIPCC__

}  // namespace dccrgx
