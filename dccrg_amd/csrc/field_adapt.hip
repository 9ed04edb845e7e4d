// Cell fields follow the mesh (dccrgx_field_follow_mesh, dccrgx.h): what
// stop_refining does to a fixed fp64 field whose mode is not off.
//  * slope pass (before the rebuild, old mesh and old values): per refined
//    local cell and LINEAR field the three limited half-differences t_d, from
//    the derivative dccrgx_gradient forms (dccrgx_stencil.hpp: the same
//    functions, so the same bits) and the extrema of the face-neighbor leaves;
//  * carry (rebuild step 6): the gather of the old payloads with the child
//    rule where a new local slot's source is a coarser old cell;
//  * restriction (after the rebuild): the merged parents' mean or sum of
//    their eight removed children, all following fields in one launch; the
//    kernel is adapt_grid's parent density (adapter.hpp:260-290) too.
// These are gather-bound passes over lists (the refined cells, the new slots,
// the merged parents): one lane per list entry, the field on blockIdx.y so a
// field's pointers stay wave-uniform.  No atomics decide a value.
#include "dccrgx_grid.hpp"
#include "dccrgx_stencil.hpp"

namespace dccrgx {

namespace {

constexpr int FBS = 256;

struct SlopeFields {
	const double* in[kFollowBatch];
};

// the child's octant in its parent (bit d = upper half along d): its place in
// map_all_children's order, which is the ascending id order
__device__ __forceinline__ int child_octant(const MapCtx& m, uint64_t id) {
	uint64_t x, y, z;
	const int l = map_indices(m, id, x, y, z);
	const uint64_t o = uint64_t(1) << (m.R - l);  // the child's length in indices
	return int((x / o) & 1u) | int(((y / o) & 1u) << 1) | int(((z / o) & 1u) << 2);
}

// t_d = alpha * e_d of dccrgx_field_follow_mesh's contract for the refined
// cells of the list that are local here (row j0 + blockIdx.y of t)
template <bool STRETCHED>
__global__ __launch_bounds__(FBS) void field_slopes_kernel(MapCtx m, double l0x, double l0y, double l0z, StretchedView G,
                                                           const uint64_t* __restrict__ slot_ids,
                                                           const uint8_t* __restrict__ slot_lvl,
                                                           const int32_t* __restrict__ face_ell,
                                                           const int32_t* __restrict__ face_fine, size_t n_local,
                                                           const int32_t* __restrict__ pslot, size_t n, SlopeFields F,
                                                           int j0, double* __restrict__ t,
                                                           int32_t* __restrict__ ppos) {
#pragma clang fp contract(off)
	const double* __restrict__ in = F.in[blockIdx.y];
	double* __restrict__ tj = t + size_t(3) * size_t(j0 + int(blockIdx.y)) * n;
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const int32_t ps = pslot[i];
		if (ps < 0 || size_t(ps) >= n_local) continue;  // refined by another process
		const size_t s = size_t(ps);
		if (blockIdx.y == 0 && j0 == 0) ppos[s] = int32_t(i);
		int32_t ev[6];
		face_row(face_ell, s, ev);
		const int lvl = slot_lvl[s] & 31;
		const double vc = in[s];
		double v[6], mn = vc, mx = vc;
		int nl[6];
#pragma unroll
		for (int dir = 0; dir < 6; dir++) {
			const int32_t e = ev[dir];
			v[dir] = face_value(in, face_fine, e);
			nl[dir] = face_level(slot_lvl, e, lvl);
			if (e >= 0) {
				mn = v[dir] < mn ? v[dir] : mn;
				mx = v[dir] > mx ? v[dir] : mx;
			} else if (e < -1) {
				// each of the four finer leaves on its own
				const int32_t* f = face_fine + 4 * size_t(-2 - e);
#pragma unroll
				for (int q = 0; q < 4; q++) {
					const double a = in[f[q]];
					mn = a < mn ? a : mn;
					mx = a > mx ? a : mx;
				}
			}
		}
		double lc[3], ln[6];
		stencil_lengths<STRETCHED>(m, l0x, l0y, l0z, G, slot_ids, s, lvl, nl, lc, ln);
		double e3[3];
#pragma unroll
		for (int d = 0; d < 3; d++) {
			const StencilDim k = stencil_dim(lc[d], ln[2 * d], ln[2 * d + 1], ev[2 * d], ev[2 * d + 1]);
			const double gd = stencil_derivative(k, v[2 * d], vc, v[2 * d + 1]);
			const double qd = lc[d] * 0.25;
			e3[d] = gd * qd;
		}
		const double delta = (fabs(e3[0]) + fabs(e3[1])) + fabs(e3[2]);
		double alpha = 1.0;
		if (delta > 0.0) {
			const double up = (mx - vc) / delta;
			const double dn = (vc - mn) / delta;
			const double lim = up < dn ? up : dn;
			alpha = lim < 1.0 ? lim : 1.0;
		}
#pragma unroll
		for (int d = 0; d < 3; d++) tj[size_t(d) * n + i] = alpha * e3[d];
	}
}

// rebuild step 6 for a SUM or LINEAR field: gather_rows_kernel, and where a
// new local slot's source is another (coarser) cell, its parent, the child
// rule with the signs of the slot's own id
__global__ __launch_bounds__(FBS) void field_follow_gather_kernel(MapCtx m, const double* __restrict__ old,
                                                                  const int32_t* __restrict__ src, size_t n, size_t nl,
                                                                  const uint64_t* __restrict__ ids,
                                                                  const uint64_t* __restrict__ old_ids, int mode,
                                                                  const double* __restrict__ t,
                                                                  const int32_t* __restrict__ ppos, size_t n_ppos,
                                                                  size_t np, double* __restrict__ out) {
#pragma clang fp contract(off)
	for (size_t s = blockIdx.x * size_t(blockDim.x) + threadIdx.x; s < n; s += size_t(gridDim.x) * blockDim.x) {
		const int32_t r = src[s];
		double v = 0.0;
		if (r >= 0) {
			v = old[r];
			if (s < nl) {
				const uint64_t id = ids[s];
				if (old_ids[r] != id) {
					if (mode == DCCRGX_FOLLOW_SUM) {
						v = v * 0.125;
					} else if (t && size_t(r) < n_ppos) {
						const int32_t p = ppos[r];
						if (p >= 0 && size_t(p) < np) {
							const int k = child_octant(m, id);
							const double t0 = t[size_t(p)], t1 = t[np + size_t(p)], t2 = t[2 * np + size_t(p)];
							v = v + (k & 1 ? t0 : -t0);
							v = v + (k & 2 ? t1 : -t1);
							v = v + (k & 4 ? t2 : -t2);
						}
					}
				}
			}
		}
		out[s] = v;
	}
}

// a merged parent's value from its eight removed children in ascending id:
// acc = acc + c_k / 8.0 (adapt_grid's density, adapter.hpp:260-290), or the
// plain sum for an extensive field
__global__ __launch_bounds__(FBS) void field_merge_parents_kernel(FollowSet F, const int32_t* __restrict__ parent_slot,
                                                                  const int32_t* __restrict__ child_idx, size_t np) {
#pragma clang fp contract(off)
	double* __restrict__ data = F.data[blockIdx.y];
	const double* __restrict__ removed = F.removed[blockIdx.y];
	const bool sum = F.mode[blockIdx.y] == DCCRGX_FOLLOW_SUM;
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < np; i += size_t(gridDim.x) * blockDim.x) {
		double c[8];
#pragma unroll
		for (int k = 0; k < 8; k++) c[k] = removed[child_idx[8 * i + k]];
		double acc = 0;
		if (sum) {
#pragma unroll
			for (int k = 0; k < 8; k++) acc += c[k];
		} else {
#pragma unroll
			for (int k = 0; k < 8; k++) acc += c[k] / 8;
		}
		data[parent_slot[i]] = acc;
	}
}

// merged families on the device: the parent of every removed child, and
// (after the parents are sorted and deduplicated) each child's place in its
// parent's row of eight, in map_all_children order (= ascending id)
__global__ void removed_parents_kernel(MapCtx m, const uint64_t* __restrict__ rm, size_t n, uint64_t* __restrict__ par) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
		par[i] = map_parent(m, rm[i]);
}

__global__ void removed_rows_kernel(MapCtx m, const uint64_t* __restrict__ rm, size_t n,
                                    const uint64_t* __restrict__ parents, size_t np, int32_t* __restrict__ cidx,
                                    int* __restrict__ err) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
		const int l = map_level(m, rm[i]);
		const uint64_t p = map_parent(m, rm[i]);
		size_t lo = 0, hi = np;
		while (lo < hi) {
			const size_t mid = (lo + hi) / 2;
			if (parents[mid] < p) lo = mid + 1;
			else hi = mid;
		}
		if (l <= 0 || lo >= np || parents[lo] != p) {
			atomicOr(err, 1);
			continue;
		}
		cidx[8 * lo + size_t(child_octant(m, rm[i]))] = int32_t(i);
	}
}

__global__ void check_rows_kernel(const int32_t* __restrict__ cidx, const int32_t* __restrict__ pslot, size_t np,
                                  size_t n_local, int* __restrict__ err) {
	for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < np; i += size_t(gridDim.x) * blockDim.x) {
		if (pslot[i] < 0 || size_t(pslot[i]) >= n_local) atomicOr(err, 2);
		for (int k = 0; k < 8; k++)
			if (cidx[8 * i + k] < 0) atomicOr(err, 4);
	}
}

}  // namespace

size_t k_merged_rows(const MapCtx& m, const DevMesh& dm, size_t n_local, LazyIds& rm, const uint64_t* parents,
                     size_t np_given, DBuf<int32_t>& cidx, DBuf<int32_t>& pslot, hipStream_t s) {
	if (rm.empty()) return 0;
	const size_t n = rm.size();
	DBuf<uint64_t> up, par;
	const uint64_t* rm_dev = rm.dev();
	if (!rm_dev) {
		upload(up, rm.host(s), s);
		rm_dev = up.p;
	}
	size_t np = np_given;
	const uint64_t* parp = parents;
	if (!(parents && np * 8 == n)) {
		// the parents of the removed cells (the families' parents as
		// stop_refining merged them, when given: sorted and unique, and
		// removed_rows / check_rows below still verify every child maps to one)
		par.alloc(n);
		removed_parents_kernel<<<grid_for(n, 256), 256, 0, s>>>(m, rm_dev, n, par.p);
		HIP_CHECK(hipGetLastError());
		np = sort_unique_u64(par.p, n, s, map_id_bits(m));
		parp = par.p;
	}
	DX_REQUIRE(np * 8 == n, "a merged family's removed children are incomplete");
	DBuf<int> err;
	cidx.alloc(8 * np);
	pslot.alloc(np);
	err.alloc(1);
	HIP_CHECK(hipMemsetAsync(cidx.p, 0xff, 8 * np * sizeof(int32_t), s));
	HIP_CHECK(hipMemsetAsync(err.p, 0, sizeof(int), s));
	removed_rows_kernel<<<grid_for(n, 256), 256, 0, s>>>(m, rm_dev, n, parp, np, cidx.p, err.p);
	HIP_CHECK(hipGetLastError());
	k_lookup_slots(parp, np, dm, pslot.p, err.p, s);  // a missing parent sets err too
	check_rows_kernel<<<grid_for(np, 256), 256, 0, s>>>(cidx.p, pslot.p, np, n_local, err.p);
	HIP_CHECK(hipGetLastError());
	int h = 0;
	d2h_small(&h, err.p, sizeof(int), s);
	DX_REQUIRE(h == 0, "merged parent is not local or a removed child's payload is missing");
	return np;
}

void k_field_merge_parents(const FollowSet& F, const int32_t* pslot, const int32_t* cidx, size_t np, hipStream_t s) {
	if (!np || F.n <= 0) return;
	DX_REQUIRE(F.n <= kFollowBatch, "internal error: too many fields in one restriction launch");
	field_merge_parents_kernel<<<dim3(grid_for(np, FBS), unsigned(F.n)), FBS, 0, s>>>(F, pslot, cidx, np);
	HIP_CHECK(hipGetLastError());
}

void k_field_slopes(const FaceStencil& S, size_t n_local, const int32_t* pslot, size_t n, const double* const* in,
                    int nlin, double* t, int32_t* ppos, hipStream_t s) {
	if (!n) return;
	for (int j0 = 0; j0 < nlin; j0 += kFollowBatch) {
		const int nb = std::min(kFollowBatch, nlin - j0);
		SlopeFields F;
		for (int j = 0; j < kFollowBatch; j++) F.in[j] = in[j0 + std::min(j, nb - 1)];
		const dim3 grid(grid_for(n, FBS), unsigned(nb));
		if (S.G.c)
			field_slopes_kernel<true><<<grid, FBS, 0, s>>>(S.m, S.l0[0], S.l0[1], S.l0[2], S.G, S.slot_ids, S.slot_lvl,
			                                               S.face_ell, S.face_fine, n_local, pslot, n, F, j0, t, ppos);
		else
			field_slopes_kernel<false><<<grid, FBS, 0, s>>>(S.m, S.l0[0], S.l0[1], S.l0[2], S.G, S.slot_ids, S.slot_lvl,
			                                                S.face_ell, S.face_fine, n_local, pslot, n, F, j0, t, ppos);
		HIP_CHECK(hipGetLastError());
	}
}

void k_field_follow_gather(const MapCtx& m, const double* old_data, const int32_t* src, size_t n_slots, size_t n_local,
                           const uint64_t* slot_ids, const uint64_t* old_slot_ids, int mode, const double* t,
                           const int32_t* ppos, size_t n_ppos, size_t n_refined, double* out, hipStream_t s) {
	if (!n_slots) return;
	field_follow_gather_kernel<<<grid_for(n_slots, FBS), FBS, 0, s>>>(m, old_data, src, n_slots, n_local, slot_ids,
	                                                                  old_slot_ids, mode, t, ppos, n_ppos, n_refined,
	                                                                  out);
	HIP_CHECK(hipGetLastError());
}

// ---- the host side ------------------------------------------------------------
void field_follow_set(Grid& g, int fid, int mode) {
	Field& f = fixed_field(g, fid);
	DX_REQUIRE(f.elem == 8, "a field that follows the mesh must be a fixed-size field of 8-byte elements (fp64)");
	DX_REQUIRE(mode >= DCCRGX_FOLLOW_OFF && mode <= DCCRGX_FOLLOW_LINEAR, "invalid follow mode");
	f.follow_mode = mode;
}

void field_slope_pass(Grid& g, const uint64_t* refined_dev, size_t n_refined) {
	g.fslopes.clear();
	std::vector<const double*> in;
	for (auto& f : g.fields) {
		f.follow_lin = -1;
		if (f.var || f.no_carry || f.follow_mode != DCCRGX_FOLLOW_LINEAR || !f.data.p) continue;
		f.follow_lin = int(in.size());
		in.push_back(reinterpret_cast<const double*>(f.data.p));
	}
	if (in.empty() || !n_refined || !g.n_local) {
		for (auto& f : g.fields) f.follow_lin = -1;
		return;
	}
	hipStream_t s = g.s_comp;
	const FaceStencil S = face_stencil(g);  // of the mesh about to be replaced
	DBuf<int32_t> pslot, err;
	pslot.alloc(n_refined);
	err.alloc(1);
	HIP_CHECK(hipMemsetAsync(err.p, 0, 4, s));
	// (cells refined by other processes may be unknown here: no slot, skipped)
	k_lookup_slots(refined_dev, n_refined, g.dm(), pslot.p, err.p, s);
	g.fslopes.n = n_refined;
	g.fslopes.t.alloc(3 * in.size() * n_refined);
	g.fslopes.ppos.alloc(g.n_local);
	k_field_slopes(S, g.n_local, pslot.p, n_refined, in.data(), int(in.size()), g.fslopes.t.p, g.fslopes.ppos.p, s);
}

void field_follow_restrict(Grid& g, const std::vector<int>& fids) {
	if (fids.empty() || g.removed_ids.empty()) return;
	hipStream_t s = g.s_comp;
	DBuf<int32_t> cidx, pslot;
	const size_t np = k_merged_rows(g.m, g.dm(), g.n_local, g.removed_ids, g.merged_dev.p, g.n_merged, cidx, pslot, s);
	for (size_t k0 = 0; k0 < fids.size(); k0 += kFollowBatch) {
		FollowSet F;
		for (size_t k = k0; k < fids.size() && F.n < kFollowBatch; k++) {
			Field& f = field(g, fids[k]);
			F.data[F.n] = reinterpret_cast<double*>(f.data.p);
			F.removed[F.n] = reinterpret_cast<const double*>(f.removed.p);
			F.mode[F.n] = f.follow_mode;
			F.n++;
			field_written(f);
		}
		k_field_merge_parents(F, pslot.p, cidx.p, np, s);
	}
}

}  // namespace dccrgx
