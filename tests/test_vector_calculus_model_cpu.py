"""tests/vector_calculus_model.py pinned before the GPU tests rely on it, and
the three entry points declared and exported.

* A linear field F = A x + b has the curl (A_zy - A_yz, A_xz - A_zx,
  A_yx - A_xy) and the divergence tr A at every cell of an unrefined open
  grid, one-sided edges included: the stencil's weights are a linear fit's.
  The field is evaluated at the exact cell centres in rational arithmetic and
  rounded once.  In half-units 2^-53 of a derivative's magnitude M the model
  may then be off by: 1 for the rounded input; 3 for a coefficient (tot, the
  product, the quotient; a one-sided quotient is 1); 3 for the difference,
  the product and the sum; and on a stretched grid 6 more, since a centre
  distance h = fl(fl(L_c / 2) + fl(L_n / 2)) of two rounded lengths is off by
  2 half-units and a coefficient holds three of them (Cartesian: h = l0
  exactly).  That is 13 per derivative.  The curl adds 1 for its difference
  (14 of M_1 + M_2), the divergence 2 for its two sums (15 of the three):
  both stay under 16 half-units = 8 * 2^-52 * M.
* div(curl F) and curl(grad phi) on unrefined grids: every D_d acts along d
  only and its rounded coefficients depend on the position along d only, so
  the operators commute and both are 0 in exact arithmetic.  What is left is
  rounding, bounded by 8 * 2^-52 * S with S the magnitude operator applied to
  the first stage's magnitudes.  The recount, in units of 2^-52: a derivative
  has three roundings (difference, product, sum) of half a unit of its M
  each, 1.5; a curl component adds its difference, 0.5 of M_1 + M_2, so the
  first stage is off by at most 2 of its magnitude (a gradient: 1.5), which
  the second stage carries to 2 S; the second stage's own derivatives add
  1.5 S and its two sums (or one difference) at most 1 S: 4.5 S for
  div(curl), 3.5 S for curl(grad).  The issue's count, which takes each
  stage's derivatives one by one (3.5 and 4), gives 7.5, rounded up to the 8
  used here; the recount lies below it, and the observed worst is printed.
"""
from fractions import Fraction

import numpy as np
import pytest

import advection_model as AM
import gradient_model as GM
import stretched_solver_cases as SC
import vector_calculus_model as VM

EPS = 2.0 ** -52
ODD_START, ODD_L0 = (0.1, -0.3, 0.2), (0.3, 0.7, 1.1)


def test_entry_points_are_declared_and_exported():
    import dccrg_amd

    L = dccrg_amd.lib()
    syms = dccrg_amd.header_symbols()
    for name in ("dccrgx_curl", "dccrgx_divergence", "dccrgx_field_axpy"):
        assert name in syms, name
        assert hasattr(L, name), name
    assert L.dccrgx_curl(None, None, None, 1.0, 0, 0) == dccrg_amd._lib.EINVAL
    assert b"null grid" in L.dccrgx_last_error()
    assert L.dccrgx_divergence(None, None, 0, 1.0, 0, 0) == dccrg_amd._lib.EINVAL
    assert b"null grid" in L.dccrgx_last_error()
    assert L.dccrgx_field_axpy(None, 0, 1.0, 1, 0) == dccrg_amd._lib.EINVAL
    assert b"null grid" in L.dccrgx_last_error()
    for name in ("curl", "divergence", "field_axpy"):
        assert callable(getattr(dccrg_amd.Dccrg, name))


def _mesh(base, coords):
    """The unrefined grid's ids, per-cell lengths and per-dimension exact
    edges (Fractions of the fp64 coordinates; coords None: Cartesian)."""
    ids = np.arange(1, base[0] * base[1] * base[2] + 1, dtype=np.uint64)
    if coords is None:
        L = GM.cartesian_lengths(ODD_L0, np.zeros(ids.size, np.int64))
        edges = [[Fraction(ODD_START[d]) + k * Fraction(ODD_L0[d]) for k in range(base[d] + 1)] for d in range(3)]
    else:
        L = GM.stretched_lengths(coords, base, 0, ids)
        edges = [[Fraction(float(x)) for x in coords[d]] for d in range(3)]
    return ids, L, edges


@pytest.mark.parametrize("geometry", ["cartesian", "stretched"])
def test_linear_field_has_the_curl_and_divergence_of_its_matrix(geometry):
    base, periodic = (4, 3, 5), (False, False, False)
    coords = SC.uneven_coords(base, 21) if geometry == "stretched" else None
    ids, L, edges = _mesh(base, coords)
    _, lo, _ = AM.boxes(ids, base, 0)
    rng = np.random.default_rng(3)
    A = rng.integers(-40, 41, (3, 3)) / 8.0
    b = rng.integers(-40, 41, 3) / 8.0
    assert all(A[i, j] != A[j, i] for i in range(3) for j in range(i))
    ctr = [[(edges[d][k] + edges[d][k + 1]) / 2 for k in range(base[d])] for d in range(3)]
    F = [np.array([float(sum(Fraction(A[j, i]) * ctr[i][int(lo[c, i])] for i in range(3)) + Fraction(b[j]))
                   for c in range(ids.size)]) for j in range(3)]
    G = VM.derivatives(ids, base, 0, periodic, L, F)
    assert not all(g.both.all() for g in G) and all(g.both.any() for g in G)  # one-sided edges take part
    cu, dv = VM.curl_of(G), VM.divergence_of(G)
    want = (A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1])
    for k in range(3):
        err = np.abs(cu.value[:, k] - want[k])
        print(geometry, "curl", k, "worst error / bound", float(np.max(err / (8 * EPS * cu.M[:, k]))))
        assert np.all(err <= 8 * EPS * cu.M[:, k])
    err = np.abs(dv.value - np.trace(A))
    print(geometry, "divergence worst error / bound", float(np.max(err / (8 * EPS * dv.M))))
    assert np.all(err <= 8 * EPS * dv.M)
    assert not cu.finer.any() and not dv.finer.any()


UNREFINED = [("cartesian", (4, 4, 4), (True, True, True)), ("cartesian", (4, 3, 5), (True, False, True)),
             ("cartesian", (4, 3, 5), (False, False, False)), ("stretched", (4, 3, 5), (True, False, True)),
             ("stretched", (4, 4, 4), (False, True, False))]


def second_order_identities(ids, base, periodic, L, F, phi, curl, grad, divergence, curl_of_grad):
    """max over cells of |div(curl F)| / (8 EPS S) and of |curl(grad phi)| /
    (8 EPS S_k), with the four operators given (the model's here, the
    device's in test_gpu_curl_divergence.py) and S from the model."""
    cu = VM.curl(ids, base, 0, periodic, L, F)
    S = VM.divergence(ids, base, 0, periodic, L, [cu.M[:, k] for k in range(3)]).M
    dc = np.abs(divergence(curl(F)))
    assert np.all(S > 0)
    worst_div = float(np.max(dc / (8 * EPS * S)))
    g = GM.gradient(ids, base, 0, periodic, L, phi)
    Sk = VM.curl(ids, base, 0, periodic, L, [g.M[:, d] for d in range(3)]).M
    cg = np.abs(curl_of_grad(grad(phi)))
    worst_curl = float(np.max(np.where(Sk > 0, cg / np.where(Sk > 0, 8 * EPS * Sk, 1.0), np.where(cg > 0, np.inf, 0))))
    return worst_div, worst_curl


@pytest.mark.parametrize("geometry,base,periodic", UNREFINED)
def test_div_curl_and_curl_grad_vanish_to_rounding(geometry, base, periodic):
    coords = SC.uneven_coords(base, 21) if geometry == "stretched" else None
    ids, L, _ = _mesh(base, coords)
    rng = np.random.default_rng(17)
    F = [rng.random(ids.size) * 2 - 1 for _ in range(3)]
    phi = rng.random(ids.size) * 2 - 1
    model = dict(curl=lambda f: [VM.curl(ids, base, 0, periodic, L, f).value[:, k] for k in range(3)],
                 grad=lambda p: [GM.gradient(ids, base, 0, periodic, L, p).grad[:, d] for d in range(3)],
                 divergence=lambda f: VM.divergence(ids, base, 0, periodic, L, f).value,
                 curl_of_grad=lambda f: VM.curl(ids, base, 0, periodic, L, f).value)
    c = VM.curl(ids, base, 0, periodic, L, F)
    assert np.all(np.abs(c.value).max(axis=0) > 0.1)  # the curl itself is not small
    wd, wc = second_order_identities(ids, base, periodic, L, F, phi, **model)
    print(geometry, base, periodic, f"div(curl) {wd:.3f} and curl(grad) {wc:.3f} of the bound 8 * 2^-52 * S")
    assert wd <= 1.0 and wc <= 1.0


def test_axpy_and_previous_contents():
    rng = np.random.default_rng(2)
    x, y = rng.random(7) * 2 - 1, rng.random(7) * 2 - 1
    got = VM.axpy(y, 0.37, x)
    assert got.tolist() == [float(np.float64(y[i]) + np.float64(np.float64(0.37) * np.float64(x[i]))) for i in range(7)]
    # accumulate: the previous content plus the scaled value, the scaled value being the plain call's
    base, periodic = (4, 3, 2), (True, False, True)
    ids, L, _ = _mesh(base, None)
    F = [rng.random(ids.size) * 2 - 1 for _ in range(3)]
    prev = [rng.random(ids.size) for _ in range(3)]
    plain = VM.curl(ids, base, 0, periodic, L, F, -0.5)
    acc = VM.curl(ids, base, 0, periodic, L, F, -0.5, prev)
    assert all(np.array_equal(acc.value[:, k], prev[k] + plain.value[:, k]) for k in range(3))
    # z has two cells and is periodic: both z-sides are one cell, D_2 = 0, so r_0 = D_1(F_2), r_1 = -D_0(F_2)
    G = VM.derivatives(ids, base, 0, periodic, L, F)
    assert not G[0].grad[:, 2].any() and np.array_equal(VM.curl_of(G).value[:, 0], G[2].grad[:, 1] - 0.0)
    d = VM.divergence(ids, base, 0, periodic, L, F, 2.0, prev[0])
    assert np.array_equal(d.value, prev[0] + 2.0 * ((G[0].grad[:, 0] + G[1].grad[:, 1]) + G[2].grad[:, 2]))
