"""dccrgx_curl, dccrgx_divergence and dccrgx_field_axpy (curl_kernel,
divergence_kernel, field_axpy_kernel in dccrg_amd/csrc/field_ops.hip).

The main check is bitwise: the header defines both operators on top of
dccrgx_gradient's derivative D_d(F), one IEEE operation per step, so a call
must give exactly what NumPy combines from Dccrg.gradient(F_k, ..., 1.0)
outputs in the contract's order - also where a group of four finer cells took
part, since the group is summed in the gradient kernel's order.

Against tests/vector_calculus_model.py (pinned by
test_vector_calculus_model_cpu.py) an output in which no finer group took part
is bitwise the model's.  With a finer group the kernel's sum of the group has
its own order.  Counted as test_gpu_gradient.py counts, in half-units 2^-53
of a derivative's magnitude M_i: three additions for the group, one
difference, one product, one sum, and the model's own half unit for its
exactly rounded group: 7 per derivative.  A curl component adds its difference
and its scaling, one half-unit of M_1 + M_2 each: 9 half-units, rounded up to
5 * 2^-52 * |scale| * (M_1 + M_2).  The divergence adds two sums and the
scaling to its three derivatives: 10 half-units,
5 * 2^-52 * |scale| * (M_0 + M_1 + M_2).  A miss is a bug, not noise."""
import numpy as np
import pytest

import gradient_model as GM
import poisson_stretched_model as PM
import stretched_solver_cases as SC
import vector_calculus_model as VM
from helpers import make_pair
from test_vector_calculus_model_cpu import second_order_identities

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ODD_START, ODD_L0 = (0.1, -0.3, 0.2), (0.3, 0.7, 1.1)  # the gradient tests'
SENTINEL = -7.5
NEXT = (1, 2, 0)
REFINED = dict(length=(4, 4, 4), R=2, periodic=(True, False, True), hood=1, rounds=2, frac=0.15)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _values(n, seed):
    return np.random.default_rng(seed).random(n) * 2 - 1


class Case:
    """A grid (or a detached view of one process), the whole mesh's sorted
    ids, the position of every slot in them, three input fields set in every
    slot (remote copies included), the outputs and three scratch fields for
    the composition.  `lengths` gives the model's per-cell lengths."""

    def __init__(self, g, o, base, R, periodic, lengths, seed=1):
        self.g, self.base, self.R, self.periodic = g, base, R, periodic
        self.ids = np.sort(o.cells()[0])
        self.at = np.searchsorted(self.ids, g.slot_ids())
        self.L = lengths(self.ids)
        self.F = [_values(self.ids.size, seed + 100 * j) for j in range(3)]
        self.f = [g.add_field(f"F{j}", np.float64) for j in range(3)]
        for f, v in zip(self.f, self.F):
            f.set(v[self.at])
        self.out = [g.add_field(n, np.float64) for n in ("cx", "cy", "cz")]
        self.dv = g.add_field("dv", np.float64)
        self.tmp = [g.add_field(n, np.float64) for n in ("gx", "gy", "gz")]
        self._G = None

    def fill(self, prev=None):
        """The four outputs' slots, remote copies included: the sentinel, or
        prev[k] (k = 3: the divergence's)."""
        for k, f in enumerate(self.out + [self.dv]):
            f.set(np.full(self.g.n_slots, SENTINEL) if prev is None else prev[k])

    def derivatives(self):
        """D[j][d] of the local slots from nine gradient outputs at scale 1.0."""
        nl = self.g.n_local
        D = []
        for f in self.f:
            self.g.gradient(f, self.tmp, 1.0)
            D.append([t.get(0, nl) for t in self.tmp])
        return D

    def model(self):
        """The model's derivatives of the whole mesh (computed once)."""
        if self._G is None:
            self._G = VM.derivatives(self.ids, self.base, self.R, self.periodic, self.L, self.F)
        return self._G


def composed_curl(D, k, scale, prev=None):
    d1 = NEXT[k]
    d2 = NEXT[d1]
    r = D[d2][d1] - D[d1][d2]
    t = np.float64(scale) * r
    return t if prev is None else prev + t


def composed_divergence(D, scale, prev=None):
    r = (D[0][0] + D[1][1]) + D[2][2]
    t = np.float64(scale) * r
    return t if prev is None else prev + t


# ---- the grids of test_gpu_gradient.py -----------------------------------------------
def _uniform(length, periodic):
    g, o = make_pair(length, 0, periodic, 1)
    g.set_geometry(ODD_START, ODD_L0)
    return Case(g, o, length, 0, periodic, lambda ids: GM.cartesian_lengths(ODD_L0, np.zeros(ids.size, np.int64)))


def _refined(seed, nprocs=1, rank=0, periodic=None):
    c = dict(REFINED, periodic=periodic or REFINED["periodic"])
    g, o = make_pair(c["length"], c["R"], c["periodic"], c["hood"], c["rounds"], c["frac"], seed=seed, nprocs=nprocs,
                     rank=rank)
    g.set_geometry(ODD_START, ODD_L0)
    return Case(g, o, c["length"], c["R"], c["periodic"],
                lambda ids: GM.cartesian_lengths(ODD_L0, GM.levels(ids, c["length"], c["R"])), seed + 10)


def _stretched(coords_only_as_block, length=(4, 4, 4), R=1, periodic=(True, False, True)):
    from oracle import oracle as O

    coords = SC.uneven_coords(length, 21)
    g, o = make_pair(length, R, periodic, 1, 1 if R else 0, 0.15)
    if coords_only_as_block:
        # what load_grid_data leaves of a file with such a block: each dimension's
        # start and first cell length as the library's own geometry, and the bytes
        g.set_geometry([c[0] for c in coords], [c[1] - c[0] for c in coords])
        g.set_geometry_block(O.stretched_geometry_block(coords))
        return Case(g, o, length, R, periodic, lambda ids: PM.fallback_lengths(coords, GM.levels(ids, length, R)), 5)
    g.set_stretched_geometry(coords)
    return Case(g, o, length, R, periodic, lambda ids: GM.stretched_lengths(coords, length, R, ids), 5)


GRIDS = {
    "uniform-4x3x2-open": lambda: _uniform((4, 3, 2), (False, False, False)),
    "uniform-4x3x2-pop": lambda: _uniform((4, 3, 2), (True, False, True)),
    "one-cell-open": lambda: _uniform((1, 1, 1), (False, False, False)),
    "one-cell-periodic": lambda: _uniform((1, 1, 1), (True, True, True)),
    "blocks-17x13x11": lambda: _uniform((17, 13, 11), (True, False, True)),  # 2431 slots: 10 blocks rounded to 16
    "refined-seed0-pop": lambda: _refined(0, periodic=(True, False, True)),
    "refined-seed1-opo": lambda: _refined(1, periodic=(False, True, False)),
    "stretched": lambda: _stretched(False),
    "file-block-without-coordinates": lambda: _stretched(True),
}


def _check_model(c, got_curl, got_div, scale, expect_finer):
    """The local slots of a plain (not accumulating) call against the model."""
    nl = c.g.n_local
    G = c.model()
    sel = c.at[:nl]
    cu, dv = VM.curl_of(G, scale), VM.divergence_of(G, scale)
    assert bool(cu.finer.any()) == expect_finer and bool(dv.finer.any()) == expect_finer
    worst = 0.0
    for got, want, M, finer in [(got_curl[k], cu.value[sel, k], cu.M[sel, k], cu.finer[sel, k]) for k in range(3)] + [
            (got_div, dv.value[sel], dv.M[sel], dv.finer[sel])]:
        assert _same(got[~finer], want[~finer]), np.flatnonzero(got[~finer] != want[~finer])[:5]
        bound = 5 * EPS * abs(scale) * M[finer]
        err = np.abs(got[finer] - want[finer])
        if err.size:
            worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1))))
        assert np.all(err <= bound), float(np.max(err / np.where(bound > 0, bound, 1)))
    print(f"finer groups: worst error {worst:.3f} of its bound")


@pytest.mark.parametrize("grid", list(GRIDS))
def test_bitwise_against_the_composition_and_against_the_model(gpu, grid):
    c = GRIDS[grid]()
    g, nl, ns = c.g, c.g.n_local, c.g.n_slots
    if grid == "blocks-17x13x11":
        assert nl == 2431
    refined = grid.startswith("refined")
    if refined:
        assert set(GM.levels(c.ids, c.base, c.R).tolist()) == {0, 1, 2}
    D = c.derivatives()
    rng = np.random.default_rng(9)
    for scale in (-1.0, 0.37):
        for accumulate in (False, True):
            prev = [rng.random(ns) * 2 - 1 for _ in range(4)] if accumulate else None
            c.fill(prev)
            g.curl(c.f, c.out, scale, accumulate)
            g.divergence(c.f, c.dv, scale, accumulate)
            got = [f.get(0, nl) for f in c.out]
            for k in range(3):
                want = composed_curl(D, k, scale, prev[k][:nl] if accumulate else None)
                assert _same(got[k], want), (scale, accumulate, k, np.flatnonzero(got[k] != want)[:5])
            want = composed_divergence(D, scale, prev[3][:nl] if accumulate else None)
            assert _same(c.dv.get(0, nl), want), (scale, accumulate, np.flatnonzero(c.dv.get(0, nl) != want)[:5])
            if not accumulate and scale == 0.37:
                _check_model(c, got, c.dv.get(0, nl), scale, expect_finer=c.R > 0)
                if grid.startswith("one-cell"):
                    assert all(_same(x, np.zeros(1)) for x in got + [c.dv.get(0, 1)])
    # the inputs are read only
    for f, v in zip(c.f, c.F):
        assert _same(f.get(), v[c.at])
    g.close()


def test_inputs_need_not_be_distinct(gpu):
    """curl(F, F, F) and div(F, F, F) from one field's three derivatives."""
    c = GRIDS["refined-seed0-pop"]()
    nl = c.g.n_local
    c.g.gradient(c.f[0], c.tmp, 1.0)
    d = [t.get(0, nl) for t in c.tmp]
    D = [d, d, d]
    c.fill()
    c.g.curl([c.f[0]] * 3, c.out, 0.37)
    c.g.divergence([c.f[0]] * 3, c.dv, 0.37)
    for k in range(3):
        assert _same(c.out[k].get(0, nl), composed_curl(D, k, 0.37))
    assert _same(c.dv.get(0, nl), composed_divergence(D, 0.37))
    c.g.close()


# ---- div(curl F) and curl(grad phi) on the device --------------------------------------
@pytest.mark.parametrize("geometry,periodic", [("cartesian", (True, False, True)), ("cartesian", (False, False, False)),
                                               ("stretched", (True, False, True))])
def test_div_curl_and_curl_grad_vanish_to_rounding(gpu, geometry, periodic):
    """Unrefined 4 x 3 x 5 under test_vector_calculus_model_cpu.py's bound
    8 * 2^-52 * S, S from the model."""
    base = (4, 3, 5)
    c = _stretched(False, base, 0, periodic) if geometry == "stretched" else _uniform(base, periodic)
    g, nl = c.g, c.g.n_local
    assert nl == c.ids.size == 60
    phi = _values(60, 77)
    order = np.argsort(c.at)  # slot of every position in the sorted ids

    def put(fields, values):
        for f, v in zip(fields, values):
            f.set(np.asarray(v)[c.at])

    def curl(F):
        put(c.f, F)
        g.curl(c.f, c.out)
        return [f.get(0, nl)[order] for f in c.out]

    def divergence(F):
        put(c.tmp, F)
        g.divergence(c.tmp, c.dv)
        return c.dv.get(0, nl)[order]

    def grad(p):
        put(c.f[:1], [p])
        g.gradient(c.f[0], c.tmp, 1.0)
        return [f.get(0, nl)[order] for f in c.tmp]

    def curl_of_grad(F):
        put(c.tmp, F)
        g.curl(c.tmp, c.out)
        return np.stack([f.get(0, nl)[order] for f in c.out], axis=1)

    first = curl(c.F)
    assert all(np.abs(x).max() > 0.1 for x in first)  # the curl itself is not small
    wd, wc = second_order_identities(c.ids, base, periodic, c.L, c.F, phi, curl, grad, divergence, curl_of_grad)
    print(geometry, periodic, f"div(curl) {wd:.3f} and curl(grad) {wc:.3f} of the bound 8 * 2^-52 * S")
    assert wd <= 1.0 and wc <= 1.0
    g.close()


# ---- detached views of several processes -----------------------------------------------
@pytest.mark.parametrize("nprocs,rank", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_views_of_several_processes(gpu, nprocs, rank):
    c = _refined(0, nprocs, rank)
    g = c.g
    nl, nr, ns = g.n_local, g.n_slots - g.n_local, g.n_slots
    ni = g.counts["inner"]
    # (the middle one of three processes has no inner cell: an empty region)
    assert nr > 0 and ni < nl and (ni > 0) == ((nprocs, rank) != (3, 1))
    c.fill()
    g.curl(c.f, c.out, 0.37)
    g.divergence(c.f, c.dv, 0.37)
    whole = [f.get(0, nl) for f in c.out + [c.dv]]
    _check_model(c, whole[:3], whole[3], 0.37, expect_finer=True)
    for f in c.out + [c.dv]:
        assert np.all(f.get(nl, nr) == SENTINEL)  # remote copies' slots are not written
    # inner, then outer: the same bits; each region writes its own slots only.  Also when accumulating.
    rng = np.random.default_rng(4)
    for accumulate in (False, True):
        prev = [rng.random(ns) * 2 - 1 for _ in range(4)] if accumulate else [np.full(ns, SENTINEL)] * 4
        c.fill(prev)
        g.curl(c.f, c.out, 0.37, accumulate)
        g.divergence(c.f, c.dv, 0.37, accumulate)
        whole = [f.get(0, nl) for f in c.out + [c.dv]]
        c.fill(prev)
        g.curl(c.f, c.out, 0.37, accumulate, region="inner")
        g.divergence(c.f, c.dv, 0.37, accumulate, region="inner")
        for k, f in enumerate(c.out + [c.dv]):
            assert _same(f.get(0, ni), whole[k][:ni]) and _same(f.get(ni, ns - ni), prev[k][ni:])
        g.curl(c.f, c.out, 0.37, accumulate, region="outer")
        g.divergence(c.f, c.dv, 0.37, accumulate, region="outer")
        for k, f in enumerate(c.out + [c.dv]):
            assert _same(f.get(0, nl), whole[k]) and _same(f.get(nl, nr), prev[k][nl:])
    # a component that is not wanted is not touched
    c.fill()
    g.curl(c.f, c.out, 0.37)
    whole = [f.get(0, nl) for f in c.out]
    c.fill()
    g.curl(c.f, [c.out[0], None, c.out[2]], 0.37)
    assert _same(c.out[0].get(0, nl), whole[0]) and _same(c.out[2].get(0, nl), whole[2])
    assert np.all(c.out[1].get() == SENTINEL)
    c.fill()
    g.curl(c.f, [None, c.out[1], None], 0.37)
    assert _same(c.out[1].get(0, nl), whole[1])
    assert np.all(c.out[0].get() == SENTINEL) and np.all(c.out[2].get() == SENTINEL)
    g.close()


# ---- field_axpy ------------------------------------------------------------------------
def test_field_axpy_is_bitwise(gpu):
    c = GRIDS["blocks-17x13x11"]()
    g, ns = c.g, c.g.n_slots
    assert g.n_local == ns == 2431
    x, y = c.f[0], c.out[0]
    xv, yv = _values(ns, 31), _values(ns, 32)
    x.set(xv)
    y.set(yv)
    g.field_axpy(y, 0.37, x)
    want = VM.axpy(yv, 0.37, xv)
    assert _same(y.get(), want) and _same(x.get(), xv)
    g.field_axpy(y, -1.5, x)
    assert _same(y.get(), VM.axpy(want, -1.5, xv))
    g.close()


@pytest.mark.parametrize("nprocs,rank", [(2, 0), (3, 1), (3, 2)])
def test_field_axpy_regions_and_remote_copies(gpu, nprocs, rank):
    """Odd and even region boundaries: the 16-byte pairs start at the first
    even slot, a leading and a trailing single slot go on their own."""
    c = _refined(0, nprocs, rank)
    g = c.g
    nl, ns, ni = g.n_local, g.n_slots, g.counts["inner"]
    assert ns > nl
    x, y = c.f[0], c.out[0]
    xv, yv = c.F[0][c.at], _values(ns, 41)
    want = VM.axpy(yv, 0.37, xv)
    y.set(yv)
    g.field_axpy(y, 0.37, x)
    assert _same(y.get(0, nl), want[:nl]) and _same(y.get(nl, ns - nl), yv[nl:])  # remote copies are not written
    y.set(yv)
    g.field_axpy(y, 0.37, x, region="inner")
    assert _same(y.get(0, ni), want[:ni]) and _same(y.get(ni, ns - ni), yv[ni:])
    g.field_axpy(y, 0.37, x, region="outer")
    assert _same(y.get(0, nl), want[:nl]) and _same(y.get(nl, ns - nl), yv[nl:])
    assert _same(x.get(), xv)
    g.close()


# ---- refusals --------------------------------------------------------------------------
def test_refusals(gpu):
    import ctypes as C
    import types

    from dccrg_amd._lib import EINVAL, lib

    c = _uniform((4, 3, 2), (False, False, False))
    g = c.g
    u32 = g.add_field("u32", np.uint32)
    var = g.add_variable_field("var", np.float64, False)
    bad = types.SimpleNamespace(id=99)
    f0, f1, f2 = c.f
    cx, cy, cz = c.out
    c.fill()
    calls = [
        (lambda: g.curl([var, f1, f2], c.out), "variable-size"),
        (lambda: g.curl(c.f, [cx, var, cz]), "variable-size"),
        (lambda: g.curl([f0, u32, f2], c.out), "8-byte"),
        (lambda: g.curl(c.f, [cx, cy, u32]), "8-byte"),
        (lambda: g.curl([f0, f1, bad], c.out), "invalid field id"),
        (lambda: g.curl(c.f, [cx, bad, cz]), "invalid field id"),
        (lambda: g.curl(c.f, [cx, f2, cz]), "is an input"),
        (lambda: g.curl(c.f, [f0, None, None]), "is an input"),
        (lambda: g.curl(c.f, [cx, cy, cx]), "one field"),
        (lambda: g.curl(c.f, [None, cy, cy]), "one field"),
        (lambda: g.curl(c.f, [None, None, None]), "all three"),
        (lambda: g.divergence([f0, var, f2], c.dv), "variable-size"),
        (lambda: g.divergence(c.f, var), "variable-size"),
        (lambda: g.divergence([u32, f1, f2], c.dv), "8-byte"),
        (lambda: g.divergence(c.f, u32), "8-byte"),
        (lambda: g.divergence([f0, f1, bad], c.dv), "invalid field id"),
        (lambda: g.divergence(c.f, bad), "invalid field id"),
        (lambda: g.divergence(c.f, f1), "is an input"),
        (lambda: g.field_axpy(cx, 2.0, var), "variable-size"),
        (lambda: g.field_axpy(var, 2.0, f0), "variable-size"),
        (lambda: g.field_axpy(cx, 2.0, u32), "8-byte"),
        (lambda: g.field_axpy(u32, 2.0, f0), "8-byte"),
        (lambda: g.field_axpy(cx, 2.0, bad), "invalid field id"),
        (lambda: g.field_axpy(bad, 2.0, f0), "invalid field id"),
        (lambda: g.field_axpy(cx, 2.0, cx), "one field"),
    ]
    for call, match in calls:
        with pytest.raises(Exception, match=match) as e:
            call()
        assert e.value.code == EINVAL
    fin = (C.c_int * 3)(f0.id, f1.id, f2.id)
    ids = (C.c_int * 3)(cx.id, cy.id, cz.id)
    for region in (-1, 3):
        for accumulate in (0, 1):
            assert lib().dccrgx_curl(g.h, fin, ids, 1.0, accumulate, region) == EINVAL
            assert lib().dccrgx_divergence(g.h, fin, c.dv.id, 1.0, accumulate, region) == EINVAL
        assert lib().dccrgx_field_axpy(g.h, cx.id, 2.0, f0.id, region) == EINVAL
    for f in c.out + [c.dv]:
        assert np.all(f.get() == SENTINEL)  # a refused call writes nothing
    for f, v in zip(c.f, c.F):
        assert _same(f.get(), v[c.at])
    g.close()
