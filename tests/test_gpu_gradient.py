"""dccrgx_gradient (gradient_kernel, dccrg_amd/csrc/field_ops.hip)
against tests/gradient_model.py, which test_gradient_model_cpu.py pins.

Both sides evaluate the header's contract one IEEE operation at a time, so a
component in which no group of four finer cells took part is bitwise the
model's.  With a finer group only the order of the group's sum is the
kernel's: three additions for the group, one difference, one product, one sum
and one scaling, plus the model's own half unit, stay under 8 half-units of
the magnitude M the model returns, so the bound is 4 * 2^-52 * |scale| * M.
A miss is a bug, not noise."""
import numpy as np
import pytest

import gradient_model as GM
import poisson_stretched_model as PM
import stretched_solver_cases as SC
from helpers import make_pair

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ODD_START, ODD_L0 = (0.1, -0.3, 0.2), (0.3, 0.7, 1.1)  # the deposit tests'
SENTINEL = -7.5


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _values(n, seed):
    return np.random.default_rng(seed).random(n) * 2 - 1


class Case:
    """A grid (or a detached view of one process), the whole mesh's sorted
    ids, the position of every slot in them, and the input field set in
    every slot, remote copies included."""

    def __init__(self, g, o, seed=1):
        self.g = g
        self.ids = np.sort(o.cells()[0])
        self.at = np.searchsorted(self.ids, g.slot_ids())
        self.phi = _values(self.ids.size, seed)
        self.f = g.add_field("phi", np.float64)
        self.f.set(self.phi[self.at])
        self.out = [g.add_field(n, np.float64) for n in ("gx", "gy", "gz")]

    def fill(self, v=SENTINEL):
        for f in self.out:
            f.set(np.full(self.g.n_slots, v))

    def check(self, G, scale, got=None, exact=False):
        """The local slots of the three outputs against the model's result."""
        nl = self.g.n_local
        got = got or [f.get(0, nl) for f in self.out]
        worst = 0.0
        for d in range(3):
            want, M, finer = (a[self.at[:nl], d] for a in (G.grad, G.M, G.finer))
            assert not (exact and finer.any())
            assert _same(got[d][~finer], want[~finer]), (d, np.flatnonzero(got[d][~finer] != want[~finer])[:5])
            bound = 4 * EPS * abs(scale) * M[finer]
            err = np.abs(got[d][finer] - want[finer])
            assert np.all(err <= bound), (d, float(np.max(err / np.where(bound > 0, bound, 1))))
            if err.size:
                worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1))))
        print(f"finer groups: worst error {worst:.3f} of its bound")
        return got


def _uniform(length, periodic, start=ODD_START, l0=ODD_L0):
    g, o = make_pair(length, 0, periodic, 1)
    g.set_geometry(start, l0)
    c = Case(g, o)
    L = GM.cartesian_lengths(l0, np.zeros(c.ids.size, np.int64))
    return c, lambda scale: GM.gradient(c.ids, length, 0, periodic, L, c.phi, scale)


# ---- uniform grids: bitwise ----------------------------------------------------------
@pytest.mark.parametrize("periodic", [(False, False, False), (True, False, True)])
def test_uniform_is_bitwise(gpu, periodic):
    """4 x 3 x 2: with z periodic a cell's two z-sides are one cell."""
    c, model = _uniform((4, 3, 2), periodic)
    for scale in (-1.0, 0.37):
        c.fill()
        c.g.gradient(c.f, c.out, scale)
        G = model(scale)
        assert G.both[:, 2].all() == periodic[2] and not G.both[:, 1].all()
        c.check(G, scale, exact=True)
    c.g.close()


@pytest.mark.parametrize("periodic", [(False, False, False), (True, True, True)])
def test_degenerate_grid_is_all_zeros(gpu, periodic):
    c, model = _uniform((1, 1, 1), periodic)
    c.fill()
    c.g.gradient(c.f, c.out, 0.37)
    for f in c.out:
        assert _same(f.get(0, 1), np.zeros(1))
    c.check(model(0.37), 0.37, exact=True)
    c.g.close()


def test_several_blocks_not_a_multiple_of_eight(gpu):
    """17 x 13 x 11 = 2431 slots, 10 blocks of 256: the launch is rounded up
    to 16 blocks, or the block permutation would write some slots twice and
    skip others."""
    c, model = _uniform((17, 13, 11), (True, False, True))
    assert c.g.n_local == 2431
    c.fill()
    c.g.gradient(c.f, c.out, -1.0)
    c.check(model(-1.0), -1.0, exact=True)
    c.g.close()


# ---- refined and stretched -----------------------------------------------------------
REFINED = dict(length=(4, 4, 4), R=2, periodic=(True, False, True), hood=1, rounds=2, frac=0.15)


def _refined(seed, nprocs=1, rank=0, periodic=None):
    c = dict(REFINED, periodic=periodic or REFINED["periodic"])
    g, o = make_pair(c["length"], c["R"], c["periodic"], c["hood"], c["rounds"], c["frac"], seed=seed, nprocs=nprocs,
                     rank=rank)
    g.set_geometry(ODD_START, ODD_L0)
    case = Case(g, o, seed + 10)
    L = GM.cartesian_lengths(ODD_L0, GM.levels(case.ids, c["length"], c["R"]))
    return case, lambda scale: GM.gradient(case.ids, c["length"], c["R"], c["periodic"], L, case.phi, scale)


@pytest.mark.parametrize("seed,periodic", [(0, (True, False, True)), (1, (False, True, False))])
def test_refined_grid(gpu, seed, periodic):
    c, model = _refined(seed, periodic=periodic)
    G = model(0.37)
    assert G.finer.any() and not G.finer.all() and set(GM.levels(c.ids, (4, 4, 4), 2).tolist()) == {0, 1, 2}
    c.fill()
    c.g.gradient(c.f, c.out, 0.37)
    c.check(G, 0.37)
    c.g.close()


def _stretched(coords_only_as_block):
    from oracle import oracle as O

    length, R, periodic = (4, 4, 4), 1, (True, False, True)
    coords = SC.uneven_coords(length, 21)
    g, o = make_pair(length, R, periodic, 1, 1, 0.15)
    if coords_only_as_block:
        # what load_grid_data leaves of a file with such a block: each dimension's
        # start and first cell length as the library's own geometry, and the bytes
        g.set_geometry([c[0] for c in coords], [c[1] - c[0] for c in coords])
        g.set_geometry_block(O.stretched_geometry_block(coords))
    else:
        g.set_stretched_geometry(coords)
    c = Case(g, o, 5)
    if coords_only_as_block:
        L = PM.fallback_lengths(coords, GM.levels(c.ids, length, R))
    else:
        L = GM.stretched_lengths(coords, length, R, c.ids)
    assert not np.array_equal(L, PM.fallback_lengths(coords, GM.levels(c.ids, length, R))) or coords_only_as_block
    return c, GM.gradient(c.ids, length, R, periodic, L, c.phi, -1.0)


def test_stretched_geometry(gpu):
    c, G = _stretched(False)
    assert G.finer.any()
    c.fill()
    c.g.gradient(c.f, c.out, -1.0)
    c.check(G, -1.0)
    c.g.close()


def test_file_block_without_coordinates_takes_the_fallback_lengths(gpu):
    """As dccrgx_poisson_cache: each dimension's start and first cell length."""
    c, G = _stretched(True)
    c.fill()
    c.g.gradient(c.f, c.out, -1.0)
    c.check(G, -1.0)
    c.g.close()


# ---- detached views of several processes -----------------------------------------------
@pytest.mark.parametrize("nprocs,rank", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_views_of_several_processes(gpu, nprocs, rank):
    c, model = _refined(0, nprocs, rank)
    g = c.g
    nl, nr = g.n_local, g.n_slots - g.n_local
    # (the middle one of three processes has no inner cell: an empty region)
    assert nr > 0 and g.counts["inner"] < nl and (g.counts["inner"] > 0) == ((nprocs, rank) != (3, 1))
    G = model(0.37)
    c.fill()
    g.gradient(c.f, c.out, 0.37)
    whole = c.check(G, 0.37)
    for f in c.out:
        assert np.all(f.get(nl, nr) == SENTINEL)  # remote copies' slots are not written
    # inner, then outer: the same bits; each region writes its own slots only
    c.fill()
    g.gradient(c.f, c.out, 0.37, region="inner")
    ni = g.counts["inner"]
    for d, f in enumerate(c.out):
        assert _same(f.get(0, ni), whole[d][:ni]) and np.all(f.get(ni, g.n_slots - ni) == SENTINEL)
    g.gradient(c.f, c.out, 0.37, region="outer")
    for d, f in enumerate(c.out):
        assert _same(f.get(0, nl), whole[d]) and np.all(f.get(nl, nr) == SENTINEL)
    # a component that is not wanted is not touched
    c.fill()
    g.gradient(c.f, [c.out[0], None, c.out[2]], 0.37)
    assert _same(c.out[0].get(0, nl), whole[0]) and _same(c.out[2].get(0, nl), whole[2])
    assert np.all(c.out[1].get() == SENTINEL)
    g.close()


# ---- refusals --------------------------------------------------------------------------
def test_refusals(gpu):
    import ctypes as C
    import types

    from dccrg_amd._lib import EINVAL, lib

    c, _ = _uniform((4, 3, 2), (False, False, False))
    g = c.g
    u32 = g.add_field("u32", np.uint32)
    var = g.add_variable_field("var", np.float64, False)
    gx, gy, gz = c.out
    c.fill()
    for call, match in ((lambda: g.gradient(var, c.out), "variable-size"),
                        (lambda: g.gradient(c.f, [gx, var, gz]), "variable-size"),
                        (lambda: g.gradient(u32, c.out), "8-byte"),
                        (lambda: g.gradient(c.f, [gx, gy, u32]), "8-byte"),
                        (lambda: g.gradient(c.f, [gx, c.f, gz]), "is the input"),
                        (lambda: g.gradient(c.f, [gx, gy, gx]), "one field"),
                        (lambda: g.gradient(c.f, [None, gy, gy]), "one field"),
                        (lambda: g.gradient(c.f, [None, None, None]), "all three"),
                        (lambda: g.gradient(c.f, [gx, types.SimpleNamespace(id=99), gz]), "invalid field id")):
        with pytest.raises(Exception, match=match) as e:
            call()
        assert e.value.code == EINVAL
    ids = (C.c_int * 3)(gx.id, gy.id, gz.id)
    for region in (-1, 3):
        assert lib().dccrgx_gradient(g.h, c.f.id, ids, 1.0, region) == EINVAL
    for f in c.out:
        assert np.all(f.get() == SENTINEL)  # a refused call writes nothing
    assert _same(c.f.get(), c.phi[c.at])
    g.close()
