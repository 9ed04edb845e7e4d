"""tests/field_adapt_model.py pinned (no GPU): the model that
test_gpu_field_follow_mesh.py compares the device code with.

- its MEAN restriction is the reference's adapt_grid density on merged
  parents (the oracle's restatement of adapter.hpp:260-290), bitwise;
- under LINEAR the eight children's mean is within 16 * 2^-53 * (|v| + Delta)
  of v: three roundings per child sum and eight of the mean, with slack;
- the children lie within [m, M] up to 8 * 2^-53 * max(|m|, |M|);
- a field linear in position, on cells with same-level neighbors on both
  sides, is not limited (alpha = 1: sum |e_d| <= 3/4 max |dv| there) and the
  children take the exact values at their centres within rounding;
- an extremum is injected."""
import math

import numpy as np

import advection_model as AM
import field_adapt_model as FM
import gradient_model as GM
from helpers import random_refines
from oracle import oracle as O

U = 2.0 ** -53


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_mean_is_the_oracles_adapt_density():
    base, R = (10, 10, 3), 2
    o = O.Grid(base, R, (True, True, False), 0, 1)
    o.set_geometry((0, 0, 0), tuple(1.0 / b for b in base))
    o.adv_prerefine(0.025, 0.25)
    di = 0.025 / R
    parents = children = 0
    for _ in range(15):
        dt = 0.5 * o.adv_max_time_step()
        o.adv_check(di)
        o.adv_steps(1, dt)
        old = np.sort(o.cells()[0])
        rho = o.adv_get(old)[:, 0]
        o.adv_adapt()
        new = np.sort(o.cells()[0])
        F = FM.follow(old, new, base, R, (True, True, False), None, rho, None, "mean")
        assert _same(F.values, o.adv_get(new)[:, 0])
        parents += int((F.kind == 2).sum())
        children += int((F.kind == 1).sum())
    assert parents > 0 and children > 0


def _refined_case(seed, periodic):
    base, R = (4, 4, 4), 2
    o = O.Grid(base, R, periodic, 1, 1)
    rng = np.random.default_rng(seed)
    for _ in range(2):
        ids = o.cells()[0]
        for c in random_refines(ids, o.mapping.batch(ids)["level"], R, rng, 0.15):
            o.refine_completely(c)
        o.stop_refining()
    old = np.sort(o.cells()[0])
    lv = o.mapping.batch(old)["level"]
    for c in random_refines(old, lv, R, rng, 0.2):
        o.refine_completely(c)
    o.stop_refining()
    return base, R, old, np.sort(o.cells()[0]), rng


def test_linear_children_keep_the_mean_and_the_bounds():
    for seed, periodic in ((0, (True, True, True)), (1, (False, True, False))):
        base, R, old, new, rng = _refined_case(seed, periodic)
        val = rng.random(old.size) * 2 - 1
        L = GM.cartesian_lengths((0.3, 0.7, 1.1), GM.levels(old, base, R))
        D = GM.gradient(old, base, R, periodic, L, val).grad
        F = FM.follow(old, new, base, R, periodic, L, val, D, "linear")
        lvl, lo, _ = AM.boxes(old, base, R)
        at = {int(c): i for i, c in enumerate(new)}
        limited = 0
        assert len(F.limiter) > 10
        for p, (v, m, M, delta, alpha, t) in F.limiter.items():
            i = int(np.searchsorted(old, np.uint64(p)))
            ch = [F.values[at[k]] for k in FM.children_of(base, R, int(lvl[i]), lo[i])]
            assert abs(math.fsum(ch) / 8.0 - v) <= 16 * U * (abs(v) + delta)
            tol = 8 * U * max(abs(m), abs(M))
            assert min(ch) >= m - tol and max(ch) <= M + tol
            assert 0.0 <= alpha <= 1.0
            limited += alpha < 1.0
        assert 0 < limited


def test_linear_field_is_reproduced_exactly():
    base, R, periodic = (4, 4, 4), 1, (False, False, False)
    l0, start = (0.3, 0.7, 1.1), (0.1, -0.3, 0.2)
    o = O.Grid(base, R, periodic, 1, 1)
    old = np.sort(o.cells()[0])
    _, lo, size = AM.boxes(old, base, R)
    ctr = np.asarray(start) + (lo + 0.5 * size[:, None]) / 2.0 * np.asarray(l0)
    a, b = np.array([0.7, -1.3, 0.4]), 0.25
    val = ctr @ a + b
    inner = [int(c) for c, x in zip(old, lo // 2) if np.all((x >= 1) & (x <= 2))]
    assert len(inner) == 8
    for c in inner:
        o.refine_completely(c)
    o.stop_refining()
    new = np.sort(o.cells()[0])
    assert new.size == old.size + 7 * 8  # nothing induced
    L = GM.cartesian_lengths(l0, np.zeros(old.size, np.int64))
    G = GM.gradient(old, base, R, periodic, L, val)
    F = FM.follow(old, new, base, R, periodic, L, val, G.grad, "linear")
    assert sorted(F.limiter) == inner
    _, nlo, nsize = AM.boxes(new, base, R)
    nctr = np.asarray(start) + (nlo + 0.5 * nsize[:, None]) / 2.0 * np.asarray(l0)
    exact = nctr @ a + b
    scale = np.abs(nctr) @ np.abs(a) + abs(b)
    for p, (v, m, M, delta, alpha, t) in F.limiter.items():
        assert alpha == 1.0
    sel = F.kind == 1
    assert sel.sum() == 64
    assert np.all(np.abs(F.values[sel] - exact[sel]) <= 16 * 2 * U * scale[sel])
    assert _same(F.values[~sel], exact[~sel])


def test_an_extremum_is_injected():
    base, R, periodic = (3, 3, 3), 1, (True, False, True)
    o = O.Grid(base, R, periodic, 1, 1)
    old = np.sort(o.cells()[0])
    rng = np.random.default_rng(3)
    L = GM.cartesian_lengths((1.0, 1.0, 1.0), np.zeros(old.size, np.int64))
    for sign in (1.0, -1.0):
        val = rng.random(old.size)
        val[13] = sign * 5.0  # the middle cell, above (below) all its neighbors
        o2 = O.Grid(base, R, periodic, 1, 1)
        o2.refine_completely(int(old[13]))
        o2.stop_refining()
        new = np.sort(o2.cells()[0])
        G = GM.gradient(old, base, R, periodic, L, val)
        assert np.any(G.grad[13] != 0)
        F = FM.follow(old, new, base, R, periodic, L, val, G.grad, "linear")
        v, m, M, delta, alpha, t = F.limiter[int(old[13])]
        assert alpha == 0.0 and delta > 0
        assert _same(F.values[F.kind == 1], np.full(8, sign * 5.0))


def test_sum_and_off():
    base, R, periodic = (2, 2, 2), 1, (False, False, False)
    o = O.Grid(base, R, periodic, 1, 1)
    lv0 = np.sort(o.cells()[0])
    o.refine_completely(3)
    o.stop_refining()
    lv1 = np.sort(o.cells()[0])
    val = np.arange(1.0, 9.0)
    down = FM.follow(lv0, lv1, base, R, periodic, None, val, None, "sum")
    assert _same(down.values[down.kind == 1], np.full(8, 3.0 * 0.125)) and (down.kind == 1).sum() == 8
    up = FM.follow(lv1, lv0, base, R, periodic, None, down.values, None, "sum")
    assert _same(up.values, val) and (up.kind == 2).sum() == 1
    off = FM.follow(lv1, lv0, base, R, periodic, None, down.values, None, None)
    assert off.values[2] == 0.0 and _same(np.delete(off.values, 2), np.delete(val, 2))
    child = FM.follow(lv0, lv1, base, R, periodic, None, val, None, None)
    assert _same(child.values[child.kind == 1], np.full(8, 3.0))
