"""tests/gradient_model.py pinned before the GPU tests rely on it.

* Consistency: for phi = x_d and phi = x_d^2 of the cell centers the model's
  d-component equals 1 and 2 x_c within 8 * 2^-52 * M on every cell with both
  d-neighbors inside the grid, on refined Cartesian and stretched meshes,
  across level jumps (the stencil's weights are the quadratic fit's through
  the three centers; a finer group's mean has the group's common coordinate).
  A neighbor across a periodic wrap is no sample of x_d, so cells at the
  grid's edge along d are left out there.  Only the own-coordinate component
  is claimed: a coarser neighbor's center is laterally offset.
* No self-force: on a uniform periodic grid the sum over cells of
  (A phi)(grad_d phi) is zero, A being poisson_stretched_model.cache's
  operator.  With power-of-two lengths and small dyadic phi every operation
  is exact, so the sum is exactly 0.
* One-sided and missing sides, the own-neighbor cell, the scale.
"""
import math

import numpy as np
import pytest

import advection_model as AM
import gradient_model as GM
import poisson_stretched_model as PM
import stretched_solver_cases as SC

EPS = 2.0 ** -52
ODD_START, ODD_L0 = (0.1, -0.3, 0.2), (0.3, 0.7, 1.1)
REFINED = dict(length=(4, 4, 4), R=2, periodic=(True, False, True), rounds=2, frac=0.15)


def _cartesian_mesh():
    c = REFINED
    ids = np.sort(SC.oracle_mesh(c).cells()[0])
    lvl, lo, size = AM.boxes(ids, c["length"], c["R"])
    L = GM.cartesian_lengths(ODD_L0, lvl)
    fin = np.array(ODD_L0) / (1 << c["R"])  # the finest cell's length
    ctr = np.array(ODD_START) + (lo + 0.5 * size[:, None]) * fin
    return c, ids, lvl, L, ctr


def _stretched_mesh(name):
    c = SC.case(name)
    ids = np.sort(SC.oracle_mesh(c).cells()[0])
    lvl, ctr, L = PM.geometry(c["coords"], c["length"], c["R"], ids)
    return c, ids, lvl, L, ctr


def _inside(ids, c, d):
    """Cells whose two d-neighbors are not across a wrap."""
    _, lo, size = AM.boxes(ids, c["length"], c["R"])
    ext = c["length"][d] << c["R"]
    return (lo[:, d] > 0) & (lo[:, d] + size < ext)


@pytest.mark.parametrize("mesh", ["cartesian", "exact", "rounded"])
def test_linear_and_quadratic_are_exact(mesh):
    c, ids, lvl, L, ctr = _cartesian_mesh() if mesh == "cartesian" else _stretched_mesh(mesh)
    assert len(set(lvl.tolist())) > 1
    jumps = 0
    for d in range(3):
        x = ctr[:, d]
        sel = _inside(ids, c, d)
        for phi, want in ((x, np.ones(ids.size)), (x * x, 2.0 * x)):
            G = GM.gradient(ids, c["length"], c["R"], c["periodic"], L, phi)
            ok = sel & G.both[:, d]
            assert ok.sum() > ids.size // 4
            err = np.abs(G.grad[ok, d] - want[ok])
            bound = 8 * EPS * G.M[ok, d]
            print(mesh, d, "worst error / bound", float(np.max(err / bound)))
            assert np.all(err <= bound)
            jumps += int(np.sum(G.finer[ok, d]))
    assert jumps > 0  # finer groups took part


def test_no_self_force_on_a_uniform_periodic_grid():
    base, R, periodic = (6, 5, 4), 0, (True, True, True)
    ids = np.arange(1, 6 * 5 * 4 + 1, dtype=np.uint64)
    lvl = np.zeros(ids.size, np.int64)
    L = GM.cartesian_lengths((0.5, 0.25, 2.0), lvl)
    rng = np.random.default_rng(11)
    phi = rng.integers(-64, 65, ids.size) / 8.0
    ch = PM.cache(ids, base, R, periodic, lvl, L, np.zeros(ids.size, np.int64))
    c, dr, nb = (ch.kept[:, k] for k in range(3))
    A = ch.sf * phi
    np.add.at(A, c, ch.f[c, dr] * phi[nb])
    G = GM.gradient(ids, base, R, periodic, L, phi)
    assert np.any(A != 0) and np.all(G.both) and not np.any(G.finer)
    for d in range(3):
        assert np.any(G.grad[:, d] != 0)
        assert math.fsum(A * G.grad[:, d]) == 0.0


def test_sides_and_scale():
    """3 x 1 x 1, x open, y periodic (the cell is its own neighbor), z open."""
    base, periodic = (3, 1, 1), (False, True, False)
    ids = np.array([1, 2, 3], np.uint64)
    L = GM.cartesian_lengths((0.5, 1.0, 2.0), np.zeros(3, np.int64))
    phi = np.array([1.0, 4.0, -2.0])
    G = GM.gradient(ids, base, 0, periodic, L, phi, scale=-2.0)
    assert np.array_equal(G.grad[:, 0], -2.0 * np.array([(4.0 - 1.0) / 0.5, 1.0 * 3.0 + 1.0 * -6.0, (-2.0 - 4.0) / 0.5]))
    assert np.array_equal(G.both, [[False, True, False], [True, True, False], [False, True, False]])
    assert not G.grad[:, 1:].any() and not G.M[:, 2].any()
    assert np.array_equal(G.M[:, 0], [(4.0 + 1.0) / 0.5, 1.0 * (2.0 + 4.0) + 1.0 * (4.0 + 1.0), (4.0 + 2.0) / 0.5])
