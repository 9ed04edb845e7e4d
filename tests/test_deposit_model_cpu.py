"""The deposit / gather model (tests/deposit_model.py) on the CPU: the weight
is a partition of unity on a periodic grid, drops exactly the part of a cloud
past an open face, deposit and gather are adjoint, and grids of one and two
cells per periodic dimension need no special case.  The two C entry points
the model stands for are declared and exported."""
import math

import numpy as np
import pytest

from deposit_model import DepositModel
from oracle import oracle as O
from particles_model import ParticleModel, seeded_particles

EPS = 2.0 ** -52


def _model(length, R, periodic, rounds, seed, start=(0.1, -0.3, 0.2), l0=(0.3, 0.7, 1.1), K=4, per_cell=4):
    o = O.Grid(length, R, periodic, 1, 1)
    rng = np.random.default_rng(seed)
    for _ in range(rounds):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        cand = ids[lv < R]
        for c in rng.choice(cand, max(1, cand.size // 10), replace=False):
            o.refine_completely(int(c))
        o.stop_refining()
    pm = ParticleModel(o, start, l0, K)
    ctr, ln = o.geometry(pm.leaves)
    for c, r in seeded_particles(pm.leaves, ctr, ln, rng, per_cell, K).items():
        pm.set(c, r)
    return pm, DepositModel(pm)


def _share_tolerance(pm):
    """Sum over c of W: every o is a difference of coordinates of magnitude
    <= X (error X 2^-53 each, a handful per dimension) divided by a length
    >= l_min; 64 units cover the three dimensions' operations."""
    X = max(np.max(np.abs(pm.start)), np.max(np.abs(pm.end)))
    return 64 * EPS * X / np.min(pm.cell_len)


@pytest.fixture(scope="module")
def periodic_refined():
    return _model((4, 4, 4), 2, (True, True, True), 2, 31)


def test_refinement_happened(periodic_refined):
    pm, _ = periodic_refined
    lv = pm.o.mapping.batch(pm.leaves)["level"]
    assert set(lv.tolist()) == {0, 1, 2} and pm.total() > 100


def test_shares_sum_to_one_on_a_periodic_grid(periodic_refined):
    pm, dm = periodic_refined
    tol = _share_tolerance(pm)
    worst = 0.0
    for s, rec in pm.cells.items():
        if not rec.shape[0]:
            continue
        total = sum(w for _, w in dm.shares(s, 1))
        worst = max(worst, float(np.max(np.abs(total - 1.0))))
        # the cloud reaches past the holding cell for all but a centred particle
        assert len(dm.shares(s, 1)) > 1
    print("largest |sum W - 1|", worst, "tolerance", tol)
    assert worst <= tol


def test_deposit_conserves_the_charge(periodic_refined):
    pm, dm = periodic_refined
    dep = dm.deposit(1, 3)
    q = np.concatenate([r[:, 3] for r in pm.cells.values()])
    total = math.fsum(v[0] for v in dep.values())
    bound = (4 * EPS + _share_tolerance(pm)) * math.fsum(np.abs(q))
    assert abs(total - math.fsum(q)) <= bound
    ngp = dm.deposit(0, None)
    assert math.fsum(v[0] for v in ngp.values()) == pm.total()
    assert all(v[0] == pm.cells[c].shape[0] for c, v in ngp.items())


def test_open_face_drops_the_share_outside():
    pm, dm = _model((4, 4, 3), 2, (True, True, False), 2, 32)
    tol = _share_tolerance(pm)
    near = far = 0
    for s, rec in pm.cells.items():
        if not rec.shape[0]:
            continue
        lo, L, hi = dm.box[s]
        z = rec[:, 2]
        a, b = z - L[2] / 2, z + L[2] / 2
        inside = (np.minimum(b, pm.end[2]) - np.maximum(a, pm.start[2])) / L[2]
        total = sum(w for _, w in dm.shares(s, 1))
        assert np.all(np.abs(total - inside) <= tol), s
        dist = np.minimum(z - pm.start[2], pm.end[2] - z)
        is_near = dist < L[2] / 2 * (1 - 1e-9)
        is_far = dist > L[2] / 2 * (1 + 1e-9)
        assert np.all(is_near | is_far)
        assert np.all(total[is_near] < 1.0) and np.all(np.abs(total[is_far] - 1.0) <= tol)
        near += int(is_near.sum())
        far += int(is_far.sum())
    assert near > 10 and far > 10


def test_deposit_and_gather_are_adjoint(periodic_refined):
    """sum_c F_c rho_c and sum_p q_p G_p are both the sum of q W F over the
    pairs: each side rounds a correctly rounded inner sum, a product and a
    correctly rounded outer sum, three half units of the sum of |q W F| a
    side."""
    pm, dm = periodic_refined
    rng = np.random.default_rng(33)
    F = {int(c): float(rng.random() * 2 - 1) for c in pm.leaves}
    dep = dm.deposit(1, 3)
    gat = dm.gather([F], 1)
    left = math.fsum(F[c] * v[0] for c, v in dep.items())
    right = math.fsum(float(q) * float(g) for s, (val, _, _) in gat.items()
                      for q, g in zip(pm.cells[s][:, 3], val[:, 0]))
    T = math.fsum(abs(float(q)) * float(m) for s, (_, mag, _) in gat.items()
                  for q, m in zip(pm.cells[s][:, 3], mag[:, 0]))
    print("adjointness", left, right, "bound", 4 * EPS * T)
    assert T > 0 and abs(left - right) <= 4 * EPS * T


@pytest.mark.parametrize("length", [(1, 1, 1), (2, 2, 2), (2, 1, 3), (3, 1, 1)])
def test_one_and_two_cells_per_periodic_dimension(length):
    pm, dm = _model(length, 0, (True, True, True), 0, 34, per_cell=6)
    pm.set(1, np.concatenate([pm.cells[1], [[0.1 + 0.05, -0.3 + 0.1, 0.2 + 1.0, 0.5]]]))  # never empty
    tol = _share_tolerance(pm)
    for s, rec in pm.cells.items():
        if rec.shape[0]:
            total = sum(w for _, w in dm.shares(s, 1))
            assert np.all(np.abs(total - 1.0) <= tol), (s, total)
    dep = dm.deposit(1, 3)
    q = np.concatenate([r[:, 3] for r in pm.cells.values()])
    assert abs(math.fsum(v[0] for v in dep.values()) - math.fsum(q)) <= (4 * EPS + tol) * math.fsum(np.abs(q))
    if length == (1, 1, 1):
        assert dm.candidates(1) == [1]  # its own images are the whole neighborhood


def test_exact_on_dyadic_data():
    """Positions on eighths of the finest cell, q on 2^-10: every share and
    every sum is exact, so the charge is conserved to the bit."""
    pm, dm = _model((4, 4, 4), 2, (True, True, True), 2, 35, start=(0, 0, 0), l0=(1, 1, 1))
    for c, rec in pm.cells.items():
        rec[:, 0:3] = np.round(rec[:, 0:3] * 32) / 32
        rec[:, 3] = np.round(rec[:, 3] * 1024) / 1024
    dep = dm.deposit(1, 3)
    q = np.concatenate([r[:, 3] for r in pm.cells.values()])
    assert math.fsum(v[0] for v in dep.values()) == math.fsum(q)
    for s, rec in pm.cells.items():
        if rec.shape[0]:
            assert np.all(sum(w for _, w in dm.shares(s, 1)) == 1.0)


def test_entry_points_are_declared_and_exported():
    import dccrg_amd

    L = dccrg_amd.lib()
    syms = dccrg_amd.header_symbols()
    for name in ("dccrgx_particles_deposit", "dccrgx_particles_gather"):
        assert name in syms, name
        assert hasattr(L, name), name
    assert L.dccrgx_particles_deposit(None, 0, 4, 1, 3, 0, 0) == dccrg_amd._lib.EINVAL
    assert b"null grid" in L.dccrgx_last_error()
