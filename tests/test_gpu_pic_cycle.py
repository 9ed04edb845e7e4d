"""Three electrostatic particle-in-cell cycles built from the public calls
(particles_deposit, Poisson_Solve, gradient, particles_gather,
particles_accelerate, particles_step) on a 6 x 6 x 6 periodic grid, against
the chain of deposit_model, poisson_stretched_model.solve, gradient_model, a
NumPy accelerate and particles_model.

A particle that lands in another cell because of one unit in the last place
cannot be bounded, so every stage's model takes the device's result of the
stage before it, and every stage is held to its own bound:

* deposit and gather: the bounds of test_gpu_particles_deposit.py;
* gradient: bitwise (a uniform grid has no finer group);
* accelerate and step: bitwise;
* the solved potential (a fixed iteration count, min = max): the bound is not
  fixed in advance.  Each cycle the model solves the same right-hand side
  twice, its global sums taken in ascending and in descending id order; the
  device's reduction tree is a third order, so it may differ from the first
  run by 10 times the gap of those two.  Measured on the model chain alone
  (this grid, these seeds, 10 iterations): gaps of 6.3e-16, 4.8e-16 and
  1.0e-15 of max|phi| in the three cycles, so bounds of 6.3e-15, 4.8e-15 and
  1.0e-14; the test prints the gap, the bound and the device's distance.

It also asserts that no record is lost and that the record count is conserved,
and the adjointness the cycle relies on: sum_p q_p E_p equals
sum_c (rho_c V_c) E_c within the deposit's and the gather's bounds."""
import math

import numpy as np
import pytest

import gradient_model as GM
import poisson_stretched_model as PM
from deposit_model import DepositModel
from particles_model import seeded_particles
from test_gpu_particles import _assert_model, _local_cells, _same
from test_gpu_particles_deposit import ODD_L0, ODD_START, _pair, _upload_all

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
K, Q, E0 = 10, 6, 7  # record: x, v, q, E
BASE, PERIODIC = (6, 6, 6), (True, True, True)
ITERS, DT, CYCLES = 10, 0.5, 3


def seed_records(m, rng):
    ctr, ln = m.o.geometry(m.leaves)
    vmax = 0.3 * m.cell_len / DT  # some records change cell every step
    lx = BASE[0] * ODD_L0[0]
    for c, r in seeded_particles(m.leaves, ctr, ln, rng, 3, K, vmax).items():
        r[:, Q] = 1 + 0.1 * np.cos(2 * np.pi * (r[:, 0] - ODD_START[0]) / lx)
        r[:, E0:E0 + 3] = 0.0
        m.set(c, r)


def rhs_of(rho):
    """-(rho - mean rho): the periodic system needs a zero-mean source."""
    return -(rho - math.fsum(rho) / rho.size)


def solve_both_orders(ch, rhs, monkeypatch):
    """The model's solution with ascending sums, and with descending ones."""
    fwd, it, _ = PM.solve(ch, rhs, np.zeros(rhs.size), ITERS, ITERS)
    with monkeypatch.context() as mp:
        mp.setattr(PM, "_sum", lambda v: sum(reversed(v.tolist()), 0.0))
        rev, rit, _ = PM.solve(ch, rhs, np.zeros(rhs.size), ITERS, ITERS)
    assert it == rit == ITERS
    return fwd["solution"], rev["solution"]


def test_three_cycles(gpu, monkeypatch):
    import dccrg_amd

    g, m, fld = _pair(BASE, start=ODD_START, l0=ODD_L0, K=K)
    seed_records(m, np.random.default_rng(71))
    _upload_all(g, fld, m)
    total = m.total()
    assert total > 216
    ids = np.sort(np.array(m.leaves, np.uint64))
    slots = g.slot_ids()
    assert g.n_local == g.n_slots == ids.size
    at = np.searchsorted(ids, slots)  # position of every slot's cell in ids
    back = np.argsort(at)             # and the slot of every id
    local = [int(c) for c in slots]
    L = GM.cartesian_lengths(ODD_L0, np.zeros(ids.size, np.int64))
    ch = PM.cache(ids, BASE, 0, PERIODIC, np.zeros(ids.size, np.int64), L, np.zeros(ids.size, np.int64))
    rho = g.add_field("rho", np.float64, False)
    g.add_field("rhs", np.float64, False)
    sol = g.add_field("solution", np.float64)
    E = [g.add_field(n, np.float64) for n in ("Ex", "Ey", "Ez")]
    solver = dccrg_amd.Poisson_Solve(max_iterations=ITERS, min_iterations=ITERS)
    dm = DepositModel(m)
    moved = 0
    for cycle in range(CYCLES):
        # deposit
        g.particles_deposit(fld, rho, K, Q, "cic", per_volume=True)
        rho_d = rho.get(0, g.n_local)
        dep = dm.deposit(1, Q)
        for c, v in zip(local, rho_d):
            tot, mag, cnt, _ = dep[c]
            V = dm.volume(c)
            assert abs(v - tot / V) <= (cnt + 2) * EPS * mag / V, (cycle, c)
        # solve, from a zero first guess, for the device's right-hand side
        rhs_d = rhs_of(rho_d)
        g.fields["rhs"].set(rhs_d)
        sol.set(np.zeros(g.n_slots))
        it, _ = solver.solve(ids, g, cache_is_up_to_date=cycle > 0)
        assert it == ITERS
        fwd, rev = solve_both_orders(ch, rhs_d[back], monkeypatch)
        phi_d = sol.get(0, g.n_local)
        scale = float(np.max(np.abs(fwd)))
        gap = float(np.max(np.abs(rev - fwd))) / scale
        err = float(np.max(np.abs(phi_d[back] - fwd))) / scale
        print(f"cycle {cycle}: solve gap of the two model orders {gap:.3e}, bound {10 * gap:.3e}, device {err:.3e}")
        assert scale > 0 and err <= 10 * gap
        # E = -grad phi
        g.gradient(sol, E, -1.0)
        G = GM.gradient(ids, BASE, 0, PERIODIC, L, phi_d[back], -1.0)
        assert not G.finer.any()
        E_d = [f.get(0, g.n_local) for f in E]
        for d in range(3):
            assert _same(E_d[d], G.grad[at, d]), (cycle, d)
        # gather
        g.particles_gather(fld, E, E0, K, "cic")
        vals = [{c: float(v) for c, v in zip(local, E_d[d])} for d in range(3)]
        gat = dm.gather(vals, 1)
        after = _local_cells(g, fld, K)
        keep = [k for k in range(K) if not E0 <= k < E0 + 3]
        left = [[] for _ in range(3)]
        slack, T = [0.0] * 3, [0.0] * 3
        for c, a in after.items():
            val, mag, cnt = gat[c]
            assert _same(np.ascontiguousarray(a[:, keep]), np.ascontiguousarray(m.cells[c][:, keep])), (cycle, c)
            assert np.all(np.abs(a[:, E0:E0 + 3] - val) <= (cnt[:, None] + 2) * EPS * mag), (cycle, c)
            q = m.cells[c][:, Q]
            for d in range(3):
                left[d].extend((q * a[:, E0 + d]).tolist())
                slack[d] += float(np.sum(np.abs(q) * ((cnt + 2) * EPS * mag[:, d])))
                T[d] += float(np.sum(np.abs(q) * mag[:, d]))
            m.set(c, a)
        # adjointness: sum_p q_p E_p = sum_c (rho_c V_c) E_c
        for d in range(3):
            right = math.fsum((rho_d[s] * dm.volume(c)) * E_d[d][s] for s, c in enumerate(local))
            bound = slack[d] + 4 * EPS * T[d] + sum(abs(E_d[d][s]) * (dep[c][2] + 3) * EPS * dep[c][1]
                                                   for s, c in enumerate(local))
            print(f"cycle {cycle}: adjointness {d}: {math.fsum(left[d])!r} {right!r} bound {bound:.3e}")
            assert T[d] > 0 and abs(math.fsum(left[d]) - right) <= bound
        # accelerate
        g.particles_accelerate(fld, E0, K, DT, Q)
        for c, a in _local_cells(g, fld, K).items():
            r = m.cells[c]
            k = np.float64(DT) * r[:, Q]
            for j in range(3):
                term = k * r[:, E0 + j]
                r[:, 3 + j] = r[:, 3 + j] + term
            assert _same(a, r), (cycle, c)
        # push
        st = g.particles_step(fld, K, None, DT)
        ms = m.step(None, DT)
        assert (st["stayed"], st["moved"], st["lost"]) == (ms["stayed"], ms["moved"], 0)
        moved += ms["moved"]
        _assert_model(g, fld, m)
        assert int(fld.sizes(0, g.n_local).sum()) == total * K * 8 and m.total() == total
    assert moved > 0
    g.close()
