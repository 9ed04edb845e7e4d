"""The advection set-up under an active stretched geometry:
advection_initialize and advection_adapt's reset pass take centers and lengths
from the stretched coordinates, and the field-reading sweeps run on them.

Expected values: lengths and centers from g.geometry() (pinned bitwise to the
reference by test_gpu_stretched.py) and from stretched_model; velocities the
formulas of tests/advection/initialize.hpp:42-78 on those centers (sums and
differences only: bitwise); the density within 1e-15 absolute (values in
[0, 0.5]; the host libm's cos and NumPy's may differ in the last bits); the
sweeps against advection_model.step on the downloaded fields within
1e-12 max|rho|, the existing sweep tolerance; the time step exactly
advection_model.max_time_step over the downloaded fields."""
import numpy as np
import pytest

import advection_model as AM
import poisson_stretched_model as PM
import stretched_model as SM

pytestmark = pytest.mark.gpu

NAMES = ("density", "vx", "vy", "vz", "lx", "ly", "lz")
BASE, R, PERIODIC = (12, 12, 3), 2, (True, True, False)


def coords():
    """Seeded uneven monotone coordinates: [0, 1] in x and y (the hump of
    initialize.hpp sits at (0.25, 0.5)), neighboring extents up to 1 : 4."""
    rng = np.random.default_rng(12)
    out = []
    for d in range(3):
        w = 0.25 + 0.75 * rng.random(BASE[d])
        c = np.concatenate([[0.0], np.cumsum(w) / np.sum(w)])
        c[-1] = 1.0
        out.append(c if d < 2 else 0.5 * c - 0.1)
    return out


def formulas(ctr):
    """initialize.hpp:42-78 -> (density, vx, vy, vz)."""
    radius = 0.15
    hr = np.minimum(np.sqrt((ctr[:, 0] - 0.25) ** 2 + (ctr[:, 1] - 0.5) ** 2), radius) / radius
    return 0.25 * (1 + np.cos(np.pi * hr)), -ctr[:, 1] + 0.5, +ctr[:, 0] - 0.5, np.zeros(ctr.shape[0])


def check_fields(g, f, cs, n, density):
    """The first n slots' velocity and length fields (and the density) against
    the formulas on the stretched geometry."""
    ids = g.slot_ids()[:n]
    ctr, L = g.geometry(ids)
    _, mc, mL = PM.geometry(cs, BASE, R, ids)
    assert SM.same_bits(ctr, mc) and SM.same_bits(L, mL)
    rho, vx, vy, vz = formulas(ctr)
    for d in range(3):
        assert SM.same_bits(f[4 + d].get(0, n), L[:, d]), NAMES[4 + d]
    for k, v in ((1, vx), (2, vy), (3, vz)):
        assert SM.same_bits(f[k].get(0, n), v), NAMES[k]
    if density:
        err = float(np.max(np.abs(f[0].get(0, n) - rho)))
        print(f"density: max abs error {err:.3e}")
        assert err <= 1e-15
    return ids, L


def family_next_to_a_different_extent(ids, cs):
    """A refined cell (inside its own level-0 cell, as every cell is) with a
    face neighbor that lies in a level-0 cell of a different extent along the
    face's dimension."""
    lvl, lo, _ = AM.boxes(ids, BASE, R)
    F = AM.faces(ids, BASE, R, PERIODIC)
    c, d, n = F[:, 0], F[:, 1] >> 1, F[:, 2]
    i0c, i0n = lo[c, d] >> R, lo[n, d] >> R
    w = [np.diff(x) for x in cs]
    wc = np.array([w[dd][i] for dd, i in zip(d, i0c)])
    wn = np.array([w[dd][i] for dd, i in zip(d, i0n)])
    return bool(np.any((lvl[c] >= 1) & (i0c != i0n) & (wc != wn))), F


def test_initialize_adapt_and_sweeps_follow_the_stretched_geometry(gpu):
    import dccrg_amd

    cs = coords()
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length(BASE).set_neighborhood_length(0)
    g.set_maximum_refinement_level(R).set_periodic(*PERIODIC).initialize()
    g.set_stretched_geometry(cs)
    f = [g.add_field(n, np.float64, n == "density") for n in NAMES]
    for _ in range(R):
        g.advection_initialize(f)
        for cell in g.advection_refine_candidates(f[0], 0.025 / R, 0.25):
            g.refine_completely(int(cell))
        g.stop_refining()
    g.advection_initialize(f)
    ids, L = check_fields(g, f, cs, g.n_slots, density=True)
    assert len({float(v) for v in L[:, 0]}) > 2 * R  # several extents at several levels
    straddle, _ = family_next_to_a_different_extent(ids[: g.n_local], cs)
    assert straddle
    assert g.advection_length_source(f) == 0

    di = 0.025 / R
    created = removed = 0
    for step in range(6):
        nl = g.n_local
        ids = g.slot_ids()[:nl]
        cols = np.stack([f[k].get(0, nl) for k in range(7)], axis=1)
        want_dt = AM.max_time_step(cols)
        got_dt = g.advection_max_time_step(f)
        assert got_dt == want_dt, (step, got_dt, want_dt)
        dt = 0.5 * got_dt
        exp = AM.step(AM.faces(ids, BASE, R, PERIODIC), cols, dt)
        # the order of test_gpu_advection_adapt.product_step
        g.start_remote_neighbor_copy_updates()
        g.advection_step(f, dt, "inner")
        g.wait_remote_neighbor_copy_update_receives()
        g.advection_step(f, dt, "outer")
        g.wait_remote_neighbor_copy_update_sends()
        g.advection_check_adaptation(f[0], di)
        g.advection_commit(f[0])
        got = f[0].get(0, nl)
        err = float(np.max(np.abs(got - exp.astype(np.float64)))) / float(np.max(np.abs(cols[:, 0])))
        print(f"step {step}: {nl} cells, density rel err {err:.3e}")
        assert err <= 1e-12, (step, err)
        c, r = g.advection_adapt(f)
        created += c
        removed += r
        check_fields(g, f, cs, g.n_local, density=False)
        assert g.advection_length_source(f) == 0
    assert created > 0
    # the reset pass's time-step bound after the last adapt
    cols = np.stack([f[k].get(0, g.n_local) for k in range(7)], axis=1)
    assert g.advection_max_time_step(f) == AM.max_time_step(cols)
    g.close()
