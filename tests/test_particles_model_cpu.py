"""The particle model (tests/particles_model.py) on the CPU: its wrap and
point location restate Cartesian_Geometry::get_real_coordinate / get_indices
and Dccrg::get_existing_cell, and its step keeps every particle in the leaf
the model locates for it."""
import numpy as np

from oracle import oracle as O
from particles_model import ParticleModel, seeded_particles


def test_wrap_on_0_3():
    m = ParticleModel(O.Grid((3, 1, 1), 0, (True, True, True), 1, 1))
    x = m.real_coordinate([[3.05, 0.5, 0.5], [-0.02, 0.5, 0.5], [3.0, 0.5, 0.5]])[:, 0]
    assert x[0] == 0.04999999999999982
    assert x[1] == 2.98
    assert x[2] == 3.0
    # the grid's end is inside for the wrap but indexes one past the last cell
    cells = m.locate([[3.05, 0.5, 0.5], [-0.02, 0.5, 0.5], [3.0, 0.5, 0.5], [2.999, 1.0, 0.5], [1.5, 0.5, 0.5]])
    assert cells.tolist() == [1, 3, 0, 0, 2]


def test_nan_outside_a_non_periodic_dimension():
    m = ParticleModel(O.Grid((4, 3, 2), 0, (True, False, False), 1, 1), start=(-1, 0.5, 0), l0=(0.5, 0.25, 1))
    r = m.real_coordinate([[1.25, 1.5, 0.5], [0.0, 0.4, 0.5], [0.0, 1.0, 2.5], [-1.5, 1.25, 2.0]])
    assert np.isnan(r[0]).tolist() == [False, True, False]  # x wraps, y is outside
    assert r[0, 0] == -0.75
    assert np.isnan(r[1]).tolist() == [False, True, False]
    assert np.isnan(r[2]).tolist() == [False, False, True]
    assert r[3].tolist() == [0.5, 1.25, 2.0]
    assert m.locate(r).tolist() == [0, 0, 0, 0]  # NaN, NaN, NaN, z at the grid's end


def test_every_particle_lies_in_its_leaf_after_every_step():
    o = O.Grid((4, 3, 2), 2, (True, True, False), 1, 1)
    rng = np.random.default_rng(3)
    for _ in range(2):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        for c in rng.choice(ids[lv < 2], 3, replace=False):
            o.refine_completely(int(c))
        o.stop_refining()
    m = ParticleModel(o, start=(-1, 0.5, 0), l0=(0.5, 0.25, 1))
    ids, _ = o.cells()
    ctr, ln = o.geometry(ids)
    for c, r in seeded_particles(ids, ctr, ln, rng, 4).items():
        m.set(c, r)
    before = m.total()
    assert before > 0
    v = np.array([0.9, -0.7, 0.45]) * m.cell_len
    lost = 0
    for _ in range(10):
        st = m.step(v, 1.0)
        lost += st["lost"]
        assert st["lost_known"] == 0  # below the finest cell length: only the open z faces lose
        for c, a in m.cells.items():
            if a.shape[0]:
                assert np.all(m.locate(a[:, 0:3]) == np.uint64(c)), c
    assert lost > 0 and m.total() == before - lost
