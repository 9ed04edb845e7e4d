"""The model of particles following the mesh (tests/particles_adapt_model.py)
on the CPU, on the refined grid the GPU tests use: with particles seeded inside
their cells nothing is lost through refinement and unrefinement, every record
ends in the leaf the model locates for it, and a family refined and merged
again holds its records in the specified order."""
import numpy as np

from helpers import random_refines
from oracle import oracle as O
from particles_adapt_model import remesh
from particles_model import ParticleModel, seeded_particles
from test_gpu_particles import REF_L0, REF_START, REFINED


def _refined_model(K=3, seed=0):
    """The oracle side of helpers.make_pair(**REFINED) with the model on it."""
    c = REFINED
    o = O.Grid(c["length"], c["R"], c["periodic"], c["hood"], 1)
    rng = np.random.default_rng(seed)
    for _ in range(c["rounds"]):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        for cell in random_refines(ids, lv, c["R"], rng, c["frac"]):
            o.refine_completely(cell)
        o.stop_refining()
    return ParticleModel(o, REF_START, REF_L0, K)


def _seed(m, rng, max_per_cell):
    ctr, ln = m.o.geometry(m.leaves)
    for c, r in seeded_particles(m.leaves, ctr, ln, rng, max_per_cell, m.K).items():
        m.set(c, r)


def _all_in_their_cells(m):
    for c, a in m.cells.items():
        if a.shape[0]:
            assert np.all(m.locate(a[:, 0:3]) == np.uint64(c)), c


def test_refine_then_unrefine_conserves_and_locates():
    m = _refined_model()
    rng = np.random.default_rng(31)
    _seed(m, rng, 5)
    before = m.total()
    assert before > 500
    lv = m.o.mapping.batch(m.leaves)["level"]
    for c in random_refines(m.leaves, lv, m.R, rng, 0.15):
        m.o.refine_completely(c)
    m.o.stop_refining()
    st = remesh(m)
    assert st["lost"] == 0 and st["to_parents"] == 0 and st["to_children"] > 0
    assert m.total() == before and sorted(m.cells) == [int(c) for c in m.leaves]
    _all_in_their_cells(m)
    lv = m.o.mapping.batch(m.leaves)["level"]
    for c in rng.choice(m.leaves[lv > 0], 60, replace=False):
        m.o.unrefine_completely(int(c))
    m.o.stop_refining()
    assert m.o.removed()[0].size > 0
    st = remesh(m)
    assert st["lost"] == 0 and st["to_children"] == 0 and st["to_parents"] > 0
    assert m.total() == before and sorted(m.cells) == [int(c) for c in m.leaves]
    _all_in_their_cells(m)


def test_family_refined_and_merged_again_keeps_its_records_in_order():
    m = _refined_model()
    rng = np.random.default_rng(32)
    _seed(m, rng, 5)
    lv = m.o.mapping.batch(m.leaves)["level"]
    done = 0
    for c in (int(x) for x in m.leaves[lv < m.R]):
        if c not in m.cells or m.cells[c].shape[0] < 3:
            continue
        rec = m.cells[c].copy()
        ctr = m.o.geometry([c])[0][0]
        m.o.refine_completely(c)
        m.o.stop_refining()
        remesh(m)
        first = int(m.o.mapping.batch([c])["child"][0])
        assert first in m.cells
        m.o.unrefine_completely(first)
        m.o.stop_refining()
        st = remesh(m)
        if c not in m.cells:  # its neighborhood forbade the merge
            continue
        assert st["lost"] == 0
        # children in ascending id = octants with x fastest; the octant of a
        # record from the parent's center, independent of locate
        octant = ((rec[:, 0] >= ctr[0]).astype(int) + 2 * (rec[:, 1] >= ctr[1]) + 4 * (rec[:, 2] >= ctr[2]))
        exp = rec[np.argsort(octant, kind="stable")]
        assert np.array_equal(m.cells[c].view(np.uint64), exp.view(np.uint64)), c
        done += 1
        if done == 3:
            break
    assert done == 3


def test_record_outside_its_parent_is_lost():
    m = _refined_model()
    rng = np.random.default_rng(33)
    _seed(m, rng, 4)
    lv = m.o.mapping.batch(m.leaves)["level"]
    c = int(m.leaves[lv < m.R][5])
    far = int(m.leaves[-1])
    pos = m.o.geometry([far])[0][0]
    assert int(m.locate(pos[None, :])[0]) == far != c
    n = m.cells[c].shape[0]
    m.set(c, np.concatenate([m.cells[c], pos[None, :], [[np.nan, 0.0, 0.0]]]))
    before = m.total()
    m.o.refine_completely(c)
    m.o.stop_refining()
    st = remesh(m)
    assert st["lost"] == 2 and st["to_children"] >= n
    assert m.total() == before - 2
    _all_in_their_cells(m)
