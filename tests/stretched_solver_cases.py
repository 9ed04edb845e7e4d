"""The meshes, coordinates and cell classes the stretched-geometry solver
tests share (a helper, not a test): built on the oracle and NumPy alone, so
the CPU tests can check that a case discriminates before a GPU test relies on
it.  The GPU tests build the same meshes through helpers.make_pair (same
seed, same refinement history) and assert that the ids agree."""
import numpy as np

import advection_model as AM
import poisson_stretched_model as PM
import stretched_model as SM
from helpers import random_refines

LARGE_LENGTH = (16, 12, 8)


def uneven_coords(length, seed, start=(-1.0, 0.25, 2.0)):
    """Seeded monotone coordinates whose neighboring level-0 cells differ in
    extent by up to a factor of four."""
    rng = np.random.default_rng(seed)
    return [np.concatenate([[start[d]], start[d] + np.cumsum(0.25 + 0.75 * rng.random(length[d]))]) for d in range(3)]


def case(name):
    if name in SM.CASES:
        R, coords = SM.case_coords(name)
        return dict(length=SM.LENGTH, R=R, periodic=SM.PERIODIC, coords=coords, rounds=2, frac=0.1)
    assert name == "large"  # more than 2048 cells: several blocks per XCD position of the cache launch
    return dict(length=LARGE_LENGTH, R=1, periodic=SM.PERIODIC, coords=uneven_coords(LARGE_LENGTH, 77), rounds=1,
                frac=0.1)


CASES = SM.CASES + ("large",)


def oracle_mesh(c, nprocs=1, hood=1, seed=0):
    """helpers.make_pair's oracle half: the refined oracle grid of a case."""
    from oracle import oracle as O

    o = O.Grid(c["length"], c["R"], c["periodic"], hood, nprocs)
    rng = np.random.default_rng(seed)
    for _ in range(c["rounds"]):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        for cell in random_refines(ids, lv, c["R"], rng, c["frac"]):
            o.refine_completely(cell)
        o.stop_refining()
    return o


def classes(ids, c, seed=5):
    """Per id 0 solve / 1 boundary / 2 skip: about an eighth of the cells
    each skipped and boundary cells, and one solve cell (its position is
    returned too) whose every face neighbor is skipped."""
    rng = np.random.default_rng(seed)
    cls = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 2]), size=ids.size)
    F = AM.faces(ids, c["length"], c["R"], c["periodic"])
    lone = int(rng.integers(ids.size))
    around = F[F[:, 0] == lone, 2]
    assert around.size and lone not in around
    cls[lone] = PM.SOLVE
    cls[around] = PM.SKIP
    return cls, lone


def model_cache(ids, c, cls, coords=None):
    """(levels, centers, lengths, Cache) of the model on the case's mesh."""
    coords = c["coords"] if coords is None else coords
    lvl, ctr, L = PM.geometry(coords, c["length"], c["R"], ids)
    return lvl, ctr, L, PM.cache(ids, c["length"], c["R"], c["periodic"], lvl, L, cls)


def rhs_of(ctr):
    return np.sin(ctr[:, 0]) * np.cos(2 * ctr[:, 1]) * np.sin(ctr[:, 2] / 4) + 0.25
