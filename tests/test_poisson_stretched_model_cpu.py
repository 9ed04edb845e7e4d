"""tests/poisson_stretched_model.py pinned before the GPU tests rely on it.

* On evenly spaced coordinates start + i * h with h a power of two the
  stretched length (c[i + 1] - c[i]) / 2^level is bitwise l0 * 2^-level, so the
  model must reproduce the oracle (the Cartesian restatement of
  poisson_solve.hpp): factors and types bitwise, iterates within the
  tolerances tests/test_gpu_poisson.py derives from the reference's own
  summation-order noise (1e-13 / 1e-11 / 1e-8 of max|oracle| after 1 / 5 / 20
  iterations, 1e-12 for the solution).
* The scenario of tests/poisson/poisson1d_stretched.cpp on the model meets
  the program's own two conditions.
* Every uneven case of the GPU tests changes the factors against what the
  Cartesian fallback (each dimension's start and first cell length) gives,
  in every dimension whose coordinates are uneven, and every dimension is
  uneven in some case.  ("exact" has the evenly spaced z coordinates 0, 1, 2
  starting at 0: there the fallback is right and nothing can differ.)
"""
import math

import numpy as np
import pytest

import poisson_stretched_model as PM
import stretched_solver_cases as SC
from oracle import oracle as O
from poisson_cases import center_refine_select, poisson3d_solution

START, L0 = (-2.0, 0.5, 8.0), (1.0, 0.5, 4.0)  # powers of two and their sums: start + i * l0 is exact
N, R = 8, 2
TOL_K = {1: 1e-13, 5: 1e-11, 20: 1e-8}


@pytest.fixture(scope="module")
def even():
    """test_gpu_poisson.build_pair's recipe on the oracle alone (the center
    refined twice plus seeded random refines), a tenth of the cells each
    skipped and boundary cells."""
    periodic = (True, True, True)
    o = O.Grid((N, N, N), R, periodic, 0, 1)
    o.set_geometry(START, L0)
    rng = np.random.default_rng(3)
    shift = np.array(START)
    for r in range(2):
        ids = np.sort(o.cells()[0])
        c, L = o.geometry(ids)
        sel = list(ids[center_refine_select(c - shift, L)])
        lv = o.mapping.batch(ids)["level"]
        cand = ids[lv < R]
        sel += list(rng.choice(cand, size=max(1, cand.size // 20), replace=False))
        for i in sel:
            o.refine_completely(int(i))
        o.stop_refining()
    ids = np.sort(o.cells()[0])
    c, L = o.geometry(ids)
    cls = rng.choice(np.array([0] * 8 + [1, 2]), size=ids.size).astype(np.int32)
    rhs = -(81.0 / 16.0) * poisson3d_solution(c - shift)
    sol0 = np.where(cls == PM.BOUNDARY, 0.1 * poisson3d_solution(c - shift), 0.0)
    coords = PM.even_coords(START, L0, (N, N, N))
    lvl, mc, mL = PM.geometry(coords, (N, N, N), R, ids)
    assert np.array_equal(mL, L) and np.array_equal(lvl, o.mapping.batch(ids)["level"])
    ch = PM.cache(ids, (N, N, N), R, periodic, lvl, mL, cls)
    return dict(o=o, ids=ids, cls=cls, rhs=rhs, sol0=sol0, ch=ch, levels=lvl)


def test_factors_and_types_equal_the_oracle_bitwise(even):
    o, ids, ch = even["o"], even["ids"], even["ch"]
    assert len(set(even["levels"].tolist())) == 3 and {0, 1, 2} == set(even["cls"].tolist())
    o.po_set(ids, even["rhs"], even["sol0"], even["cls"])
    o.po_solve(max_iterations=1)
    exp = o.po_get(ids)
    got = PM.factor_table(ch)
    for k, nm in enumerate(PM.FACTORS):
        assert np.array_equal(got[:, k], exp[:, O.Grid.PO_FIELDS.index(nm)]), nm
    assert np.array_equal(ch.type, exp[:, 14].astype(np.int32))
    assert np.count_nonzero(ch.kept[:, 3]) > 0  # finer neighbors take part


@pytest.mark.parametrize("iters", sorted(TOL_K))
def test_iterates_match_the_oracle(even, iters):
    o, ids, ch = even["o"], even["ids"], even["ch"]
    o.po_set(ids, even["rhs"], even["sol0"], even["cls"])
    oit, ores = o.po_solve(max_iterations=iters, min_iterations=iters)
    exp = o.po_get(ids)
    st, it, res = PM.solve(ch, even["rhs"], even["sol0"], iters, iters)
    assert it == oit == iters
    assert abs(res - ores) <= 1e-10 * abs(ores)
    sel = ch.type == PM.SOLVE
    for nm in PM.STATE:
        e = exp[:, O.Grid.PO_FIELDS.index(nm)]
        tol = 1e-12 if nm in ("solution", "best_solution") else TOL_K[iters]
        scale = max(float(np.max(np.abs(e[sel]))), 1e-300)
        err = float(np.max(np.abs(st[nm][sel] - e[sel]))) / scale
        print(f"{iters} iterations, {nm}: {err:.3e} (tolerance {tol:g})")
        assert err <= tol, (nm, err)
    # cells that are not solved keep their solution
    assert np.array_equal(st["solution"][~sel], even["sol0"][~sel])


def test_one_dimensional_periodic_grid_matches_the_oracle():
    """n x 1 x 1 periodic, the scenario's shape: a cell is its own face
    neighbor in y and z, as in the oracle."""
    n, h = 16, 0.5
    o = O.Grid((n, 1, 1), 0, (True, True, True), 0, 1)
    o.set_geometry((0, 0, 0), (h, 1, 1))
    ids = np.arange(1, n + 1, dtype=np.uint64)
    coords = PM.even_coords((0, 0, 0), (h, 1, 1), (n, 1, 1))
    lvl, ctr, L = PM.geometry(coords, (n, 1, 1), 0, ids)
    rhs = np.sin(2 * math.pi * ctr[:, 0] / (n * h))
    cls = np.zeros(n, np.int32)
    ch = PM.cache(ids, (n, 1, 1), 0, (True, True, True), lvl, L, cls)
    o.po_set(ids, rhs, np.zeros(n), cls)
    oit, ores = o.po_solve(5, 5)
    exp = o.po_get(ids)
    got = PM.factor_table(ch)
    for k, nm in enumerate(PM.FACTORS):
        assert np.array_equal(got[:, k], exp[:, O.Grid.PO_FIELDS.index(nm)]), nm
    st, it, res = PM.solve(ch, rhs, np.zeros(n), 5, 5)
    e = exp[:, 0]
    assert it == oit and float(np.max(np.abs(st["solution"] - e))) <= 1e-12 * float(np.max(np.abs(e)))


def test_poisson1d_stretched_scenario_on_the_model():
    """poisson1d_stretched.cpp:311-332: at 8 cells the stretched norm is not
    above the evenly spaced one, and the evenly spaced norm never grows."""
    old = float("inf")
    for n in PM.STRETCHED1D_SIZES:
        r = PM.poisson1d_stretched(n)
        ns, nr = r["stretched"][0], r["reference"][0]
        print(f"{n} cells: stretched {ns:.6g} ({r['stretched'][1]} it), evenly spaced {nr:.6g} ({r['reference'][1]} it)")
        if n == 8:
            assert ns <= nr, (ns, nr)
        assert nr <= old, (n, nr, old)
        old = nr
    x = PM.stretched1d_coords(16)[0]
    w = np.diff(x)
    assert x[0] == 0 and x[-1] == 2 * math.pi and np.all(w > 0)
    assert np.allclose(np.maximum(w[::2] / w[1::2], w[1::2] / w[::2]), 3.0, rtol=1e-12)


@pytest.mark.parametrize("name", SC.CASES)
def test_uneven_cases_discriminate(name):
    c = SC.case(name)
    ids = np.sort(SC.oracle_mesh(c).cells()[0])
    cls, lone = SC.classes(ids, c)
    lvl, ctr, L, ch = SC.model_cache(ids, c, cls)
    assert ch.type[lone] == PM.SKIP and cls[lone] == PM.SOLVE
    assert {0, 1, 2} <= set(ch.type.tolist()) and len(set(lvl.tolist())) > 1
    fb = PM.cache(ids, c["length"], c["R"], c["periodic"], lvl, PM.fallback_lengths(c["coords"], lvl), cls)
    assert np.array_equal(fb.type, ch.type)
    for d in range(3):
        w = np.diff(c["coords"][d])
        differs = int(np.count_nonzero((ch.f[:, 2 * d] != fb.f[:, 2 * d]) | (ch.f[:, 2 * d + 1] != fb.f[:, 2 * d + 1])))
        if np.all(w == w[0]):
            assert name == "exact" and d == 2 and differs == 0
        else:
            assert differs > 0, (name, d)
    if name == "large":
        assert ids.size > 2048


def test_every_dimension_is_uneven_in_some_case():
    for d in range(3):
        assert any(len(set(np.diff(SC.case(n)["coords"][d]).tolist())) > 1 for n in SC.CASES), d
