"""Poisson_Solve under an active stretched geometry
(dccrgx_set_stretched_geometry) against tests/poisson_stretched_model.py,
which test_poisson_stretched_model_cpu.py pins to the oracle.

* Factors and cell types: bitwise.  The cache kernel takes every length as
  (c[i0 + 1] - c[i0]) / 2^level with contraction off, the model from
  stretched_model.cell_geometry, and both restate set_scaling_factor in the
  reference's operand order.
* Iterates after k BiCG iterations: test_gpu_poisson.py's tolerances (1e-13 /
  1e-11 / 1e-8 of max|model| at k = 1 / 5 / 20, 1e-12 for the solution), the
  reference's own summation-order noise.
* The facade example's printed norms: within 1e-12 max|x| sqrt(n) of the
  model's (n cells each within 1e-12 max|x|).
"""
import numpy as np
import pytest

import poisson_stretched_model as PM
import stretched_solver_cases as SC
from helpers import make_pair

pytestmark = pytest.mark.gpu

TOL_K = {1: 1e-13, 5: 1e-11, 20: 1e-8}


def _grid(name):
    """The case's refined grid with its stretched geometry, the sorted ids."""
    c = SC.case(name)
    g, o = make_pair(c["length"], c["R"], c["periodic"], 1, c["rounds"], c["frac"])
    g.set_stretched_geometry(c["coords"])
    ids = g.local_cells()
    assert np.array_equal(ids, np.sort(SC.oracle_mesh(c).cells()[0]))
    return c, g, o, ids


def _fields(g, ids, rhs_v, sol_v):
    slots = g.slot_ids()[: g.n_local]
    order = np.searchsorted(ids, slots)
    rhs = g.add_field("rhs", np.float64, False)
    sol = g.add_field("solution", np.float64, False)
    rhs.set(rhs_v[order])
    sol.set(sol_v[order])
    return order


def _state(g, order, names):
    import dccrg_amd

    out = {}
    for nm in names:
        f = g.fields["solution"] if nm == "solution" else dccrg_amd.Poisson_Solve.field(g, nm)
        out[nm] = f.get(0, order.size)
    return out


def _assert_factors(g, order, table, types):
    got = _state(g, order, PM.FACTORS + ("type",))
    for k, nm in enumerate(PM.FACTORS):
        assert np.array_equal(got[nm], table[order, k]), nm
    assert np.array_equal(got["type"], types[order].astype(np.int32))


_MODEL = {}


def _model(name, ids):
    """The model's cache, right-hand side and first guess of a case, once."""
    if name not in _MODEL:
        c = SC.case(name)
        cls, lone = SC.classes(ids, c)
        lvl, ctr, L, ch = SC.model_cache(ids, c, cls)
        rhs = SC.rhs_of(ctr)
        sol0 = np.where(cls == PM.BOUNDARY, 0.5 * rhs, 0.0)
        _MODEL[name] = dict(cls=cls, lone=lone, ch=ch, rhs=rhs, sol0=sol0)
    return _MODEL[name]


# ---- 1. factors and types ------------------------------------------------------------
@pytest.mark.parametrize("name", SC.CASES)
def test_factors_and_types_bitwise(gpu, name):
    import dccrg_amd

    c, g, o, ids = _grid(name)
    M = _model(name, ids)
    cls, ch = M["cls"], M["ch"]
    order = _fields(g, ids, M["rhs"], M["sol0"])
    dccrg_amd.Poisson_Solve().cache_system_info(ids[cls == PM.SOLVE], g, ids[cls == PM.SKIP])
    _assert_factors(g, order, PM.factor_table(ch), ch.type)
    # skipped, boundary and solved cells, and the cell whose every face neighbor is skipped
    assert {0, 1, 2} <= set(ch.type.tolist()) and cls[M["lone"]] == PM.SOLVE and ch.type[M["lone"]] == PM.SKIP
    if name == "large":
        assert g.n_local > 2048  # more than one block per XCD position
    g.close()


# ---- 2. iterates -----------------------------------------------------------------------
@pytest.mark.parametrize("iters", sorted(TOL_K))
def test_fixed_iterations_match_model(gpu, iters):
    import dccrg_amd

    name = "rounded"
    c, g, o, ids = _grid(name)
    M = _model(name, ids)
    cls, ch = M["cls"], M["ch"]
    order = _fields(g, ids, M["rhs"], M["sol0"])
    s = dccrg_amd.Poisson_Solve(max_iterations=iters, min_iterations=iters)
    it, res = s.solve(ids[cls == PM.SOLVE], g, ids[cls == PM.SKIP])
    st, mit, mres = PM.solve(ch, M["rhs"], M["sol0"], iters, iters)
    assert it == mit == iters
    print(f"{iters} iterations: residual {res!r}, model {mres!r}")
    assert abs(res - mres) <= 1e-10 * abs(mres)
    got = _state(g, order, PM.STATE)
    sel = (ch.type == PM.SOLVE)[order]
    for nm in PM.STATE:
        e = st[nm][order]
        tol = 1e-12 if nm in ("solution", "best_solution") else TOL_K[iters]
        scale = max(float(np.max(np.abs(e[sel]))), 1e-300)
        err = float(np.max(np.abs(got[nm][sel] - e[sel]))) / scale
        print(f"{iters} iterations, {nm}: {err:.3e} (tolerance {tol:g})")
        assert err <= tol, (nm, err)
    assert np.array_equal(got["solution"][~sel], M["sol0"][order][~sel])
    g.close()


# ---- 3. geometry changes take effect at the next cache pass ------------------------------
def test_geometry_changes_at_the_next_cache_pass(gpu):
    import dccrg_amd
    from oracle import oracle as O

    name = "exact"
    c, g, o, ids = _grid(name)
    M = _model(name, ids)
    cls, ch = M["cls"], M["ch"]
    order = _fields(g, ids, M["rhs"], M["sol0"])
    s = dccrg_amd.Poisson_Solve(max_iterations=1)
    solve, skip = ids[cls == PM.SOLVE], ids[cls == PM.SKIP]
    s.cache_system_info(solve, g, skip)
    _assert_factors(g, order, PM.factor_table(ch), ch.type)
    # back to Cartesian: the oracle's factors
    start, l0 = (-1.0, 0.5, 0.0), (0.5, 0.25, 1.0)
    g.set_geometry(start, l0)
    _assert_factors(g, order, PM.factor_table(ch), ch.type)  # not before the next cache pass
    s.cache_system_info(solve, g, skip)
    o.set_geometry(start, l0)
    o.po_set(ids, M["rhs"], M["sol0"], cls.astype(np.int32))
    o.po_solve(max_iterations=1)
    exp = o.po_get(ids)
    cart = np.stack([exp[:, O.Grid.PO_FIELDS.index(nm)] for nm in PM.FACTORS], axis=1)
    assert not np.array_equal(cart, PM.factor_table(ch))
    _assert_factors(g, order, cart, exp[:, 14])
    # stretched again, the cache declared up to date: the old factors stay
    g.set_stretched_geometry(c["coords"])
    s.solve(solve, g, skip, cache_is_up_to_date=True)
    _assert_factors(g, order, cart, exp[:, 14])
    # the next cache pass: the stretched factors
    s.solve(solve, g, skip)
    _assert_factors(g, order, PM.factor_table(ch), ch.type)
    g.close()


# ---- 4. two processes (host transport), run by the test below -------------------------------
def sc_stretched_poisson(rank, world):
    """The refined 'rounded' case across real processes (the oracle deals the
    level-0 cells out by id, so the process boundary lies between the two z
    layers, 0.3 and 0.7 thick): the factors gathered by id equal the
    one-address-space model bitwise, the solution after 5 iterations is within
    1e-12 max|x|, and some face between cells of different processes joins
    level-0 cells of different extent."""
    import dccrg_amd
    import advection_model as AM
    from test_gpu_transport import _gather, _grid as transport_grid

    c = SC.case("rounded")
    o = SC.oracle_mesh(c, nprocs=world)
    all_ids, own = o.cells()
    g = transport_grid(c["length"], c["R"], c["periodic"], 1)
    g.set_cells(all_ids, own)
    g.set_stretched_geometry(c["coords"])
    k = np.argsort(all_ids)
    ids, own = all_ids[k], own[k]
    cls, lone = SC.classes(ids, c)
    lvl, ctr, L, ch = SC.model_cache(ids, c, cls)
    rhs_v = SC.rhs_of(ctr)
    sol0 = np.where(cls == PM.BOUNDARY, 0.5 * rhs_v, 0.0)
    slots = g.slot_ids()[: g.n_local]
    at = np.searchsorted(ids, slots)
    rhs = g.add_field("rhs", np.float64, False)
    sol = g.add_field("solution", np.float64, False)
    rhs.set(rhs_v[at])
    sol.set(sol0[at])
    s = dccrg_amd.Poisson_Solve(max_iterations=5, min_iterations=5)
    it, res = s.solve(ids[cls == PM.SOLVE], g, ids[cls == PM.SKIP])
    st, mit, mres = PM.solve(ch, rhs_v, sol0, 5, 5)
    mine = {nm: dccrg_amd.Poisson_Solve.field(g, nm).get(0, slots.size) for nm in PM.FACTORS + ("type",)}
    mine["solution"] = sol.get(0, slots.size)
    parts = _gather((slots, mine))
    got = {nm: np.full(ids.size, np.nan) for nm in mine}
    seen = np.zeros(ids.size, np.int64)
    for p_slots, p in parts:
        j = np.searchsorted(ids, p_slots)
        seen[j] += 1
        for nm in p:
            got[nm][j] = p[nm]
    table = PM.factor_table(ch)
    res_d = dict(every_cell_once=bool(np.all(seen == 1)), iterations=it == mit == 5,
                 residual=abs(res - mres) <= 1e-10 * abs(mres),
                 types=bool(np.array_equal(got["type"], ch.type.astype(np.float64))),
                 remote=g.n_slots > g.n_local)
    for kk, nm in enumerate(PM.FACTORS):
        res_d[nm] = bool(np.array_equal(got[nm], table[:, kk]))
    sel = ch.type == PM.SOLVE
    scale = float(np.max(np.abs(st["solution"][sel])))
    res_d["solution"] = float(np.max(np.abs(got["solution"] - st["solution"]))) <= 1e-12 * scale
    # the process boundary runs between level-0 cells of different extent
    F = AM.faces(ids, c["length"], c["R"], c["periodic"])
    d = F[:, 1] >> 1
    ext = L * (2.0 ** lvl)[:, None]  # the level-0 cell's extent (exact: a power of two times the length)
    res_d["uneven_process_boundary"] = bool(np.any((own[F[:, 0]] != own[F[:, 2]])
                                                   & (ext[F[:, 0], d] != ext[F[:, 2], d])))
    g.close()
    return res_d


def test_two_processes(gpu, tmp_path):
    from test_gpu_transport import _run_group

    results = _run_group(2, tmp_path, names=["sc_stretched_poisson"], module="test_gpu_poisson_stretched")
    assert len(results.get("sc_stretched_poisson", {})) == 2
    for rank, (kind, out) in sorted(results["sc_stretched_poisson"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"


# ---- 5. the facade example -----------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario():
    return {n: PM.poisson1d_stretched(n) for n in PM.STRETCHED1D_SIZES}


@pytest.mark.parametrize("P", [1, 2])
def test_facade_example(gpu, scenario, P):
    """examples/poisson_stretched.cpp: exit status 0 (the reference program's
    two conditions hold) and every printed norm within 1e-12 max|x| sqrt(n)
    of the model's."""
    from test_gpu_facade import mpirun

    out = mpirun("poisson_stretched", P)
    lines = [ln.split() for ln in out.splitlines() if ln.startswith("cells ")]
    assert [int(w[1]) for w in lines] == list(PM.STRETCHED1D_SIZES), out
    for w in lines:
        n = int(w[1])
        assert w[2] == "stretched" and w[6] == "even"
        for name, at in (("stretched", 3), ("reference", 7)):
            norm, it, res, x = scenario[n][name]
            bound = 1e-12 * float(np.max(np.abs(x))) * np.sqrt(n)
            print(f"{P} ranks, {n} cells, {name}: {float(w[at])!r} model {norm!r} bound {bound:.3e}")
            assert abs(float(w[at]) - norm) <= bound, (n, name, w[at], norm)
            assert int(w[at + 1]) == it
