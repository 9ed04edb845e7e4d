"""Particles follow the mesh through stop_refining
(Dccrg.particles_follow_mesh, dccrg_amd/csrc/particles.hip) against the model
of tests/particles_adapt_model.py.

Everything is compared per cell id, bitwise, order included: a refined
parent's records go to the child point location names for them, each child's
in the parent's order; a merged family's parent holds its children's records
in ascending child id.  The statistics are compared with the model's."""
import numpy as np
import pytest

import stretched_model as SM
from helpers import random_refines
from particles_adapt_model import remesh
from particles_model import ParticleModel, seeded_particles
from test_gpu_particles import REF_L0, REF_START, REFINED, _assert_model, _local_cells, _pair, _same, _seed, _upload

pytestmark = pytest.mark.gpu


def _adapt(g, m, refine=(), unrefine=()):
    """The same requests to the product and to the oracle, stop_refining on
    both, the model redistributed.  Returns the model's counts."""
    for c in refine:
        assert g.refine_completely(int(c))
        m.o.refine_completely(int(c))
    for c in unrefine:
        assert g.unrefine_completely(int(c)) == m.o.unrefine_completely(int(c))
    g.stop_refining()
    m.o.stop_refining()
    return remesh(m)


def _check(g, fld, m, st):
    got = g.particles_adapt_stats(fld)
    print("adapt", got, st)
    assert got == st
    _assert_model(g, fld, m)


def _random_requests(g, m, rng, frac, n_unrefine):
    ids = np.sort(g.local_cells())
    lv = m.o.mapping.batch(ids)["level"]
    ref = random_refines(ids, lv, m.R, rng, frac)
    cand = np.setdiff1d(ids[lv > 0], np.array(ref, np.uint64))
    unref = rng.choice(cand, min(n_unrefine, cand.size), replace=False) if cand.size else []
    return ref, [int(c) for c in unref]


def test_small_grid_full_empty_one_octant_and_center_planes(gpu):
    """2 x 2 x 2, R = 2: four level-0 cells refined at once - one of 300
    records (more than a wave and than a block), one of none, one with all
    records in a single octant, one with records exactly on its three center
    planes and on its min corner - then one of the children (the level-0 cells
    beside it are refined with it)."""
    g, m, fld = _pair((2, 2, 2), R=2, periodic=(False, False, False))
    g.particles_follow_mesh(fld, 3)
    rng = np.random.default_rng(41)
    ctr, ln = m.o.geometry(m.leaves)
    lo = {int(c): x - l / 2 for c, x, l in zip(m.leaves, ctr, ln)}
    for c in m.leaves:
        m.set(c, lo[int(c)] + rng.random((3, 3)))
    m.set(1, lo[1] + rng.random((300, 3)))
    m.set(8, np.zeros((0, 3)))
    m.set(4, lo[4] + np.array([0.5, 0.0, 0.5]) + 0.5 * rng.random((70, 3)))  # octant x high, y low, z high
    p = lo[6] + rng.random((40, 3))
    p[0:10, 0] = lo[6][0] + 0.5
    p[10:20, 1] = lo[6][1] + 0.5
    p[20:30, 2] = lo[6][2] + 0.5
    p[30] = lo[6] + 0.5
    p[31] = lo[6]
    p[32:36, 0:2] = lo[6][0:2] + 0.5
    m.set(6, p)
    _upload(g, fld, m)
    before = m.total()
    st = _adapt(g, m, refine=(1, 4, 6, 8))
    assert st == dict(to_children=300 + 70 + 40, to_parents=0, lost=0)
    _check(g, fld, m, st)
    kids = m.o.mapping.batch(m.o.mapping.batch([4])["child"])["siblings"][0]
    assert [m.cells[int(k)].shape[0] for k in kids] == [0, 0, 0, 0, 0, 70, 0, 0]
    full = max((int(k) for k in m.o.mapping.batch(m.o.mapping.batch([1])["child"])["siblings"][0]),
               key=lambda k: m.cells[k].shape[0])
    n_full = m.cells[full].shape[0]
    assert n_full > 20
    st = _adapt(g, m, refine=(full,))
    assert st["lost"] == 0 and st["to_children"] > n_full  # the level-0 cells beside it hold records too
    _check(g, fld, m, st)
    assert m.total() == before
    g.close()


def test_refined_grid_three_rounds_with_steps(gpu):
    g, m, fld = _pair(start=REF_START, l0=REF_L0, **REFINED)
    g.particles_follow_mesh(fld)
    rng = np.random.default_rng(42)
    _seed(g, m, fld, rng, 5)
    v = tuple(0.9 * np.array([0.9, -0.7, 0.45]) * m.cell_len)
    moved = dict(to_children=0, to_parents=0)
    for rnd in range(3):
        before = m.total()
        ref, unref = _random_requests(g, m, rng, 0.08, 80)
        st = _adapt(g, m, ref, unref)
        assert st["lost"] == 0 and m.total() == before
        _check(g, fld, m, st)
        for k in moved:
            moved[k] += st[k]
        sg = g.particles_step(fld, 3, v, 0.5)
        sm = m.step(v, 0.5)
        assert (sg["stayed"], sg["moved"], sg["lost"]) == (sm["stayed"], sm["moved"], sm["lost"])
        _assert_model(g, fld, m)
    assert moved["to_children"] > 100 and moved["to_parents"] > 100
    g.close()


def test_whole_records_of_six_doubles(gpu):
    """K = 6 with per-particle velocities: doubles 3..5 travel with their position."""
    g, m, fld = _pair(start=REF_START, l0=REF_L0, K=6, **REFINED)
    g.particles_follow_mesh(fld, 6)
    rng = np.random.default_rng(43)
    _seed(g, m, fld, rng, 5, vmax=0.9 * m.cell_len)
    ref, _ = _random_requests(g, m, rng, 0.15, 0)
    st = _adapt(g, m, ref)
    assert st["lost"] == 0 and st["to_children"] > 100
    _check(g, fld, m, st)
    sg = g.particles_step(fld, 6, None, 0.5)
    sm = m.step(None, 0.5)
    assert (sg["stayed"], sg["moved"], sg["lost"]) == (sm["stayed"], sm["moved"], sm["lost"])
    _assert_model(g, fld, m)
    _, unref = _random_requests(g, m, rng, 0.0, 200)
    st = _adapt(g, m, (), unref)
    assert st["lost"] == 0 and st["to_parents"] > 100
    _check(g, fld, m, st)
    g.close()


def test_stretched_geometry_with_boundary_records(gpu):
    """The 'rounded' case (R = 3): records inside their cells and on every
    level-0 and finest boundary of the cells to be refined that the model
    locates in them - the rounding-quirk boundaries among them."""
    from test_gpu_stretched import _pair as stretched_pair

    g, m, fld, coords, R = stretched_pair("rounded")
    g.particles_follow_mesh(fld, 3)
    rng = np.random.default_rng(44)
    ctr, ln = m.geometry(m.leaves)
    for c, r in seeded_particles(m.leaves, ctr, ln, rng, 4).items():
        m.set(c, r)
    lv = m.o.mapping.batch(m.leaves)["level"]
    ref = random_refines(m.leaves, lv, R, rng, 0.15)
    pc, pl = m.geometry(np.array(ref, np.uint64))
    special = [SM.special_values(coords[d], R) for d in range(3)]
    on_boundary = 0
    for c, x, l in zip(ref, pc, pl):
        lo, hi = x - l / 2, x + l / 2
        pts = []
        for d in range(3):
            sv = special[d]
            sv = sv[(sv >= np.nextafter(lo[d], -np.inf)) & (sv <= np.nextafter(hi[d], np.inf))]
            p = lo + l * rng.random((sv.size, 3))
            p[:, d] = sv
            pts.append(p)
        pts = np.concatenate(pts)
        pts = pts[m.locate(pts) == np.uint64(c)]
        on_boundary += pts.shape[0]
        m.set(c, np.concatenate([m.cells[c], pts]))
    assert on_boundary > 200
    _upload(g, fld, m)
    before = m.total()
    st = _adapt(g, m, ref)
    assert st["lost"] == 0 and st["to_children"] >= on_boundary and m.total() == before
    _check(g, fld, m, st)
    _, unref = _random_requests(g, m, rng, 0.0, 300)
    st = _adapt(g, m, (), unref)
    assert st["lost"] == 0 and st["to_parents"] > 0
    _check(g, fld, m, st)
    g.close()


def test_off_by_default_then_on_then_off(gpu):
    g, m, fld = _pair((4, 4, 2), R=1)
    rng = np.random.default_rng(45)
    _seed(g, m, fld, rng, 6)
    rec = {c: a.copy() for c, a in m.cells.items()}
    assert g.particles_adapt_stats(fld) == dict(to_children=0, to_parents=0, lost=0)

    def cycle(follow):
        """Refine cell 6, merge it again; the children's and the parent's
        records after each stop_refining, and the removed store."""
        fld.set([rec[int(c)].reshape(-1) for c in g.slot_ids()[: g.n_local]])
        assert g.refine_completely(6)
        new = g.stop_refining()
        assert new.size == 8
        kids = _local_cells(g, fld, 3)
        s1 = g.particles_adapt_stats(fld)
        assert g.unrefine_completely(int(new[0]))
        g.stop_refining()
        removed = g.get_removed_cells()
        assert sorted(removed.tolist()) == sorted(new.tolist())
        store = dict(zip(removed.tolist(), fld.get_removed()))
        return kids, new, _local_cells(g, fld, 3), store, s1, g.particles_adapt_stats(fld)

    n6 = rec[6].shape[0]
    assert n6 > 0
    zero = dict(to_children=0, to_parents=0, lost=0)
    kids, new, after, store, s1, s2 = cycle(False)
    assert all(kids[int(c)].shape[0] == 0 for c in new) and 6 not in kids
    assert after[6].shape[0] == 0 and s1 == zero and s2 == zero
    assert all(a.size == 0 for a in store.values())
    assert all(_same(after[c], rec[c]) for c in rec if c != 6)

    g.particles_follow_mesh(fld, 3)
    kids, new, after, store_on, s1, s2 = cycle(True)
    assert sum(kids[int(c)].shape[0] for c in new) == n6
    assert s1 == dict(to_children=n6, to_parents=0, lost=0) and s2 == dict(to_children=0, to_parents=n6, lost=0)
    assert np.array_equal(np.sort(after[6], axis=0), np.sort(rec[6], axis=0))
    # the removed store answers as without following: every child's own records
    assert all(_same(store_on[int(c)].reshape(-1, 3), kids[int(c)]) for c in new)
    assert _same(after[6], np.concatenate([kids[int(c)] for c in np.sort(new)]))

    g.particles_follow_mesh(fld, 0)
    kids, new, after, store, s1, s2 = cycle(False)
    assert all(kids[int(c)].shape[0] == 0 for c in new) and after[6].shape[0] == 0
    g.close()


def test_two_fields_each_by_its_own_flag(gpu):
    g, m, fld = _pair((4, 4, 2), R=1)
    other = g.add_variable_field("tags", np.float64, False)
    g.particles_follow_mesh(fld, 3)
    rng = np.random.default_rng(46)
    _seed(g, m, fld, rng, 6)
    other.set([m.cells[int(c)].reshape(-1) for c in g.slot_ids()[: g.n_local]])
    st = _adapt(g, m, refine=(6, 11))
    _check(g, fld, m, st)
    assert st["to_children"] > 0
    tags = _local_cells(g, other, 3)
    for c in m.cells:
        level = int(m.o.mapping.batch([c])["level"][0])
        assert tags[c].shape[0] == (0 if level == 1 else m.cells[c].shape[0])
    assert g.particles_adapt_stats(other) == dict(to_children=0, to_parents=0, lost=0)
    g.close()


def test_refusals_and_lost_records(gpu):
    import dccrg_amd

    g, m, fld = _pair((4, 3, 2), R=1)
    fixed = g.add_field("density", np.float64)
    for bad, match in ((lambda: g.particles_follow_mesh(fixed, 3), "fixed-size"),
                       (lambda: g.particles_follow_mesh(fld, 2), "at least 3 doubles")):
        with pytest.raises(dccrg_amd.DccrgError, match=match) as e:
            bad()
        assert e.value.code == dccrg_amd._lib.EINVAL
    g.particles_follow_mesh(fld, 3)
    rng = np.random.default_rng(47)
    _seed(g, m, fld, rng, 4)
    ctr5, ln5 = m.o.geometry([5])
    m.set(5, (ctr5[0] - ln5[0] / 2) + ln5[0] * rng.random((6, 3)))
    sl = g.slot_ids()[: g.n_local]
    # a cell of 4 doubles: refused before anything changes, the requests kept
    fld.set([np.zeros(4) if int(c) == 9 else m.cells[int(c)].reshape(-1) for c in sl])
    assert g.refine_completely(5)
    with pytest.raises(dccrg_amd.DccrgError, match="not a multiple of 8") as e:
        g.stop_refining()
    assert e.value.code == dccrg_amd._lib.EINVAL
    assert np.array_equal(g.slot_ids()[: g.n_local], sl)
    # a misplaced record (a position in another cell) and a NaN in cell 5
    far = m.o.geometry([24])[0][0]
    assert int(m.locate(far[None, :])[0]) == 24
    n5 = m.cells[5].shape[0]
    m.set(5, np.concatenate([m.cells[5][: n5 // 2], far[None, :], [[0.0, np.nan, 0.0]], m.cells[5][n5 // 2:]]))
    _upload(g, fld, m)
    before = m.total()
    m.o.refine_completely(5)
    new = g.stop_refining()  # the request made before the refusal
    m.o.stop_refining()
    assert new.size == 8
    st = remesh(m)
    assert st == dict(to_children=n5, to_parents=0, lost=2) and m.total() == before - 2
    _check(g, fld, m, st)
    # a stretched geometry given only as a file block: refused like the step
    from oracle import oracle as O

    g.set_geometry_block(O.stretched_geometry_block([[0.0, 0.5, 1.5, 3.0, 5.0], [0.0, 1.0, 2.0, 4.0], [0.0, 1.0, 2.0]]))
    assert g.refine_completely(1)
    with pytest.raises(dccrg_amd.DccrgError, match="stretched geometry"):
        g.stop_refining()
    g.close()


def test_advection_adapt_carries_the_particles(gpu):
    from test_gpu_advection import gpu_grid, prerefine
    from test_gpu_advection_adapt import product_step

    base, R = (16, 16, 16), 2
    g, f = gpu_grid(base, R)
    fld = g.add_variable_field("particles", np.float64, False)
    g.particles_follow_mesh(fld, 3)
    prerefine(g, f, R)
    rng = np.random.default_rng(48)
    sl = g.slot_ids()[: g.n_local]
    ctr, ln = g.geometry(sl)
    pos = (ctr - ln / 2)[:, None, :] + ln[:, None, :] * rng.random((sl.size, 2, 3))
    fld.set(list(pos.reshape(sl.size, 6)))
    before = 2 * sl.size
    assert np.array_equal(g.get_existing_cells_at(pos.reshape(-1, 3)), np.repeat(sl, 2))
    tot = dict(to_children=0, to_parents=0, lost=0)
    for _ in range(4):
        dt = 0.5 * g.advection_max_time_step(f)
        product_step(g, f, dt, 0.025 / R)
        st = g.particles_adapt_stats(fld)
        for k in tot:
            tot[k] += st[k]
    print("advection_adapt", tot)
    assert tot["lost"] == 0 and tot["to_children"] + tot["to_parents"] > 0
    sl = g.slot_ids()[: g.n_local]
    cells = fld.get(0, g.n_local)
    cnt = np.array([a.size // 3 for a in cells])
    assert int(cnt.sum()) == before - tot["lost"]
    assert np.array_equal(g.get_existing_cells_at(np.concatenate(cells).reshape(-1, 3)), np.repeat(sl, cnt))
    g.close()


# ---- several processes (host transport), run by the fixture below -----------
def sc_particles_adapt(rank, world):
    """The refined case across real processes, a third of the cells moved on
    first so that families are split across ranks: three rounds of refine and
    unrefine requests from every rank, a halo and a particle step between
    them.  The cells gathered by id equal the one-address-space model bitwise
    after every stop_refining and every step, and the counts summed over the
    ranks are the model's."""
    from oracle import oracle as O
    from test_gpu_transport import _gather, _grid

    c = REFINED
    o = O.Grid(c["length"], c["R"], c["periodic"], c["hood"], world)
    rng = np.random.default_rng(0)
    for _ in range(c["rounds"]):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        for cell in random_refines(ids, lv, c["R"], rng, c["frac"]):
            o.refine_completely(cell)
        o.stop_refining()
    g = _grid(c["length"], c["R"], c["periodic"], c["hood"])
    g.set_cells(*o.cells())
    g.set_geometry(REF_START, REF_L0)
    loc = g.local_cells()
    mv = loc[loc % np.uint64(3) == 0]
    g.balance_load_to(mv, np.full(mv.size, (rank + 1) % world, np.int32))
    part = _gather(g.local_cells())
    pid = np.concatenate(part)
    pown = np.concatenate([np.full(len(v), r, np.int32) for r, v in enumerate(part)])
    order = np.argsort(pid)
    o.set_cells(pid[order], pown[order])
    m = ParticleModel(o, REF_START, REF_L0)
    fld = g.add_variable_field("particles", np.float64, True)
    g.particles_follow_mesh(fld, 3)
    ctr, ln = o.geometry(m.leaves)
    for cell, r in seeded_particles(m.leaves, ctr, ln, np.random.default_rng(51), 5).items():
        m.set(cell, r)
    _upload(g, fld, m)
    v = tuple(0.9 * np.array([0.9, -0.7, 0.45]) * m.cell_len)
    res = dict(equal=True, stats=True, lost=True, step=True, remote_children=False, merged=False, refined=False)

    def gathered_equal():
        mine = _local_cells(g, fld, 3)
        nr = g.n_slots - g.n_local
        empty = not nr or int(fld.sizes(g.n_local, nr).sum()) == 0
        cells = {}
        parts = _gather((mine, empty))
        for p in parts:
            cells.update(p[0])
        return (sorted(cells) == sorted(m.cells) and all(_same(cells[k], m.cells[k]) for k in cells)
                and all(p[1] for p in parts))

    for rnd in range(3):
        mine = g.local_cells().tolist()
        before = set(mine)
        acts = []
        for cell in mine:
            u = np.random.default_rng(cell * 131 + rnd).random()
            lvl = g.get_refinement_level(cell)
            if lvl > 0 and u < 0.5:
                acts.append((0, cell))
            elif lvl < c["R"] and u > 0.93:
                acts.append((1, cell))
        for k, cell in acts:
            (g.unrefine_completely, g.refine_completely)[k](cell)
        for lst in _gather(acts):
            for k, cell in lst:
                (o.unrefine_completely, o.refine_completely)[k](cell)
        g.stop_refining()
        o.stop_refining()
        st = remesh(m)
        got = _gather(g.particles_adapt_stats(fld))
        res["stats"] = res["stats"] and {k: sum(p[k] for p in got) for k in st} == st
        res["lost"] = res["lost"] and st["lost"] == 0
        res["merged"] = res["merged"] or st["to_parents"] > 0
        res["refined"] = res["refined"] or st["to_children"] > 0
        # (every gather is collective: evaluated before the flag it feeds)
        remote = any(_gather(any(int(x) not in before for x in g.get_removed_cells())))
        res["remote_children"] = res["remote_children"] or remote
        eq = gathered_equal()
        res["equal"] = res["equal"] and eq
        sg = _gather(g.particles_step(fld, 3, v, 0.5, halo=True))
        sm = m.step(v, 0.5)
        res["step"] = res["step"] and sum(p["lost"] for p in sg) == sm["lost"] and sm["lost_known"] == 0
        eq = gathered_equal()
        res["equal"] = res["equal"] and eq
    g.close()
    return res


@pytest.fixture(scope="module")
def adapt_results(gpu, tmp_path_factory):
    from test_gpu_transport import _run_group

    return {w: _run_group(w, tmp_path_factory.mktemp(f"paw{w}"), names=["sc_particles_adapt"],
                          module="test_gpu_particles_adapt") for w in (2, 3)}


@pytest.mark.parametrize("world", [2, 3])
def test_particles_follow_mesh_across_processes(adapt_results, world):
    results = adapt_results[world]
    assert "sc_particles_adapt" in results and len(results["sc_particles_adapt"]) == world
    for rank, (kind, out) in sorted(results["sc_particles_adapt"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"
