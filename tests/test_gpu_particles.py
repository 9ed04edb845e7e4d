"""Device-resident particles (dccrg_amd/csrc/particles.hip) against the model
of tests/particles_model.py.

Results are compared bitwise, per cell id, order included: both sides do the
same IEEE operations in the same order (x + v dt as a rounded product and a
rounded sum, the reference's wrap and index formulas), and the order inside a
cell is specified (stayers, then arrivals by source id and index)."""
import numpy as np
import pytest

from helpers import make_pair
from particles_model import ParticleModel, seeded_particles

pytestmark = pytest.mark.gpu

REF_START, REF_L0 = (-1.0, 0.5, 0.0), (0.5, 0.25, 1.0)
REFINED = dict(length=(8, 6, 4), R=2, periodic=(True, True, False), hood=1, rounds=2, frac=0.1)


def _upload(g, fld, m):
    sl = g.slot_ids()[: g.n_local]
    fld.set([m.cells[int(c)].reshape(-1) for c in sl])


def _local_cells(g, fld, K):
    sl = g.slot_ids()[: g.n_local]
    return {int(c): a.reshape(-1, K) for c, a in zip(sl, fld.get(0, g.n_local))}


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _assert_model(g, fld, m):
    got = _local_cells(g, fld, m.K)
    assert sorted(got) == sorted(m.cells)
    bad = [c for c in got if not _same(got[c], m.cells[c])]
    assert not bad, (bad[:5], got[bad[0]], m.cells[bad[0]])
    nr = g.n_slots - g.n_local
    assert not nr or int(fld.sizes(g.n_local, nr).sum()) == 0


def _pair(length, R=0, periodic=(True, True, True), hood=1, rounds=0, frac=0.1, start=(0, 0, 0), l0=(1, 1, 1), K=3):
    g, o = make_pair(length, R, periodic, hood, rounds, frac)
    g.set_geometry(start, l0)
    m = ParticleModel(o, start, l0, K)
    fld = g.add_variable_field("particles", np.float64, True)
    return g, m, fld


def _seed(g, m, fld, rng, max_per_cell, vmax=None):
    ids = m.leaves
    ctr, ln = m.o.geometry(ids)
    for c, r in seeded_particles(ids, ctr, ln, rng, max_per_cell, m.K, vmax).items():
        m.set(c, r)
    _upload(g, fld, m)


def _run(g, m, fld, steps, velocity, dt):
    tot = dict(stayed=0, moved=0, lost=0, lost_known=0)
    for _ in range(steps):
        st = g.particles_step(fld, m.K, velocity, dt)
        ms = m.step(velocity, dt)
        print("step", st, ms)
        assert (st["stayed"], st["moved"], st["lost"]) == (ms["stayed"], ms["moved"], ms["lost"])
        assert st["arrived"] == 0 and st["handed_over"] == 0
        _assert_model(g, fld, m)
        for k in tot:
            tot[k] += ms[k]
    return tot


def test_reference_scenario(gpu):
    """tests/particles/simple.cpp: 3 x 1 x 1 periodic, neighborhood 1, 50 steps of vx = 0.1."""
    g, m, fld = _pair((3, 1, 1))
    rng = np.random.default_rng(11)
    for c in (1, 2, 3):
        n = int(rng.integers(1, 6))
        m.set(c, np.array([c - 1, 0, 0]) + rng.random((n, 3)))
    _upload(g, fld, m)
    before = m.total()
    tot = _run(g, m, fld, 50, (0.1, 0.0, 0.0), 1.0)
    assert tot["lost"] == 0 and tot["moved"] > 0
    assert m.total() == before
    assert sum(a.shape[0] for a in _local_cells(g, fld, 3).values()) == before
    g.close()


def test_refined_grid(gpu):
    g, m, fld = _pair(start=REF_START, l0=REF_L0, **REFINED)
    _seed(g, m, fld, np.random.default_rng(12), 5)
    v = 2.0 * np.array([0.9, -0.7, 0.45]) * m.cell_len
    tot = _run(g, m, fld, 12, tuple(v), 0.5)
    # a displacement below the finest cell length always lands in neighbors_of
    # at neighborhood length 1: particles leave through the open z faces only
    assert tot["lost_known"] == 0
    assert tot["lost"] > 0 and tot["moved"] > 0
    g.close()


def test_neighborhood_length_0_loses_diagonal_moves(gpu):
    g, m, fld = _pair((4, 4, 4), hood=0)
    _seed(g, m, fld, np.random.default_rng(13), 4)
    tot = _run(g, m, fld, 2, (0.6, 0.6, 0.0), 1.0)
    assert tot["lost_known"] > 0 and tot["moved"] > 0  # the destination exists, but is no face neighbor
    g.close()


def test_neighborhood_length_2_delivers_long_moves(gpu):
    g, m, fld = _pair((6, 5, 4), hood=2)
    _seed(g, m, fld, np.random.default_rng(14), 4)
    before = m.total()
    tot = _run(g, m, fld, 2, (1.9, 0.0, 0.0), 1.0)
    assert tot["lost"] == 0 and tot["stayed"] == 0 and tot["moved"] == 2 * before
    g.close()


def test_one_full_cell_among_empty_cells(gpu):
    """300 particles in the last cell (more than a wave and than a block) and
    five in the first, 1 198 empty cells between them: a block whose particles
    span more slots than it keeps offsets for."""
    g, m, fld = _pair((12, 10, 10))
    rng = np.random.default_rng(15)
    last = int(m.leaves[-1])
    ctr, ln = m.o.geometry([1, last])
    m.set(1, (ctr[0] - ln[0] / 2) + ln[0] * rng.random((5, 3)))
    m.set(last, (ctr[1] - ln[1] / 2) + ln[1] * rng.random((300, 3)))
    _upload(g, fld, m)
    tot = _run(g, m, fld, 3, (0.3, -0.2, 0.25), 1.0)
    assert tot["lost"] == 0 and tot["moved"] > 0
    g.close()


def test_pool_of_20000(gpu):
    g, m, fld = _pair((10, 10, 10), periodic=(True, False, True))
    rng = np.random.default_rng(16)
    ctr, ln = m.o.geometry(m.leaves)
    for c, x, l in zip(m.leaves, ctr, ln):
        m.set(c, (x - l / 2) + l * rng.random((20, 3)))
    _upload(g, fld, m)
    assert m.total() == 20000
    tot = _run(g, m, fld, 2, (0.3, 0.2, -0.1), 1.0)
    assert tot["moved"] > 1000 and tot["lost"] > 0
    g.close()


def test_empty_pool(gpu):
    g, m, fld = _pair((5, 4, 3))
    assert g.particles_step(fld, 3, (0.1, 0.0, 0.0), 1.0) == dict(stayed=0, moved=0, arrived=0, handed_over=0, lost=0)
    _upload(g, fld, m)  # every cell sized to zero records
    assert sum(g.particles_step(fld, 3, (0.1, 0.0, 0.0), 1.0).values()) == 0
    _assert_model(g, fld, m)
    g.close()


def test_every_particle_moves(gpu):
    g, m, fld = _pair((7, 5, 3))
    rng = np.random.default_rng(17)
    ctr, ln = m.o.geometry(m.leaves)
    for c, x, l in zip(m.leaves, ctr, ln):
        m.set(c, (x - l / 2) + l * rng.random((int(rng.integers(0, 7)), 3)) * np.array([0.98, 1, 1]))
    _upload(g, fld, m)
    before = m.total()
    # x < min + 0.98, so min - 1 < x - 0.99 < min: every particle leaves its cell for the next one
    tot = _run(g, m, fld, 2, (-0.99, 0.0, 0.0), 1.0)
    assert tot["stayed"] == 0 and tot["moved"] == 2 * before and tot["lost"] == 0
    g.close()


def test_per_particle_velocities(gpu):
    """K = 6: doubles 3..5 are each particle's velocity and travel unchanged."""
    g, m, fld = _pair(start=REF_START, l0=REF_L0, K=6, **REFINED)
    rng = np.random.default_rng(18)
    _seed(g, m, fld, rng, 5, vmax=1.8 * m.cell_len)
    tags = np.sort(np.concatenate([a[:, 3:6].reshape(-1) for a in m.cells.values()]))
    with pytest.raises(Exception, match="at least 6 doubles"):
        g.particles_step(fld, 3, None, 0.5)
    tot = dict(moved=0, lost=0)
    for _ in range(6):
        st = g.particles_step(fld, 6, None, 0.5)
        ms = m.step(None, 0.5)
        assert (st["stayed"], st["moved"], st["lost"]) == (ms["stayed"], ms["moved"], ms["lost"])
        _assert_model(g, fld, m)
        tot["moved"] += ms["moved"]
        tot["lost"] += ms["lost"]
    assert tot["moved"] > 0
    got = _local_cells(g, fld, 6)
    left = np.sort(np.concatenate([a[:, 3:6].reshape(-1) for a in got.values()]))
    assert np.all(np.isin(left, tags)) and left.size == tags.size - 3 * tot["lost"]
    g.close()


def test_get_existing_cells_at(gpu):
    g, m, fld = _pair(start=REF_START, l0=REF_L0, **REFINED)
    rng = np.random.default_rng(19)
    lo, hi = m.start, m.end
    pts = lo + (hi - lo) * (rng.random((2000, 3)) * 1.5 - 0.25)  # a quarter of the extent outside on either side
    # on cell faces (finest-level planes), exactly at the grid's end and start
    k = rng.integers(0, m.glen.astype(np.int64) + 1, size=(400, 3))
    on_face = rng.random((400, 3)) < 0.5
    pts[:400] = np.where(on_face, lo + k * m.cell_len, pts[:400])
    pts[400:440, 0] = hi[0]
    pts[440:480, 1] = hi[1]
    pts[480:520, 2] = hi[2]
    pts[520:540] = lo
    pts[540] = hi
    pts[541] = np.nan
    exp = m.locate(pts)
    got = g.get_existing_cells_at(pts)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
    assert np.count_nonzero(exp) > 300 and np.count_nonzero(exp == 0) > 300
    assert not exp[400:520].any() and exp[520] != 0
    assert g.get_existing_cells_at(np.zeros((0, 3))).size == 0
    g.close()


def test_refusals(gpu):
    g, m, fld = _pair((4, 3, 2))
    fixed = g.add_field("density", np.float64)
    v = (0.1, 0.0, 0.0)
    with pytest.raises(Exception, match="fixed-size"):
        g.particles_step(fixed, 3, v, 1.0)
    with pytest.raises(Exception, match="at least 3 doubles"):
        g.particles_step(fld, 2, v, 1.0)
    with pytest.raises(Exception, match="at least 6 doubles"):
        g.particles_step(fld, 5, None, 1.0)
    fld.set([np.zeros(3 if s != 2 else 4) for s in range(g.n_local)])
    with pytest.raises(Exception, match="not a multiple of 8"):
        g.particles_step(fld, 3, v, 1.0)
    fld.set([np.zeros(3) for _ in range(g.n_local)])
    assert sum(g.particles_step(fld, 3, v, 1.0).values()) == g.n_local
    from oracle import oracle as O

    g.set_geometry_block(O.stretched_geometry_block([[0.0, 0.5, 1.5, 3.0, 5.0], [0.0, 1.0, 2.0, 4.0], [0.0, 1.0, 2.0]]))
    with pytest.raises(Exception, match="stretched geometry"):
        g.particles_step(fld, 3, v, 1.0)
    with pytest.raises(Exception, match="stretched geometry"):
        g.get_existing_cells_at([[0.5, 0.5, 0.5]])
    g.close()


# ---- several processes (host transport), run by the fixture below -----------
def sc_particles(rank, world):
    """The refined case across real processes with the halo before every step
    and a slab migrating after step 4: the cells gathered by id equal the
    one-address-space model bitwise after every step, handed over == arrived
    and local particles before == after + lost, summed over the ranks."""
    from oracle import oracle as O
    from helpers import random_refines
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
    m = ParticleModel(o, REF_START, REF_L0)
    fld = g.add_variable_field("particles", np.float64, True)
    ctr, ln = o.geometry(m.leaves)
    for cell, r in seeded_particles(m.leaves, ctr, ln, np.random.default_rng(21), 5).items():
        m.set(cell, r)
    _upload(g, fld, m)
    v = tuple(2.0 * np.array([0.9, -0.7, 0.45]) * m.cell_len)
    res = dict(equal=True, handed=True, conserved=True, lost=True, remote=False, migrated=False, crossed=False)
    for step in range(8):
        if step == 4:
            loc = g.local_cells()
            z = g.geometry(loc)[0][:, 2]
            mv = loc[z < 1.0]
            g.balance_load_to(mv, np.full(mv.size, (rank + 1) % world, np.int32))
            res["migrated"] = any(_gather(bool(mv.size)))
        before = sum(a.shape[0] for a in _local_cells(g, fld, 3).values())
        st = g.particles_step(fld, 3, v, 0.5, halo=True)
        ms = m.step(v, 0.5)
        mine = _local_cells(g, fld, 3)
        after = sum(a.shape[0] for a in mine.values())
        nr = g.n_slots - g.n_local
        res["remote"] = res["remote"] or nr > 0
        empty = not nr or int(fld.sizes(g.n_local, nr).sum()) == 0
        parts = _gather((mine, st, before, after, empty))
        cells = {}
        for p in parts:
            cells.update(p[0])
        ok = sorted(cells) == sorted(m.cells) and all(_same(cells[k], m.cells[k]) for k in cells)
        res["equal"] = res["equal"] and ok and all(p[4] for p in parts)
        tot = {k: sum(p[1][k] for p in parts) for k in st}
        res["crossed"] = res["crossed"] or tot["arrived"] > 0
        res["handed"] = res["handed"] and tot["handed_over"] == tot["arrived"]
        res["conserved"] = res["conserved"] and sum(p[2] for p in parts) == sum(p[3] for p in parts) + tot["lost"]
        res["lost"] = res["lost"] and tot["lost"] == ms["lost"] and ms["lost_known"] == 0
    g.close()
    return res


@pytest.fixture(scope="module")
def particle_results(gpu, tmp_path_factory):
    from test_gpu_transport import _run_group

    return {w: _run_group(w, tmp_path_factory.mktemp(f"pw{w}"), names=["sc_particles"], module="test_gpu_particles")
            for w in (2, 3)}


@pytest.mark.parametrize("world", [2, 3])
def test_particles_across_processes(particle_results, world):
    results = particle_results[world]
    assert "sc_particles" in results and len(results["sc_particles"]) == world
    for rank, (kind, out) in sorted(results["sc_particles"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"
