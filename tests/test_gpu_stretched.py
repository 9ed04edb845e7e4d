"""Stretched_Cartesian_Geometry on the device (dccrgx_set_stretched_geometry):
geometry, point location, particles.

Everything is compared bitwise.  The expected values come from
tests/stretched_model.py, the reference's loops restated on IEEE doubles (and
pinned to the reference itself by tests/test_stretched_ref_cpu.py), and from
tests/golden/stretched_ref.json, the reference's own answers; the device code
restates the same operations in the same order with contraction off."""
import json
import os
import subprocess

import numpy as np
import pytest

import stretched_model as SM
from helpers import make_pair
from test_gpu_particles import _assert_model, _local_cells, _same, _upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_COORDS = 1536  # doubles of coordinates a block keeps in LDS (kCoordCache, particles.hip)
REFINES = dict(rounds=2, frac=0.1)


def _pair(name, K=3, hood=1, rounds=2, frac=0.1):
    """The case's refined grid with its stretched geometry, the model, a
    particle field."""
    R, coords = SM.case_coords(name)
    g, o = make_pair(SM.LENGTH, R, SM.PERIODIC, hood, rounds, frac)
    g.set_stretched_geometry(coords)
    m = SM.StretchedParticleModel(o, coords, K)
    fld = g.add_variable_field("particles", np.float64, True)
    return g, m, fld, coords, R


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "stretched_ref.json")) as f:
        raw = json.load(f)
    out = {}
    for name in SM.CASES:
        R, coords = SM.case_coords(name)
        pts = SM.point_set(coords, R)
        out[name] = SM.unpack(R, pts[~SM.at_first_coordinate(coords, pts)], raw[name])
    return out


# ---- point location --------------------------------------------------------------
@pytest.mark.parametrize("name", SM.CASES)
def test_locate(gpu, name):
    g, m, _, coords, R = _pair(name)
    pts = SM.point_set(coords, R)
    exp = m.locate(pts)
    got = g.get_existing_cells_at(pts)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (bad[:10], pts[bad[:10]], got[bad[:10]], exp[bad[:10]])
    assert np.count_nonzero(exp) > 1000 and np.count_nonzero(exp == 0) > 100
    # the first boundary belongs to the first cell (the facade's rule), wrapped points are found
    first = SM.at_first_coordinate(coords, pts)
    assert first.any() and np.count_nonzero(exp[first]) > 0
    g.close()


def test_rounding_quirk_is_kept(gpu):
    """c0 + 2^R li < c1 in x's second and z's last level-0 cell of the
    'rounded' case: x's third boundary belongs to the third cell, z's end is
    one index past the grid."""
    g, m, _, coords, R = _pair("rounded", rounds=0)
    mid = [(c[0] + c[-1]) / 2 for c in coords]
    pts = np.array([[coords[0][2], mid[1], mid[2]], [mid[0], mid[1], coords[2][2]], [coords[0][1], mid[1], mid[2]]])
    exp = m.locate(pts)
    ind = SM.indices_of(coords, R, m.real_coordinate(pts))
    assert ind[0, 0] == 2 << R and ind[1, 2] == 2 << R and ind[2, 0] == (1 << R) - 1
    assert exp[1] == 0 and exp[0] != 0 and exp[2] != 0
    assert np.array_equal(g.get_existing_cells_at(pts), exp)
    g.close()


def test_coordinates_searched_in_global_memory(gpu):
    """More coordinates than a block keeps in LDS: base (cap + 3, 1, 1)."""
    n = LDS_COORDS + 3
    rng = np.random.default_rng(31)
    coords = [np.concatenate([[-3.0], -3.0 + np.cumsum(0.05 + rng.random(n))]), np.array([0.0, 1.0]),
              np.array([2.0, 2.5])]
    assert sum(c.size for c in coords) > LDS_COORDS
    g, o = make_pair((n, 1, 1), 0, (True, False, True), 1)
    g.set_stretched_geometry(coords)
    m = SM.StretchedParticleModel(o, coords)
    cx = coords[0]
    pick = np.concatenate([np.arange(0, 20), np.arange(20, n - 20, 7), np.arange(n - 20, n + 1)])
    v = np.concatenate([cx[pick], np.nextafter(cx[pick], -np.inf), np.nextafter(cx[pick], np.inf),
                        cx[0] + (cx[-1] - cx[0]) * (rng.random(300) * 1.5 - 0.25)])
    pts = np.stack([v, rng.random(v.size), 2.0 + 0.5 * rng.random(v.size)], axis=1)
    exp = m.locate(pts)
    got = g.get_existing_cells_at(pts)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
    assert np.unique(exp).size > 200
    # the particle step's locate pass on the same path
    fld = g.add_variable_field("particles", np.float64, True)
    ctr, ln = m.geometry(m.leaves)
    for c, x, l in zip(m.leaves[::9], ctr[::9], ln[::9]):
        m.set(c, (x - l / 2) + l * rng.random((3, 3)))
    _upload(g, fld, m)
    _run(g, m, fld, 2, (0.04, 0.0, 0.1), 1.0)
    g.close()


# ---- geometry ------------------------------------------------------------------------
@pytest.mark.parametrize("name", SM.CASES)
def test_geometry_and_fill(gpu, golden, name):
    g, m, _, coords, R = _pair(name)
    ids = g.slot_ids()
    G = golden[name]
    row = ids.astype(np.int64) - 1  # the golden file: every possible cell, by id
    ctr, ln = g.geometry(ids)
    assert SM.same_bits(ctr, G["center"][row]) and SM.same_bits(ln, G["length"][row])
    mc, ml = m.geometry(ids)
    assert SM.same_bits(mc, ctr) and SM.same_bits(ml, ln)
    bad_c, bad_l = g.geometry([0, int(g.get_last_cell()) + 1])
    assert np.isnan(bad_c).all() and np.isnan(bad_l).all()
    f = [g.add_field(n, np.float64, n == "density") for n in ("density", "vx", "vy", "vz", "lx", "ly", "lz")]
    cf = [g.add_field(n, np.float64, False) for n in ("cx", "cy", "cz")]
    g.fill_geometry(center=cf, length=f[4:7])
    for d in range(3):
        assert SM.same_bits(cf[d].get(0, g.n_slots), G["center"][row, d])
        assert SM.same_bits(f[4 + d].get(0, g.n_slots), G["length"][row, d])
    assert g.advection_length_source(f) == 0
    # one component alone, the others untouched
    cf[1].set(np.zeros(g.n_slots))
    g.fill_geometry(center=[cf[0], None, None])
    assert not cf[1].get(0, g.n_slots).any() and SM.same_bits(cf[0].get(0, g.n_slots), G["center"][row, 0])
    g.fill_geometry(length=[None, f[5], None])
    g.fill_geometry()
    with pytest.raises(Exception, match="fp64"):
        g.fill_geometry(center=[g.add_field("u32", np.uint32), None, None])
    with pytest.raises(Exception, match="twice"):
        g.fill_geometry(center=[cf[0], cf[0], None])
    cf[2].device_ptr()
    with pytest.raises(Exception, match="handed out"):
        g.fill_geometry(center=cf)
    g.close()


def test_fill_on_a_cartesian_grid(gpu):
    """Filled length fields are bitwise advection_initialize's, so the sweeps'
    length table accepts them; the centers are geometry()'s."""
    from test_gpu_advection_lengths import gpu_grid, prerefine

    g, f = gpu_grid((12, 12, 3), 2)
    prerefine(g, f, 2)
    ns = g.n_slots
    assert g.advection_length_source(f) == 1
    want = [f[4 + d].get(0, ns) for d in range(3)]
    assert len({float(v) for v in want[0]}) > 1  # several levels
    for d in range(3):
        f[4 + d].set(np.zeros(ns))
    assert g.advection_length_source(f) == 0
    cf = [g.add_field(n, np.float64, False) for n in ("cx", "cy", "cz")]
    g.fill_geometry(center=cf, length=f[4:7])
    for d in range(3):
        assert SM.same_bits(f[4 + d].get(0, ns), want[d])
    assert g.advection_length_source(f) == 1
    ctr, ln = g.geometry(g.slot_ids())
    for d in range(3):
        assert SM.same_bits(cf[d].get(0, ns), ctr[:, d]) and SM.same_bits(want[d], ln[:, d])
    g.close()


# ---- the C ABI's rules -----------------------------------------------------------------
def test_refusals_leave_the_geometry_unchanged(gpu):
    import dccrg_amd

    R, coords = SM.case_coords("exact")
    g, o = make_pair(SM.LENGTH, R, SM.PERIODIC, 1)
    assert g.stretched_geometry() is None and g.geometry_block() == b""

    def refused(bad, dim):
        with pytest.raises(dccrg_amd.DccrgError, match=f"dimension {dim}") as e:
            g.set_stretched_geometry(bad)
        assert e.value.code == dccrg_amd._lib.EINVAL

    def bad_sets():
        refused([coords[0][:-1], coords[1], coords[2]], 0)  # a wrong count
        refused([coords[0], np.append(coords[1], 9.0), coords[2]], 1)
        refused([coords[0], coords[1], np.array([0.0, 1.0, 1.0])], 2)  # not increasing
        refused([np.array([0.0, 0.5, 0.25, 3.0, 5.0]), coords[1], coords[2]], 0)
        refused([coords[0], np.array([0.0, np.nan, 2.0, 4.0]), coords[2]], 1)  # NaN
        refused([coords[0], coords[1], np.array([0.0, 1.0, np.inf])], 2)

    bad_sets()
    assert g.stretched_geometry() is None and g.geometry_block() == b""
    c0, l0 = g.geometry([5])
    g.set_stretched_geometry(coords)
    block = g.geometry_block()
    bad_sets()
    got = g.stretched_geometry()
    assert all(np.array_equal(a, b) for a, b in zip(got, coords)) and g.geometry_block() == block
    c1, l1 = g.geometry([5])
    assert not np.array_equal(l0, l1)
    bad_sets()
    assert np.array_equal(g.geometry([5])[1], l1)
    g.close()


def test_file_block_save_load_adopt(gpu, tmp_path):
    import dccrg_amd
    from oracle import oracle as O

    g, m, _, coords, R = _pair("rounded")
    assert g.geometry_block() == O.stretched_geometry_block(coords) == SM.geometry_block(coords)
    a = g.add_field("a", np.uint32)
    a.set(np.arange(g.n_slots, dtype=np.uint32))
    pts = SM.point_set(coords, R, n_random=300)
    want = g.get_existing_cells_at(pts)
    assert np.array_equal(want, m.locate(pts))
    path = tmp_path / "stretched.dc"
    g.save_grid_data(path)
    exp_block = O.grid_block_stretched_bytes(SM.LENGTH, R, 1, SM.PERIODIC, coords)
    assert exp_block in path.read_bytes()
    h = dccrg_amd.Dccrg(0, 1, 0)
    h.add_field("a", np.uint32)
    h.load_grid_data(path)
    # a loaded block is a file block only, as before
    assert h.stretched_geometry() is None and h.geometry_block() == g.geometry_block()
    with pytest.raises(Exception, match="stretched geometry"):
        h.get_existing_cells_at(pts)
    h.adopt_geometry_block()
    assert all(np.array_equal(x, y) for x, y in zip(h.stretched_geometry(), coords))
    assert np.array_equal(h.get_existing_cells_at(pts), want)
    # set_geometry_block drops the coordinates again
    h.set_geometry_block(g.geometry_block())
    assert h.stretched_geometry() is None
    with pytest.raises(Exception, match="stretched geometry"):
        h.get_existing_cells_at(pts)
    with pytest.raises(Exception, match="no stretched geometry block"):
        dccrg_amd.Dccrg(0, 1, 0).adopt_geometry_block()
    g.close()
    h.close()


def test_set_geometry_returns_to_cartesian(gpu):
    from particles_model import ParticleModel

    g, m, _, coords, R = _pair("exact")
    pts = SM.point_set(coords, R, n_random=300)
    assert np.array_equal(g.get_existing_cells_at(pts), m.locate(pts))
    start, l0 = (-1.0, 0.5, 0.0), (0.5, 0.25, 1.0)
    g.set_geometry(start, l0)
    assert g.stretched_geometry() is None and g.geometry_block() == b""
    cm = ParticleModel(m.o, start, l0)
    assert np.array_equal(g.get_existing_cells_at(pts), cm.locate(pts))
    ids = g.slot_ids()
    ctr, ln = g.geometry(ids)
    oc, ol = m.o.geometry(ids)
    assert SM.same_bits(ctr, oc) and SM.same_bits(ln, ol)
    # a block given as bytes stays through set_geometry, as before
    g.set_geometry_block(SM.geometry_block(coords))
    g.set_geometry(start, l0)
    assert g.geometry_block() == SM.geometry_block(coords)
    g.close()


# ---- the particle step ---------------------------------------------------------------------
def _run(g, m, fld, steps, velocity, dt):
    tot = dict(stayed=0, moved=0, lost=0, lost_known=0)
    for _ in range(steps):
        st = g.particles_step(fld, m.K, velocity, dt)
        ms = m.step(velocity, dt)
        assert st == dict(stayed=ms["stayed"], moved=ms["moved"], arrived=0, handed_over=0, lost=ms["lost"]), (st, ms)
        _assert_model(g, fld, m)
        for k in tot:
            tot[k] += ms[k]
    return tot


def _seed(g, m, fld, rng, max_per_cell, vmax=None):
    from particles_model import seeded_particles

    ctr, ln = m.geometry(m.leaves)
    for c, r in seeded_particles(m.leaves, ctr, ln, rng, max_per_cell, m.K, vmax).items():
        m.set(c, r)
    _upload(g, fld, m)


@pytest.mark.parametrize("name", SM.CASES)
def test_particles_uniform_velocity(gpu, name):
    g, m, fld, coords, R = _pair(name)
    _seed(g, m, fld, np.random.default_rng(41), 5)
    v = 2.0 * 1.2 * np.array([0.9, -0.7, 1.0]) * m.smallest  # |v dt| up to 1.2 of the smallest cell
    tot = _run(g, m, fld, 10, tuple(v), 0.5)
    assert tot["moved"] > 0 and tot["stayed"] > 0 and tot["lost"] > 0  # (y is not periodic)
    g.close()


def test_particles_own_velocities(gpu):
    g, m, fld, coords, R = _pair("exact", K=6)
    _seed(g, m, fld, np.random.default_rng(42), 5, vmax=2.0 * 1.2 * m.smallest)
    tot = _run(g, m, fld, 10, None, 0.5)
    assert tot["moved"] > 0 and tot["stayed"] > 0
    g.close()


def test_one_full_cell_among_empty_cells(gpu):
    """300 particles (more than a block pass) in one cell, none elsewhere."""
    g, m, fld, coords, R = _pair("rounded")
    rng = np.random.default_rng(43)
    cell = int(m.leaves[m.leaves.size // 2])
    ctr, ln = m.geometry([cell])
    m.set(cell, (ctr[0] - ln[0] / 2) + ln[0] * rng.random((300, 3)))
    _upload(g, fld, m)
    tot = _run(g, m, fld, 3, tuple(0.4 * ln[0] * np.array([1.0, -1.0, 1.0])), 1.0)
    assert tot["moved"] > 0
    g.close()


# ---- several processes (host transport), run by the fixture below -----------------------------
def sc_stretched_particles(rank, world):
    """The refined 'exact' case across real processes with the halo before
    every step and a slab migrating after step 3: the cells gathered by id
    equal the one-address-space model bitwise after every step."""
    from oracle import oracle as O
    from helpers import random_refines
    from particles_model import seeded_particles
    from test_gpu_transport import _gather, _grid

    R, coords = SM.case_coords("exact")
    o = O.Grid(SM.LENGTH, R, SM.PERIODIC, 1, world)
    rng = np.random.default_rng(0)
    for _ in range(REFINES["rounds"]):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        for cell in random_refines(ids, lv, R, rng, REFINES["frac"]):
            o.refine_completely(cell)
        o.stop_refining()
    g = _grid(SM.LENGTH, R, SM.PERIODIC, 1)
    g.set_cells(*o.cells())
    g.set_stretched_geometry(coords)
    m = SM.StretchedParticleModel(o, coords)
    fld = g.add_variable_field("particles", np.float64, True)
    ctr, ln = m.geometry(m.leaves)
    for cell, r in seeded_particles(m.leaves, ctr, ln, np.random.default_rng(44), 5).items():
        m.set(cell, r)
    _upload(g, fld, m)
    v = tuple(2.0 * 1.2 * np.array([0.9, -0.7, 1.0]) * m.smallest)
    res = dict(equal=True, handed=True, conserved=True, lost=True, remote=False, migrated=False, crossed=False)
    for step in range(6):
        if step == 3:
            loc = g.local_cells()
            x = g.geometry(loc)[0][:, 0]
            mv = loc[x < 1.5]
            g.balance_load_to(mv, np.full(mv.size, (rank + 1) % world, np.int32))
            res["migrated"] = any(_gather(bool(mv.size)))
        before = sum(a.shape[0] for a in _local_cells(g, fld, 3).values())
        st = g.particles_step(fld, 3, v, 0.5, halo=True)
        ms = m.step(v, 0.5)
        mine = _local_cells(g, fld, 3)
        after = sum(a.shape[0] for a in mine.values())
        res["remote"] = res["remote"] or g.n_slots > g.n_local
        parts = _gather((mine, st, before, after))
        cells = {}
        for p in parts:
            cells.update(p[0])
        ok = sorted(cells) == sorted(m.cells) and all(_same(cells[k], m.cells[k]) for k in cells)
        res["equal"] = res["equal"] and ok
        tot = {k: sum(p[1][k] for p in parts) for k in st}
        res["crossed"] = res["crossed"] or tot["arrived"] > 0
        res["handed"] = res["handed"] and tot["handed_over"] == tot["arrived"]
        res["conserved"] = res["conserved"] and sum(p[2] for p in parts) == sum(p[3] for p in parts) + tot["lost"]
        res["lost"] = res["lost"] and tot["lost"] == ms["lost"]
    g.close()
    return res


def test_particles_across_two_processes(gpu, tmp_path):
    from test_gpu_transport import _run_group

    results = _run_group(2, tmp_path, names=["sc_stretched_particles"], module="test_gpu_stretched")
    assert len(results.get("sc_stretched_particles", {})) == 2
    for rank, (kind, out) in sorted(results["sc_stretched_particles"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"


# ---- the facade ----------------------------------------------------------------------------------
def test_facade_locates_like_its_host_geometry(gpu):
    """examples/stretched_locate.cpp: Dccrg<Cell, Stretched_Cartesian_Geometry>::
    get_existing_cell(coordinate), answered on the device, against
    geometry.get_indices + get_existing_cell(indices) on the host."""
    exe = os.path.join(ROOT, "examples", "bin", "stretched_locate")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} missing: run __graft_entry__.build() first")
    r = subprocess.run(["/opt/conda/bin/mpiexec", "-n", "1", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "located" and int(words[1]) > 150 and int(words[3]) > 100 and int(words[5]) == 0, r.stdout
