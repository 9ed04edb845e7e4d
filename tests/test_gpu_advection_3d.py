"""The advection sweeps with three non-zero velocity components, level jumps
across z faces, a periodic z axis and distinct cell lengths, against the
plain model of tests/advection_model.py (which tests/test_advection_model_cpu.py
holds to the oracle within 1e-12 on these same meshes and states).

Everywhere else in the suite the state is the reference's own: vz = 0, no
dependence on z, lx == ly.  There every z-face flux is rho * dt * 0 * area on
both sides of every comparison, so a wrong z neighbor, sign, area, staged vz
or level on a z face leaves every assertion green.  Here each sweep kernel
is checked per cell after each of 4 steps of 0.5 dt:
|gpu - model| <= 1e-12 * max|model|, the model fed its own previous output,
and advection_max_time_step is bitwise the model's.

Kernel paths (PATHS), each on every mesh of MESHES where it can be reached:
  table    the default: the face table at the first step, the length-table
           tile kernels from the second (length source 1)
  fields   DCCRGX_LEN_TABLE=0: the field-reading tile kernels (source 0)
  free     every cell its own three lengths: source 0 on its own
  nbrec    DCCRGX_NBREC=1: the neighbor records
  bands    one advection_check_adaptation before the first step, so the face
           table sweep also writes the bands (advection_ell_lds_kernel<true>);
           a grid without refinement levels has no check
  tiles1   tiles built before the first step (advection_layout), so the tile
           kernels also see the first step's state
  vz0      vz exactly 0 in a tenth of the cells (the isnormal rule of the
           time step; a zero face velocity), on three meshes
DCCRGX_TILES is the only switch read once per process: a test cannot flip
it, so its two overrides are not covered.

Meshes, with what advection_layout() must report so that a mesh cannot
silently stop exercising its kernel: see LAYOUT."""
import contextlib
import functools

import numpy as np
import pytest

import advection_model as M
import dccrg_amd
from test_advection_model_cpu import (CASES, MESHES, STEPS_GPU, case_id, cross_level_z_faces, mesh, overcap_cells,
                                      trajectory, zhalf_cells)
from test_gpu_advection_lds import nested
from test_gpu_advection_lengths import NAMES, gpu_grid, l0_of, len_table, prerefine

pytestmark = pytest.mark.gpu

TOL = 1e-12
PATHS = ("table", "fields", "free", "nbrec", "bands", "tiles1", "vz0")
VZ0_ON = ("prerefined", "zhalf", "raster")


def reachable(name, path):
    if path == "bands":  # check_for_adaptation returns at once without refinement levels: no bands to write
        return MESHES[name][1] > 0
    return path != "vz0" or name in VZ0_ON


RUNS = [(name, per, path) for name, per in CASES for path in PATHS if reachable(name, path)]


def refine_cells(cells, g, f):
    for c in cells:
        g.refine_completely(int(c))
    g.stop_refining()
    g.advection_initialize(f)


MAKE = {
    "prerefined": lambda g, f: prerefine(g, f, 2),
    "nested": nested,
    "zhalf": lambda g, f: refine_cells(zhalf_cells(), g, f),
    "zwide": lambda g, f: refine_cells(zhalf_cells((16, 8, 16)), g, f),
    "uniform": lambda g, f: g.advection_initialize(f),
    "raster": lambda g, f: g.advection_initialize(f),
    "overcap": lambda g, f: refine_cells(overcap_cells(), g, f),
}


def check_layout(name, lay):
    """LAYOUT: what each mesh must make the library do."""
    general = lay["tiles"] - lay["regular_tiles"]
    assert lay["tiles"] > 0, lay
    if name == "prerefined":  # general tiles of three levels, finer faces
        assert lay["finer_faces"] > 0 and general > 0, lay
    elif name == "nested":  # four levels in general tiles
        assert lay["finer_faces"] > 0 and general > 0 and lay["ext_max"] <= 1024, lay
    elif name == "zhalf":
        # a level-0 8^3 box whose two z sides face refined cells: 512 out-of-tile
        # neighbors, all across z (its x and y neighbors are its own cells, by the wrap)
        assert lay["ext_max"] == 512 and lay["finer_faces"] == 128, lay
    elif name == "zwide":
        # two such boxes side by side in x: 640 out-of-tile neighbors each, more
        # than the 512 columns the general kernel stages with its own cells
        assert 512 < lay["ext_max"] <= 1024 and lay["finer_faces"] == 256, lay
    elif name == "uniform":  # all tiles regular: z wrap between regular tiles (TTT), missing z sides (TTF)
        assert general == 0 and lay["regular_tiles"] == 8, lay
    elif name == "raster":  # id-ordered slots: raster runs, no regular tile
        assert lay["regular_tiles"] == 0, lay
    elif name == "overcap":  # a tile beyond the tile kernel's 1024 neighbors: the untiled advection_kernel
        assert lay["ext_max"] > 1024, lay
    else:
        raise AssertionError(name)


def by_id(sorted_ids, values, ids):
    k = np.searchsorted(sorted_ids, ids)
    assert np.array_equal(sorted_ids[k], ids)
    return k, values[k]


def upload_state(g, f, sorted_ids, cols, lengths_too):
    """rho, vx, vy, vz (and the lengths) of every slot, remote copies
    included, by id.  Returns the local slots' positions in sorted_ids."""
    slots = g.slot_ids()
    assert slots.size == g.n_slots
    k, vals = by_id(sorted_ids, cols, slots)
    if not lengths_too:
        # the library's own lengths (advection_initialize) are the model's, bitwise
        for j in (4, 5, 6):
            assert np.array_equal(f[j].get(), vals[:, j]), NAMES[j]
    for j in range(7 if lengths_too else 4):
        f[j].set(np.ascontiguousarray(vals[:, j]))
    return k[: g.n_local]


def compare(got, model, where, step, label):
    exp = model[where].astype(np.float64)
    scale = float(np.max(np.abs(model)))
    ratio = float(np.max(np.abs(got - exp))) / scale
    print(f"{label} step {step}: |gpu - model| / max|model| = {ratio:.3e}")
    assert ratio <= TOL, (label, step, ratio, int(np.argmax(np.abs(got - exp))))


@contextlib.contextmanager
def nbrec(monkeypatch, on):
    """DCCRGX_NBREC is read per call (as test_gpu_advection.nbrec_on sets it)."""
    if on:
        monkeypatch.setenv("DCCRGX_NBREC", "1")
    else:
        monkeypatch.delenv("DCCRGX_NBREC", raising=False)
    try:
        yield
    finally:
        monkeypatch.delenv("DCCRGX_NBREC", raising=False)


@functools.lru_cache(maxsize=None)
def mesh_facts(name, periodic):
    """What the table of meshes states about the leaf set, from the model's
    faces (the GPU grid's leaves are asserted to be these)."""
    ids, lvl, F = mesh(name, periodic)
    if name == "nested":
        assert set(np.unique(lvl)) == {0, 1, 2, 3} and cross_level_z_faces(lvl, F) == 704
    if name == "zhalf":
        assert int(np.sum(lvl == 0)) == 512 and cross_level_z_faces(lvl, F) == 1024
    if name == "zwide":
        assert int(np.sum(lvl == 0)) == 1024 and cross_level_z_faces(lvl, F) == 2048
    if name == "overcap":
        assert int(np.sum(lvl == 0)) == 512 and cross_level_z_faces(lvl, F) == 1024
    return True


@pytest.mark.parametrize("name,periodic,path", RUNS, ids=case_id)
def test_sweeps_match_the_model(gpu, monkeypatch, name, periodic, path):
    base, R = MESHES[name][:2]
    variant = path if path in ("free", "vz0") else "full"
    ids, lvl, F = mesh(name, periodic)
    assert mesh_facts(name, periodic)
    cols, dt, model = trajectory(name, periodic, variant, STEPS_GPU)
    label = f"{name} {case_id(periodic)} {path}"
    with len_table(path != "fields"), nbrec(monkeypatch, path == "nbrec"):
        g, f = gpu_grid(base, R, periodic)
        MAKE[name](g, f)
        assert np.array_equal(np.sort(g.slot_ids()[: g.n_local]), ids)
        where = upload_state(g, f, ids, cols, variant == "free")
        assert g.advection_max_time_step(f) == dt
        if path == "tiles1":
            check_layout(name, g.advection_layout())
        if path == "bands":
            g.advection_check_adaptation(f[0], 0.025 / R)
        for k in range(STEPS_GPU):
            g.advection_step(f, 0.5 * dt)
            g.advection_commit(f[0])
            compare(f[0].get(0, g.n_local), model[k], where, k, label)
        src = g.advection_length_source(f)
        assert src == (0 if path in ("fields", "free", "nbrec") else 1), (label, src)
        check_layout(name, g.advection_layout())
        assert g.advection_max_time_step(f) == dt  # the velocities and lengths are untouched
        g.close()


@pytest.mark.parametrize("axis", [0, 2], ids=["x", "z"])
def test_two_ranks_match_the_model(gpu, axis):
    """The nested mesh cut by an x plane (or a z plane) into two ranks on
    detached views (the periodic wrap of that axis crosses ranks too), the
    density halo moved by the library's pack / place: the haloed densities
    enter non-zero fluxes, through level jumps too.  Velocities and lengths of
    the remote copies are set as well; every local cell against the model
    after every step."""
    from test_gpu_multirank import emulated_exchange

    name, periodic = "nested", (True, True, True)
    base, R = MESHES[name][:2]
    ids, lvl, F = mesh(name, periodic)
    cols, dt, model = trajectory(name, periodic, "full", STEPS_GPU)
    _, lo, _ = M.boxes(ids, base, R)
    # by the level-0 parent, so families stay whole.  The nested blocks are symmetric about the middle
    # plane of each axis (the same level on both its sides), so the cut lies one level-0 cell beside it,
    # where cells of different levels face each other
    owners = (lo[:, axis] >= (base[axis] // 2 - 1) << R).astype(np.int32)
    # only faces of that axis cross the cut (the wrap included), level jumps among them
    cross = owners[F[:, 0]] != owners[F[:, 2]]
    jump = lvl[F[:, 0]] != lvl[F[:, 2]]
    assert np.any(cross & jump) and np.any(cross & ~jump) and np.all(F[cross, 1] >> 1 == axis)
    assert np.any(~cross & jump & (F[:, 1] >= 4))  # z level jumps within a rank (with the z cut: besides)
    gs, wheres = [], []
    for r in range(2):
        g = dccrg_amd.Dccrg(r, 2, 0).set_initial_length(base).set_neighborhood_length(0)
        g.set_maximum_refinement_level(R).set_periodic(*periodic).initialize()
        g.set_geometry((0, 0, 0), l0_of(base))
        f = [g.add_field(n, np.float64, n == "density") for n in NAMES]
        g.set_cells(ids, owners)
        g.advection_initialize(f)
        assert np.array_equal(np.sort(g.slot_ids()[: g.n_local]), ids[owners == r])
        assert g.counts["outer"] > 0 and g.n_slots > g.n_local
        wheres.append(upload_state(g, f, ids, cols, False))
        gs.append(g)
    for k in range(STEPS_GPU):
        emulated_exchange(gs, ["density"])
        for r, g in enumerate(gs):
            f = [g.fields[n] for n in NAMES]
            g.advection_step(f, 0.5 * dt, "inner")
            g.advection_step(f, 0.5 * dt, "outer")
            g.advection_commit(f[0])
        for r, g in enumerate(gs):
            compare(g.fields["density"].get(0, g.n_local), model[k], wheres[r], k, f"{name} cut {'xyz'[axis]} rank {r}")
    for g in gs:
        g.close()
