"""Tile sweeps that take the cell lengths from the refinement level
(ensure_len_table, dccrgx_advection_length_source) against the same sweeps
reading the length fields (DCCRGX_LEN_TABLE=0).

On a Cartesian grid the three length fields hold l0[d] * 2^-level; the
library verifies that bitwise for every slot and then stages the lengths
from a per-level table.  The values staged are the bits the fields hold and
the flux expressions are untouched, so every comparison here is bitwise
(np.array_equal), never a tolerance.  The level-0 lengths are distinct and
no powers of two, so a swapped axis or a wrong level changes bits."""
import contextlib
import os

import numpy as np
import pytest

import dccrg_amd
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NAMES = ("density", "vx", "vy", "vz", "lx", "ly", "lz")


def l0_of(base):
    """Distinct level-0 lengths, none a power of two, the domain close to the
    unit cube (the initial hump then refines as in test_gpu_advection.py)."""
    return (1.03 / base[0], 0.97 / base[1], 1.09 / base[2])


@contextlib.contextmanager
def len_table(on):
    old = os.environ.pop("DCCRGX_LEN_TABLE", None)
    if not on:
        os.environ["DCCRGX_LEN_TABLE"] = "0"
    try:
        yield
    finally:
        os.environ.pop("DCCRGX_LEN_TABLE", None)
        if old is not None:
            os.environ["DCCRGX_LEN_TABLE"] = old


def gpu_grid(base, R, periodic=(True, True, False)):
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length(base).set_neighborhood_length(0)
    g.set_maximum_refinement_level(R).set_periodic(*periodic).initialize()
    g.set_geometry((0, 0, 0), l0_of(base))
    f = [g.add_field(n, np.float64, n == "density") for n in NAMES]
    return g, f


def prerefine(g, f, R, relative_diff=0.025, diff_threshold=0.25):
    for _ in range(R):
        g.advection_initialize(f)
        for c in g.advection_refine_candidates(f[0], relative_diff / R, diff_threshold):
            g.refine_completely(int(c))
        g.stop_refining()
    g.advection_initialize(f)


def run(base, R, steps, on, refine=True, edit=None, external=()):
    """`steps` sweeps on a fresh grid (the face table at the first step, tiles
    from the second on); `edit(g, f, k)` runs before step k and may return a
    value that is recorded.  Returns the densities after every step, the
    length source asked after the last step, the layout and what the edits
    returned."""
    with len_table(on):
        g, f = gpu_grid(base, R)
        if refine:
            prerefine(g, f, R)
        else:
            g.advection_initialize(f)
        for k in external:
            f[k].device_ptr()
        dt = g.advection_max_time_step(f)
        out, seen = [], []
        for k in range(steps):
            if edit is not None:
                seen.append(edit(g, f, k))
            g.advection_step(f, 0.5 * dt)
            g.advection_commit(f[0])
            out.append(f[0].get(0, g.n_local))
        src = g.advection_length_source(f)
        lay = g.advection_layout()
        g.close()
    return out, src, lay, seen


# (base, R, refined, what the layout must contain).  (16, 16, 16) with R = 0
# keeps its slots in id order, so its tiles are raster runs and none is a
# regular box; the nearest shape whose tiles are all regular is the same
# uniform mesh with a maximum refinement level of 1 and nothing refined
# (Morton slot order): periodic wrap in x and y, missing sides in z.
SHAPES = [
    ((32, 32, 8), 2, True, ("regular", "general", "finer")),
    ((12, 12, 3), 2, True, ()),
    ((10, 10, 4), 1, True, ()),
    ((16, 16, 16), 0, True, ()),
    ((16, 16, 16), 1, False, ("regular", "all_regular")),
]


@pytest.mark.parametrize("base,R,refine,must", SHAPES)
def test_length_table_bitwise_equals_length_fields(gpu, base, R, refine, must):
    a, src_a, lay, _ = run(base, R, 4, True, refine)
    b, src_b, lay_b, _ = run(base, R, 4, False, refine)
    assert src_a == 1 and src_b == 0
    general = lay["tiles"] - lay["regular_tiles"]
    if "regular" in must:
        assert lay["regular_tiles"] > 0, lay
    if "all_regular" in must:
        assert general == 0, lay
    if "general" in must:
        assert general > 0, lay
    if "finer" in must:
        assert lay["finer_faces"] > 0, lay
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # the bench line's byte count follows the source; SURVEY's counts do not
    assert lay["bytes_needed"] < lay_b["bytes_needed"]
    assert lay["alg_bytes"] == lay_b["alg_bytes"] and lay["alg_bytes_core"] == lay_b["alg_bytes_core"]


FB = ((16, 16, 4), 2)


def test_one_changed_length_falls_back_and_returns(gpu):
    """One local slot of ly rewritten between steps: the sweeps read the
    fields (source 0) and give bitwise what the forced-off run gives, which
    differs from the unedited run; with the old value back the table is used
    again."""
    def edit(g, f, k):
        if k == 2:
            v = f[5].get()
            edit.old = v.copy()
            v[int(np.argmax(f[0].get(0, g.n_local)))] *= 1.5  # the cell at the top of the hump
            f[5].set(v)
            return g.advection_length_source(f)
        if k == 4:
            f[5].set(edit.old)
            return g.advection_length_source(f)
        return g.advection_length_source(f) if k == 1 else None

    a, src, _, seen = run(*FB, 6, True, edit=edit)
    assert seen[1] == 1 and seen[2] == 0 and seen[4] == 1 and src == 1
    b, src_b, _, seen_b = run(*FB, 6, False, edit=edit)
    assert src_b == 0 and seen_b[2] == 0
    c, _, _, _ = run(*FB, 6, True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[3], c[3])  # the edit mattered


def test_scaled_lengths_read_the_fields(gpu):
    def edit(g, f, k):
        if k == 2:
            for j in (4, 5, 6):
                f[j].set(f[j].get() * 1.25)

    a, src, _, _ = run(*FB, 4, True, edit=edit)
    b, _, _, _ = run(*FB, 4, False, edit=edit)
    assert src == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("k_field", [4, 5, 6])
def test_external_length_field_reads_the_fields(gpu, k_field):
    a, src, _, _ = run(*FB, 3, True, external=(k_field,))
    b, _, _, _ = run(*FB, 3, False)
    assert src == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_geometry_block_reads_the_fields(gpu):
    base = FB[0]
    coords = [list(np.linspace(0.0, 1.0, n + 1) ** 2) for n in base]

    def edit(g, f, k):
        if k == 2:
            before = g.advection_length_source(f)
            g.set_geometry_block(O.stretched_geometry_block(coords))
            return before, g.advection_length_source(f)

    a, src, _, seen = run(*FB, 4, True, edit=edit)
    b, _, _, _ = run(*FB, 4, False)
    assert seen[2] == (1, 0) and src == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_other_geometry_reads_the_fields(gpu):
    """set_geometry with other lengths after a verdict of 1, the fields left
    alone: the fields no longer are the geometry's, so they are read."""
    def edit(g, f, k):
        if k == 2:
            before = g.advection_length_source(f)
            g.set_geometry((0, 0, 0), (0.1, 0.07, 0.13))
            return before, g.advection_length_source(f)

    a, src, _, seen = run(*FB, 4, True, edit=edit)
    b, _, _, _ = run(*FB, 4, False)
    assert seen[2] == (1, 0) and src == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def slabs(base, R, P, steps, on):
    """The mesh of a one-rank pre-refined grid split into P z-slabs on
    detached views (as test_gpu_advection.py's four-rank parity test), the
    density halo moved by the library's pack / place."""
    from test_gpu_multirank import emulated_exchange

    with len_table(on):
        ref, rf = gpu_grid(base, R)
        prerefine(ref, rf, R)
        dt = ref.advection_max_time_step(rf)
        leaves = np.sort(ref.slot_ids()[: ref.n_local])
        l0p = np.array([ref.get_cell_from_indices(ref.get_indices(int(c)), 0) for c in leaves], np.int64)
        ref.close()
        owners = ((l0p - 1) * P // int(np.prod(base))).astype(np.int32)
        gs = []
        for r in range(P):
            g = dccrg_amd.Dccrg(r, P, 0).set_initial_length(base).set_neighborhood_length(0)
            g.set_maximum_refinement_level(R).set_periodic(True, True, False).initialize()
            g.set_geometry((0, 0, 0), l0_of(base))
            for n in NAMES:
                g.add_field(n, np.float64, n == "density")
            g.set_cells(leaves, owners)
            g.advection_initialize([g.fields[n] for n in NAMES])
            gs.append(g)
        for _ in range(steps):
            emulated_exchange(gs, ["density"])
            for g in gs:
                f = [g.fields[n] for n in NAMES]
                g.advection_step(f, 0.5 * dt, "inner")
                g.advection_step(f, 0.5 * dt, "outer")
                g.advection_commit(f[0])
        out = [g.fields["density"].get(0, g.n_local) for g in gs]
        src = [g.advection_length_source([g.fields[n] for n in NAMES]) for g in gs]
        outer = [g.counts["outer"] for g in gs]
        tiles = [g.advection_layout()["tiles"] for g in gs]
        for g in gs:
            g.close()
    return out, src, outer, tiles


def test_slabs_with_halo_lengths_bitwise(gpu):
    """Lengths of the remote copies are read as neighbors by the outer tiles:
    the check covers them, and the runs with and without the table agree."""
    a, src_a, outer, tiles = slabs((32, 32, 16), 2, 4, 4, True)
    b, src_b, _, _ = slabs((32, 32, 16), 2, 4, 4, False)
    assert all(s == 1 for s in src_a) and all(s == 0 for s in src_b)
    assert all(n > 0 for n in outer) and all(n > 0 for n in tiles)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
