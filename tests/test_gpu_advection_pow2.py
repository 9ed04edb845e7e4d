"""Tile sweeps that multiply by a reciprocal where the divisor is a power of
two (Grid::LenTable::pow2, dccrgx_advection_divide_source) against the same
build dividing everywhere (DCCRGX_DIV_POW2=0).

With level-0 cell lengths that are powers of two, the divisor of a face
between two cells of one level (2 l_a) and a cell's volume are powers of two
at every level, their reciprocals are exact, and a product with an exact
reciprocal rounds the real number the quotient rounds.  So every comparison
here is of the 64-bit patterns (np.array_equal on the uint64 views, NaN
payloads included), never a tolerance.  The level-0 lengths differ per axis
(1/32, 1/16, 1/8 and the like), so a reciprocal taken from another axis or
another level changes bits.

Four sweeps per run: the first is the face table's (it divides, in both
runs), the other three the tile kernels'.  Every run asserts what it ran:
the divide source, the length source, the velocity mask and the kinds of
tile in the layout, so a fall-back cannot pass for the path under test."""
import contextlib
import functools
import os

import numpy as np
import pytest

from test_gpu_advection_lengths import FB, gpu_grid, l0_of, prerefine
from test_gpu_advection_uniform import MESH, set_velocities

pytestmark = pytest.mark.gpu

STEPS = 4

# powers of two, distinct per axis, the hump of advection_initialize (center
# (0.25, 0.5), radius 0.15) inside the domain
L0 = {
    "prerefined": (1 / 32, 1 / 16, 1 / 8),
    "nested": (1 / 8, 1 / 4, 1 / 2),
    "ext1024": (1 / 16, 1 / 8, 1 / 4),
    "one_tile": (1 / 8, 1 / 4, 1 / 2),
    "all_regular": (1 / 16, 1 / 8, 1 / 32),
    "fb": (1 / 16, 1 / 8, 1 / 4),
}


@contextlib.contextmanager
def div_pow2(on):
    old = os.environ.pop("DCCRGX_DIV_POW2", None)
    if not on:
        os.environ["DCCRGX_DIV_POW2"] = "0"
    try:
        yield
    finally:
        os.environ.pop("DCCRGX_DIV_POW2", None)
        if old is not None:
            os.environ["DCCRGX_DIV_POW2"] = old


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def f64(pattern):
    return np.array([pattern], np.uint64).view(np.float64)[0]


# +-inf, NaNs with a payload of either sign, +-0, the smallest subnormal of
# either sign, 1e-300-scale values
SPECIAL = [np.inf, -np.inf, f64(0x7FF8000000000ABC), f64(0xFFF8000000000123), 0.0, -0.0, 5e-324, -5e-324, 1e-300,
           -3e-300, 7e-301]


def jump_groups(g):
    """Slots beside a level jump: the first and the last local cell with a
    finer face neighbor, each with all its face neighbors (the finer ones and
    those of its own or a coarser level)."""
    ids = [int(c) for c in g.slot_ids()[: g.n_local]]
    slot = {c: s for s, c in enumerate(ids)}
    groups = []
    for order in (range(len(ids)), range(len(ids) - 1, -1, -1)):
        for s in order:
            lv = g.get_refinement_level(ids[s])
            nbs = [n for n, _ in g.get_face_neighbors_of(ids[s])]
            if any(g.get_refinement_level(n) > lv for n in nbs):
                groups.append([s] + [slot[n] for n in nbs if n in slot])
                break
    assert len(groups) == 2 and all(len(q) > 5 for q in groups), groups
    return groups


def set_special(g, f, fields):
    """The special values into `fields` (indices into f) at the cells beside
    two level jumps and at a few slots spread over the mesh (cells of regular
    tiles among them), each field with the list shifted by one."""
    n = g.n_local
    slots = [s for q in jump_groups(g) for s in q] + list(range(3, n, max(1, n // 23)))
    for j, k in enumerate(fields):
        v = f[k].get()
        for i, s in enumerate(slots):
            v[s] = SPECIAL[(i + j) % len(SPECIAL)]
        f[k].set(v)
    return len(slots)


def run(name, l0, mask, on, steps=STEPS, edit=None, special=()):
    """`steps` sweeps of mesh `name` with level-0 lengths l0 and the velocity
    components of `mask` uniform (None: as advection_initialize leaves them,
    vz = 0); `special`: the fields that get the special values, after the
    time step is taken; `edit(g, f, k)` runs before step k.  The divide
    source is asked after every step."""
    base, R, make = MESH[name]
    with div_pow2(on):
        g, f = gpu_grid(base, R)
        g.set_geometry((0, 0, 0), l0)
        make(g, f)
        if mask is not None:
            set_velocities(g, f, mask)
        dt = g.advection_max_time_step(f)
        if special:
            set_special(g, f, special)
        out, src, seen = [], [], []
        for k in range(steps):
            if edit is not None:
                seen.append(edit(g, f, k))
            g.advection_step(f, 0.5 * dt)
            g.advection_commit(f[0])
            out.append(bits(f[0].get(0, g.n_local)))
            src.append(g.advection_divide_source(f))
        res = dict(out=out, src=src, seen=seen, lay=g.advection_layout(), len_src=g.advection_length_source(f),
                   vel_src=g.advection_velocity_source(f))
        g.close()
    return res


@functools.lru_cache(maxsize=None)
def pair(name, mask, special=()):
    """The multiplying run and the forced-off run, computed once and shared
    (read only)."""
    a, b = run(name, L0[name], mask, True, special=special), run(name, L0[name], mask, False, special=special)
    assert a["len_src"] == 1 and b["len_src"] == 1
    assert a["src"][-1] == 1, a["src"]
    assert all(s == 0 for s in b["src"]), b["src"]
    assert a["vel_src"] == b["vel_src"]
    return a, b


def assert_bitwise(a, b):
    assert len(a["out"]) == len(b["out"])
    for k, (x, y) in enumerate(zip(a["out"], b["out"])):
        assert np.array_equal(x, y), ("density bits differ from the dividing run's at step", k, int((x != y).sum()))
    assert not np.array_equal(a["out"][0], a["out"][-1])  # the sweeps moved something


def assert_tiles(name, lay):
    general = lay["tiles"] - lay["regular_tiles"]
    if name == "prerefined":
        assert lay["regular_tiles"] > 0 and general > 0 and lay["finer_faces"] > 0, lay
    elif name == "nested":
        assert general >= 1 and lay["finer_faces"] > 0, lay
    elif name == "ext1024":
        assert lay["ext_max"] == 1024 and lay["finer_faces"] > 0, lay
    elif name == "one_tile":
        assert lay["tiles"] == lay["regular_tiles"] == 1, lay
    else:
        assert name == "all_regular" and lay["tiles"] == lay["regular_tiles"] > 1, lay


@pytest.mark.parametrize("mask", [0, 4, 7])
def test_masks_on_regular_and_general_tiles(gpu, mask):
    a, b = pair("prerefined", mask)
    assert_tiles("prerefined", a["lay"])
    assert a["vel_src"] == mask
    assert_bitwise(a, b)
    # the byte counts do not depend on the divide source
    for key in ("bytes_needed", "alg_bytes", "alg_bytes_core"):
        assert a["lay"][key] == b["lay"][key], key


@pytest.mark.parametrize("name", ["nested", "ext1024", "one_tile", "all_regular"])
def test_other_meshes(gpu, name):
    """Three levels in one tile with cross-level and same-level faces in one
    wave; ext cells loaded at staging; periodic x and y with missing z faces;
    no general tile.  Velocities as initialized (vz = 0: mask 4)."""
    a, b = pair(name, None)
    assert_tiles(name, a["lay"])
    assert a["vel_src"] == 4
    assert_bitwise(a, b)


@pytest.mark.parametrize("l0", [(1 / 32, 0.97 / 32, 1 / 8), l0_of((32, 32, 8))], ids=["one_axis", "no_axis"])
def test_an_axis_that_is_no_power_of_two_divides_everywhere(gpu, l0):
    a, b = run("prerefined", l0, None, True), run("prerefined", l0, None, False)
    assert a["src"] == [0] * STEPS and b["src"] == [0] * STEPS
    assert a["len_src"] == 1 and b["len_src"] == 1
    assert_tiles("prerefined", a["lay"])
    assert_bitwise(a, b)


@pytest.mark.parametrize("name,fields,mask", [("nested", (0, 1, 2), 4), ("prerefined", (0, 1, 2, 3), 0)])
def test_special_values(gpu, name, fields, mask):
    """+-inf, NaN payloads, +-0, subnormals and 1e-300-scale values in the
    density and the velocities, beside level jumps and elsewhere."""
    a, b = pair(name, None, fields)
    assert_tiles(name, a["lay"])
    assert a["vel_src"] == mask
    last = a["out"][-1].view(np.float64)
    assert np.isnan(last).any() and np.isfinite(last).any()
    assert_bitwise(a, b)
    c, _ = pair(name, None)
    assert not np.array_equal(a["out"][-1], c["out"][-1])  # the values reached the densities


def test_an_edited_length_divides_and_returns(gpu):
    """One local slot of ly rewritten between steps: the length table falls
    back, so the divide source is 0 and the result the dividing run's; with
    the old value back the sweeps multiply again."""
    def edit(g, f, k):
        if k == 2:
            v = f[5].get()
            edit.old = v.copy()
            v[int(np.argmax(f[0].get(0, g.n_local)))] *= 1.5  # the cell at the top of the hump
            f[5].set(v)
            return g.advection_divide_source(f), g.advection_length_source(f)
        if k == 4:
            f[5].set(edit.old)
            return g.advection_divide_source(f), g.advection_length_source(f)
        return (g.advection_divide_source(f), g.advection_length_source(f)) if k == 1 else None

    a = run("fb", L0["fb"], None, True, 6, edit)
    assert a["seen"][1] == (1, 1) and a["seen"][2] == (0, 0) and a["seen"][4] == (1, 1), a["seen"]
    assert a["src"] == [1, 1, 0, 0, 1, 1], a["src"]
    b = run("fb", L0["fb"], None, False, 6, edit)
    assert b["src"] == [0] * 6 and b["seen"][2] == (0, 0) and b["seen"][4] == (0, 1), (b["src"], b["seen"])
    c = run("fb", L0["fb"], None, True, 6)
    assert c["src"] == [1] * 6
    assert_bitwise(a, b)
    assert not np.array_equal(a["out"][3], c["out"][3])  # the edit mattered


@pytest.mark.parametrize("exp,expect", [(-300, 1), (-330, 0), (340, 1), (341, 0)])
def test_verdict_needs_normal_reciprocals_at_every_level(gpu, exp, expect):
    """Powers of two whose volume (2^-1083 at level 31 of 2^-330) or its
    reciprocal (2^-1023 of 2^341 at level 0) is no normal double keep the
    division; the length table is used either way.  No sweep is made."""
    base, R, make = MESH["one_tile"]
    g, f = gpu_grid(base, R)
    g.set_geometry((0, 0, 0), (2.0 ** exp,) * 3)
    make(g, f)
    assert g.advection_length_source(f) == 1
    assert g.advection_divide_source(f) == expect
    g.close()
