"""The length-table tile sweeps without length rows in LDS: the regular
kernel takes every length a face reads from the tile's own level, the
general kernel from a level byte per LDS column, and both size their
persistent grids by the blocks per CU the runtime reports.

Every comparison is bitwise (np.array_equal) against the same sweep reading
the length fields (DCCRGX_LEN_TABLE=0), over 4 steps, with the distinct
non-power-of-two level-0 lengths of test_gpu_advection_lengths.py: a wrong
level or a swapped axis changes bits.  The shapes of that file ((32, 32, 8)
R = 2; (16, 16, 16) R = 1 unrefined) already run the new kernels; this file
adds what they leave out: three levels in one tile, a regular tile between
general ones, tiles with more than 512 out-of-tile neighbors (the ones the
general kernel loads at staging), fewer tiles than blocks, and the
blocks-per-CU witness.

The meshes with more than 512 out-of-tile neighbors are made by hand
(HALF_REFINED): an unrefined 8^3 box of level-0 cells whose x sides
(640 neighbors) or x and y sides (1024, the kernel's capacity, whose LDS
leaves two blocks per CU) face refined cells."""
import functools
import os
import sys

import numpy as np
import pytest

from test_gpu_advection_lengths import NAMES, gpu_grid, len_table, prerefine

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import tile_stats  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS = 4


def level0_ids(base, box):
    """Ids of the level-0 cells with indices in box = ((x0, x1), (y0, y1), (z0, z1))."""
    (x0, x1), (y0, y1), (z0, z1) = box
    return [1 + x + base[0] * (y + base[1] * z) for z in range(z0, z1) for y in range(y0, y1) for x in range(x0, x1)]


def nested(g, f):
    """Base (8, 8, 4), R = 3: a 4 x 4 x 2 block of cells refined at every
    level, each inside the one before (levels 0..3 all exist, a coarser and a
    finer neighbor for the cells of levels 1 and 2)."""
    for lvl in range(3):
        lo = 2 * ((2 << lvl) - 1), (2 << lvl) - 1  # the block's first cell in level-lvl cells: x and y, z
        unit = 8 >> lvl  # a level-lvl cell in finest cells
        for z in range(lo[1], lo[1] + 2):
            for y in range(lo[0], lo[0] + 4):
                for x in range(lo[0], lo[0] + 4):
                    g.refine_completely(g.get_cell_from_indices((x * unit, y * unit, z * unit), lvl))
        g.stop_refining()
    g.advection_initialize(f)


def half_refined(both, g, f):
    """Base (16, 16, 8), R = 1: the level-0 box [0, 8)^3 stays, the box beyond
    its x sides (periodic: one box) is refined, with `both` the one beyond
    its y sides too."""
    for c in level0_ids((16, 16, 8), ((8, 16), (0, 8), (0, 8))):
        g.refine_completely(c)
    if both:
        for c in level0_ids((16, 16, 8), ((0, 8), (8, 16), (0, 8))):
            g.refine_completely(c)
    g.stop_refining()
    g.advection_initialize(f)


def unrefined(g, f):
    g.advection_initialize(f)


MESHES = {
    "nested": ((8, 8, 4), 3, nested),
    "prerefined": ((32, 32, 8), 2, lambda g, f: prerefine(g, f, 2)),
    "ext640": ((16, 16, 8), 1, functools.partial(half_refined, False)),
    "ext1024": ((16, 16, 8), 1, functools.partial(half_refined, True)),
    "one_tile": ((8, 8, 8), 1, unrefined),
    "four_tiles": ((16, 16, 8), 1, unrefined),
}


def sweep(name, on):
    base, R, make = MESHES[name]
    with len_table(on):
        g, f = gpu_grid(base, R)
        make(g, f)
        dt = g.advection_max_time_step(f)
        out = []
        for _ in range(STEPS):
            g.advection_step(f, 0.5 * dt)
            g.advection_commit(f[0])
            out.append(f[0].get(0, g.n_local))
        res = dict(out=out, src=g.advection_length_source(f), lay=g.advection_layout(), occ=g.advection_occupancy(),
                   ids=g.slot_ids()[: g.n_local], base=base, R=R)
        g.close()
    return res


@functools.lru_cache(maxsize=None)
def pair(name):
    """The table run and the field-reading run of a mesh, computed once and
    shared (read only)."""
    a, b = sweep(name, True), sweep(name, False)
    assert a["src"] == 1 and b["src"] == 0
    assert np.array_equal(a["ids"], b["ids"])
    return a, b


def assert_bitwise(name):
    a, b = pair(name)
    for x, y in zip(a["out"], b["out"]):
        assert np.array_equal(x, y)
    assert not np.array_equal(a["out"][0], a["out"][-1])  # the sweeps moved something
    return a


def tiles_of(a):
    """The CPU restatement of the tile cut and classification (scripts/tile_stats.py)."""
    L = tile_stats.layout(a["ids"], a["base"], a["R"])
    assert L["starts"].size - 1 == a["lay"]["tiles"]
    return L, tile_stats.classify(L, a["base"], a["R"])


def test_three_levels_in_one_general_tile(gpu):
    a = assert_bitwise("nested")
    lay = a["lay"]
    L, reason = tiles_of(a)
    assert set(np.unique(L["lvl"])) == {0, 1, 2, 3}
    st = L["starts"]
    per_tile = [np.unique(L["lvl"][st[t]:st[t + 1]]).size for t in range(st.size - 1)]
    assert np.all(np.diff(st) <= 512) and max(per_tile) >= 3, per_tile
    assert lay["finer_faces"] > 0 and lay["tiles"] - lay["regular_tiles"] >= 1, lay


def test_regular_tile_between_general_tiles(gpu):
    a = assert_bitwise("prerefined")
    lay = a["lay"]
    L, reason = tiles_of(a)
    assert int((reason == 1).sum()) == lay["regular_tiles"] > 0, lay
    assert lay["tiles"] - lay["regular_tiles"] > 0 and lay["finer_faces"] > 0, lay
    # a regular tile one of whose neighbor boxes lies in a general tile
    base, R = a["base"], a["R"]
    glen = np.array(base, np.int64) << R
    where = {(int(lv), int(x), int(y), int(z)): s for s, (lv, (x, y, z)) in enumerate(zip(L["lvl"], L["ind"]))}
    st = L["starts"]
    found = 0
    for t in np.nonzero(reason == 1)[0]:
        lv, ln, c = int(L["lvl"][st[t]]), int(L["clen"][st[t]]), L["ind"][st[t]]
        for d in range(6):
            nb = c.copy()
            nb[d >> 1] += 8 * ln if d & 1 else -8 * ln
            if d >> 1 < 2:
                nb[d >> 1] %= glen[d >> 1]  # periodic in x and y
            s0 = where.get((lv, int(nb[0]), int(nb[1]), int(nb[2])), -1)
            if s0 >= 0 and reason[np.searchsorted(st, s0, side="right") - 1] != 1:
                found += 1
    assert found > 0


@pytest.mark.parametrize("name,ext_max,blocks", [("ext640", 640, 3), ("ext1024", 1024, 2)])
def test_more_than_512_out_of_tile_neighbors(gpu, name, ext_max, blocks):
    a = assert_bitwise(name)
    assert a["lay"]["ext_max"] == ext_max > 512, a["lay"]
    assert a["lay"]["finer_faces"] > 0
    # the LDS of ext_max columns decides the blocks per CU: fewer at the
    # capacity, never more than the kernel is compiled for, and still right
    occ = a["occ"]["general"]
    assert 2 <= occ["blocks_per_cu"] <= blocks and occ["blocks_per_cu"] == occ["blocks_per_cu_query"], a["occ"]


@pytest.mark.parametrize("name,tiles", [("one_tile", 1), ("four_tiles", 4)])
def test_fewer_tiles_than_blocks(gpu, name, tiles):
    a = assert_bitwise(name)
    assert a["lay"]["tiles"] == a["lay"]["regular_tiles"] == tiles, a["lay"]


def test_layout_reports_blocks_per_cu(gpu):
    a, b = pair("nested")
    lay, occ = a["lay"], a["occ"]
    assert lay["regular_blocks_per_cu"] == occ["regular"]["blocks_per_cu"]
    assert lay["general_blocks_per_cu"] == occ["general"]["blocks_per_cu"]
    for kind in ("regular", "general"):
        # what was launched is what the runtime reports for that kernel and LDS size
        assert occ[kind]["blocks_per_cu"] == occ[kind]["blocks_per_cu_query"] >= 2, occ
    assert occ["general"]["lds_bytes"] > 0
    # the field-reading kernels keep their two blocks per CU
    assert b["occ"]["regular"]["blocks_per_cu"] == 2 and b["occ"]["general"]["blocks_per_cu"] == 2, b["occ"]
