"""Stretched_Cartesian_Geometry in plain Python (a helper, not a test).

A literal restatement of the reference's loops
(dccrg_stretched_cartesian_geometry.hpp: get_length 298-337, get_center
346-403, get_min / get_max 417-455, get_real_coordinate 504-548, get_indices
557-607, linear scans included) on Python floats, which are IEEE doubles: one
rounded operation per Python operation, in the reference's operand order, so a
device result can be compared bitwise.

One deliberate difference, the facade's host get_indices
(include/dccrg_stretched_cartesian_geometry.hpp:159-176): a coordinate exactly
at a dimension's first boundary belongs to the first cell, where the
reference's scan steps below index 0.  ``facade_rule=False`` gives the
reference's own loop and raises there.

``StretchedParticleModel`` is tests/particles_model.py's model with this
geometry; the cases, point sets and the golden file's codec used by
tests/test_stretched_ref_cpu.py and tests/test_gpu_stretched.py live here too.
"""
import base64
import math
import zlib

import numpy as np

from particles_model import ParticleModel

ERROR_INDEX = 0xFFFFFFFFFFFFFFFF
NAN = float("nan")


# ---- the reference's functions, one dimension at a time ----------------------
def real_coordinate_1d(c, periodic, x):
    """get_real_coordinate 517-545."""
    start, end = c[0], c[-1]
    if x >= start and x <= end:
        return x
    if not periodic or x != x:
        # (the reference wraps a NaN in a periodic dimension with operations
        # that all give NaN)
        return NAN
    grid_length = end - start
    if x < start:
        distance = start - x
        return x + grid_length * float(math.ceil(distance / grid_length))
    distance = x - end
    return x - grid_length * float(math.ceil(distance / grid_length))


def indices_1d(c, R, x, facade_rule=True):
    """get_indices 573-603: error_index outside [c[0], c[-1]]."""
    if not (x >= c[0] and x <= c[-1]):
        return ERROR_INDEX
    level_0_length_in_indices = 1 << R
    coord_start_index = 0
    while c[coord_start_index] < x:
        coord_start_index += 1
    if coord_start_index == 0:
        if not facade_rule:
            raise IndexError("the reference's scan steps below index 0 at the first coordinate")
    else:
        coord_start_index -= 1
    length_of_index = (c[coord_start_index + 1] - c[coord_start_index]) / float(level_0_length_in_indices)
    index_offset = 0
    while c[coord_start_index] + float(index_offset) * length_of_index < x:
        index_offset += 1
    if index_offset > 0:  # (at x == c[0] under the facade's rule the loop never runs)
        index_offset -= 1
    return coord_start_index * level_0_length_in_indices + index_offset


def length_1d(c, R, level, index):
    """get_length 317-334."""
    coord_start_index = index // (1 << R)
    return (c[coord_start_index + 1] - c[coord_start_index]) / float(1 << level)


def center_1d(c, R, level, index):
    """get_center 366-400."""
    level_0_length_in_indices = 1 << R
    coord_start_index = index // level_0_length_in_indices
    length_of_index = (c[coord_start_index + 1] - c[coord_start_index]) / float(level_0_length_in_indices)
    cell_length = length_1d(c, R, level, index)
    return (c[coord_start_index]
            + length_of_index * float(index - coord_start_index * level_0_length_in_indices)
            + cell_length / 2)


def cell_geometry(coords, R, levels, indices):
    """dict(length, center, min, max), each (n, 3), of cells given by their
    refinement levels and indices (NaN where the level is negative)."""
    cs = [[float(v) for v in c] for c in coords]
    n = len(levels)
    out = {k: np.full((n, 3), np.nan) for k in ("length", "center", "min", "max")}
    for i in range(n):
        lvl = int(levels[i])
        if lvl < 0:
            continue
        for d in range(3):
            L = length_1d(cs[d], R, lvl, int(indices[i][d]))
            ctr = center_1d(cs[d], R, lvl, int(indices[i][d]))
            out["length"][i, d] = L
            out["center"][i, d] = ctr
            out["min"][i, d] = ctr - L / 2
            out["max"][i, d] = ctr + L / 2
    return out


def real_coordinates(coords, periodic, pts):
    cs = [[float(v) for v in c] for c in coords]
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.empty(pts.shape)
    for i in range(pts.shape[0]):
        for d in range(3):
            out[i, d] = real_coordinate_1d(cs[d], bool(periodic[d]), float(pts[i, d]))
    return out


def indices_of(coords, R, pts, facade_rule=True):
    cs = [[float(v) for v in c] for c in coords]
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.empty(pts.shape, np.uint64)
    for i in range(pts.shape[0]):
        for d in range(3):
            out[i, d] = indices_1d(cs[d], R, float(pts[i, d]), facade_rule)
    return out


def geometry_block(coords):
    """Stretched_Cartesian_Geometry::write 652-715: int id 2, three uint64
    counts, the coordinates."""
    cs = [np.asarray(c, np.float64) for c in coords]
    return (np.int32(2).tobytes() + np.array([c.size for c in cs], np.uint64).tobytes()
            + b"".join(c.tobytes() for c in cs))


# ---- the model ----------------------------------------------------------------
class StretchedParticleModel(ParticleModel):
    def __init__(self, o, coords, K=3):
        self.coords = [np.asarray(c, np.float64).copy() for c in coords]
        start = [c[0] for c in self.coords]
        super().__init__(o, start, [c[1] - c[0] for c in self.coords], K)
        self.end = np.array([c[-1] for c in self.coords])  # get_end 279
        self.cell_len = None  # no single finest cell length
        self.smallest = np.array([np.diff(c).min() for c in self.coords]) / np.float64(1 << self.R)

    def real_coordinate(self, x):
        return real_coordinates(self.coords, self.periodic, x)

    def locate(self, x):
        """get_existing_cell(coordinate), dccrg.hpp:6316-6336: the indices of
        the real coordinate, error_cell when one is error_index (or past the
        grid: the rounding quirk at the last cell's upper boundary), then the
        smallest leaf at them."""
        c = self.real_coordinate(x)
        ind = indices_of(self.coords, self.R, c)
        ok = np.all(ind < self.glen, axis=1)
        out = np.zeros(c.shape[0], np.uint64)
        todo = np.flatnonzero(ok)
        for lvl in range(self.R, -1, -1):
            if todo.size == 0:
                break
            ids = self.o.mapping.from_indices(ind[todo], np.full(todo.size, lvl, np.int32))
            k = np.searchsorted(self.leaves, ids)
            hit = (k < self.leaves.size) & (self.leaves[np.minimum(k, self.leaves.size - 1)] == ids) & (ids != 0)
            out[todo[hit]] = ids[hit]
            todo = todo[~hit]
        return out

    def geometry(self, ids):
        """(centers, lengths) of cells, as Dccrg.geometry."""
        b = self.o.mapping.batch(ids)
        g = cell_geometry(self.coords, self.R, b["level"], b["indices"])
        return g["center"], g["length"]


# ---- cases, point sets, the golden file ------------------------------------------
LENGTH = (4, 3, 2)
PERIODIC = (True, False, True)


def case_coords(name):
    """'exact': boundaries that are sums of powers of two, R = 2.  'rounded':
    cumulative sums of 0.1, 0.3 and 0.7, R = 3: neither the boundaries nor
    c0 + k * li are representable, and the starts are chosen so that in x's
    second cell and in z's last cell c0 + 2^R li < c1 (the reference's
    rounding quirk: the upper boundary indexes the next level-0 cell)."""
    if name == "exact":
        return 2, [np.array([0.0, 0.5, 1.5, 3.0, 5.0]), np.array([0.0, 1.0, 2.0, 4.0]), np.array([0.0, 1.0, 2.0])]
    assert name == "rounded"
    steps = np.array([0.1, 0.3, 0.7, 0.1, 0.3, 0.7])
    return 3, [np.concatenate([[-0.7], -0.7 + np.cumsum(steps[1:5])]),
               np.concatenate([[0.3], 0.3 + np.cumsum(steps[1:4])]),
               np.concatenate([[-0.6], -0.6 + np.cumsum(steps[1:3])])]


CASES = ("exact", "rounded")


def special_values(c, R):
    """One dimension's telling coordinates: every level-0 boundary, every
    finest sub-boundary formed as c[i0] + k * li, each of those one ulp below
    and above, the grid's start and end, 1 and 2.5 grid lengths outside on
    both sides, NaN."""
    c = np.asarray(c, np.float64)
    v = list(c)
    l0 = np.float64(1 << R)
    for i0 in range(c.size - 1):
        li = (c[i0 + 1] - c[i0]) / l0
        v += [c[i0] + np.float64(k) * li for k in range(int(l0) + 1)]
    v = np.array(v)
    v = np.concatenate([v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)])
    L = c[-1] - c[0]
    out = np.concatenate([v, [c[0], c[-1], c[0] - L, c[0] - 2.5 * L, c[-1] + L, c[-1] + 2.5 * L, np.nan]])
    return out


def point_set(coords, R, seed=0, n_random=2000):
    """(n, 3) points: every special value of each dimension with the other
    two coordinates random inside the grid, then n_random points over 1.2
    times the grid's extent."""
    rng = np.random.default_rng(seed)
    lo = np.array([c[0] for c in coords])
    hi = np.array([c[-1] for c in coords])
    blocks = []
    for d in range(3):
        v = special_values(coords[d], R)
        p = lo + (hi - lo) * rng.random((v.size, 3))
        p[:, d] = v
        blocks.append(p)
    blocks.append(lo + (hi - lo) * (rng.random((n_random, 3)) * 1.2 - 0.1))
    # all three special at once: corners and boundary crossings
    m = min(special_values(coords[d], R).size for d in range(3))
    blocks.append(np.stack([special_values(coords[d], R)[:m] for d in range(3)], axis=1))
    return np.concatenate(blocks)


def at_first_coordinate(coords, pts):
    """The points the reference's get_indices cannot take: a coordinate
    exactly at its dimension's first boundary."""
    first = np.array([c[0] for c in coords])
    return np.any(pts == first, axis=1)


def enc(a):
    """An array as text: base64 of the deflated little-endian bytes."""
    a = np.ascontiguousarray(a)
    return dict(dtype=a.dtype.str, shape=list(a.shape),
                z=base64.b64encode(zlib.compress(a.tobytes(), 9)).decode())


def dec(d):
    return np.frombuffer(zlib.decompress(base64.b64decode(d["z"])), np.dtype(d["dtype"])).reshape(d["shape"]).copy()


# The golden file keeps the reference's answers without repeating what
# repeats: a cell's length, center, min and max along a dimension depend on
# its level and its index along that dimension only, so there is one row per
# (dimension, level, index); get_real_coordinate is kept where it is not the
# given coordinate bit for bit.  pack() checks that unpack() gives back every
# value the reference printed.
CELL_KEYS = ("length", "center", "min", "max")


def _cell_rows(R):
    """Every possible cell's table row per dimension, and the row count."""
    from oracle import oracle as O

    mp = O.Mapping(LENGTH, R)
    b = mp.batch(np.arange(1, mp.last_cell + 1, dtype=np.uint64))
    lvl, ind = b["level"].astype(np.int64), b["indices"].astype(np.int64)
    rows, at = np.empty(ind.shape, np.int64), 0
    for d in range(3):
        first = at + LENGTH[d] * ((1 << lvl) - 1)  # the levels below take length * (2^level - 1) rows
        rows[:, d] = first + (ind[:, d] >> (R - lvl))
        at += LENGTH[d] * ((2 << R) - 1)
    return rows, at


def unpack(R, pts, packed):
    """The reference's answers in full: CELL_KEYS (cells, 3) by id - 1, real
    and indices (points, 3), block."""
    rows, _ = _cell_rows(R)
    table = dec(packed["cells"])
    out = {k: table[rows, i] for i, k in enumerate(CELL_KEYS)}
    real = np.array(pts, np.float64).reshape(-1)
    real[dec(packed["real_at"])] = dec(packed["real"])
    out.update(real=real.reshape(-1, 3), indices=dec(packed["indices"]), block=dec(packed["block"]))
    return out


def pack(R, pts, full):
    rows, n = _cell_rows(R)
    table = np.full((n, 4), np.nan)
    for i, k in enumerate(CELL_KEYS):
        table[rows, i] = full[k]
    flat, real = np.asarray(pts, np.float64).reshape(-1), full["real"].reshape(-1)
    at = np.flatnonzero(flat.view(np.uint64) != real.view(np.uint64)).astype(np.uint32)
    packed = dict(cells=enc(table), real_at=enc(at), real=enc(real[at]), indices=enc(full["indices"]),
                  block=enc(full["block"]))
    back = unpack(R, pts, packed)
    assert all(same_bits(back[k], full[k]) for k in full), "the reference's answers do not unpack"
    return packed


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        # (any NaN equals any NaN: the payload of a quiet NaN is not specified)
        an, bn = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(an, bn) and np.array_equal(a[~an].view(np.uint64), b[~bn].view(np.uint64)))
    return bool(np.array_equal(a, b))
