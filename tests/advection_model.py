"""A plain model of one advection step (tests/advection/solve.hpp:44-279) on
a refined grid, NumPy only.  It knows nothing of the library and nothing of
the oracle's neighbor code: the faces come from painting the leaves into an
array of finest cells and looking one cell beyond each side, the fluxes are
summed per cell in np.longdouble.

faces(ids, base, R, periodic) -> (n_faces, 3) int64 rows
    (cell, dir 0..5 = -x,+x,-y,+y,-z,+z, neighbor), cell and neighbor as
    positions in `ids`.
step(F, cols, dt) -> the new densities (np.longdouble); cols[:, 0..6] are
    rho, vx, vy, vz, lx, ly, lz.
max_time_step(cols) -> float (the rule of solve.hpp:289-333, in fp64).
coverage(F, cols, levels) -> counts[dir, rel, sign]: rel 0 same level,
    1 the neighbor is coarser, 2 finer; sign 0 for v < 0, 1 for v >= 0.
"""
import numpy as np

LD = np.longdouble


def boxes(ids, base, R):
    """Per id its refinement level and its first corner and edge in finest
    cells (the id mapping: level l holds prod(base) * 8^l ids, x fastest)."""
    ids = np.asarray(ids, np.uint64).astype(np.int64)
    base = np.asarray(base, np.int64)
    n0 = int(np.prod(base))
    first = 1 + np.cumsum([0] + [n0 * 8 ** l for l in range(R + 1)])  # first id of each level, and one past the last
    lvl = np.searchsorted(first, ids, side="right") - 1
    assert np.all((lvl >= 0) & (lvl <= R)), "id outside the grid"
    k = ids - first[lvl]
    nx, ny = base[0] << lvl, base[1] << lvl
    ind = np.stack([k % nx, (k // nx) % ny, k // (nx * ny)], axis=1)
    size = np.int64(1) << (R - lvl)
    return lvl, ind * size[:, None], size


def centres(ids, base, R):
    """Cell centres scaled to the unit cube."""
    _, lo, size = boxes(ids, base, R)
    ext = (np.asarray(base, np.int64) << R).astype(np.float64)
    return (lo + 0.5 * size[:, None]) / ext


def paint(ids, base, R):
    """The finest-cell array of base << R holding each leaf's position in ids."""
    lvl, lo, size = boxes(ids, base, R)
    ext = tuple(int(b) << R for b in base)
    occ = np.full(ext, -1, np.int64)
    for l in np.unique(lvl):
        sel = np.nonzero(lvl == l)[0]
        s = int(size[sel[0]])
        coarse = np.full(tuple(e // s for e in ext), -1, np.int64)
        c = lo[sel] // s
        coarse[c[:, 0], c[:, 1], c[:, 2]] = sel
        fine = coarse.repeat(s, 0).repeat(s, 1).repeat(s, 2)
        assert not np.any((fine >= 0) & (occ >= 0)), "overlapping leaves"
        occ = np.where(fine >= 0, fine, occ)
    assert np.all(occ >= 0), "the leaves do not cover the grid"
    return occ, size


def faces(ids, base, R, periodic):
    occ, size = paint(ids, base, R)
    edge = size[occ]  # per finest cell the edge of its leaf
    out = []
    for axis in range(3):
        n = occ.shape[axis]
        coord = np.arange(n).reshape([n if a == axis else 1 for a in range(3)])
        for up in (0, 1):
            # finest cells on that side of their leaf (leaves are aligned to their edge)
            on_side = ((coord + 1) % edge == 0) if up else (coord % edge == 0)
            beyond = np.roll(occ, -1 if up else 1, axis)  # the layer one cell beyond
            if not periodic[axis]:
                on_side = on_side & (coord != (n - 1 if up else 0))
            pair = np.stack([occ[on_side], beyond[on_side]], axis=1)
            pair = np.unique(pair, axis=0)
            out.append(np.stack([pair[:, 0], np.full(len(pair), 2 * axis + up), pair[:, 1]], axis=1))
    F = np.concatenate(out)
    return F[np.lexsort((F[:, 2], F[:, 1], F[:, 0]))]


def _face_velocity(F, cols):
    c, d, n = F[:, 0], F[:, 1], F[:, 2]
    a = d >> 1
    la_c, la_n = cols[c, 4 + a], cols[n, 4 + a]
    va_c, va_n = cols[c, 1 + a], cols[n, 1 + a]
    return (la_c * va_n + la_n * va_c) / (la_c + la_n)


def step(F, cols, dt):
    cols = np.asarray(cols, LD)
    dt = LD(dt)
    c, d, n = F[:, 0], F[:, 1], F[:, 2]
    a = d >> 1
    b, e = (a + 1) % 3, (a + 2) % 3
    area = np.minimum(cols[c, 4 + b] * cols[c, 4 + e], cols[n, 4 + b] * cols[n, 4 + e])
    v = _face_velocity(F, cols)
    up = (d & 1) == 1  # the +side: v >= 0 carries the cell's density out
    donor = np.where((v >= 0) == up, cols[c, 0], cols[n, 0])
    flux = donor * dt * v * area
    gain = np.zeros(len(cols), LD)
    np.add.at(gain, c, np.where(up, -flux, flux))
    return cols[:, 0] + gain / (cols[:, 4] * cols[:, 5] * cols[:, 6])


def max_time_step(cols):
    cols = np.asarray(cols, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        s = cols[:, 4:7] / np.abs(cols[:, 1:4])
    normal = np.isfinite(s) & (np.abs(s) >= np.finfo(np.float64).tiny)
    return float(np.min(s[normal], initial=np.finfo(np.float64).max))


def coverage(F, cols, levels):
    levels = np.asarray(levels)
    v = _face_velocity(F, np.asarray(cols, LD))
    dl = levels[F[:, 2]] - levels[F[:, 0]]
    rel = np.where(dl == 0, 0, np.where(dl < 0, 1, 2))
    counts = np.zeros((6, 3, 2), np.int64)
    np.add.at(counts, (F[:, 1], rel, (v >= 0).astype(np.int64)), 1)
    return counts
