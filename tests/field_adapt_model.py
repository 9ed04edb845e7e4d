"""Fixed fp64 cell fields following the mesh through stop_refining
(dccrgx_field_follow_mesh, include/dccrgx.h), NumPy only (a helper, not a
test), in the manner of particles_adapt_model.remesh.

It knows nothing of the library: the old and the new leaves come from the
oracle grid (or any two id lists), the face neighbors of the old mesh from
advection_model.faces, the derivative D and the lengths from the caller (the
product's own gradient(scale=1) output, or gradient_model's).  The header's
contract is restated in fp64, one rounded operation per Python operation.

follow(...) returns the new values aligned with the new leaves and, for the
LINEAR mode, what the limiter saw per refined parent.

Modes: None / "off", "mean", "sum", "linear".
"""
import numpy as np

import advection_model as AM


def _first(base, R):
    n0 = int(np.prod(np.asarray(base, np.int64)))
    return 1 + np.cumsum([0] + [n0 * 8 ** l for l in range(R + 2)])


def cell_id(base, R, lvl, lo):
    """The id of the cell of level lvl whose first corner is lo (finest cells)."""
    size = 1 << (R - lvl)
    ix, iy, iz = (int(lo[d]) // size for d in range(3))
    nx, ny = int(base[0]) << lvl, int(base[1]) << lvl
    return int(_first(base, R)[lvl]) + ix + iy * nx + iz * nx * ny


def parent_of(base, R, lvl, lo):
    size = 2 << (R - lvl)
    return cell_id(base, R, lvl - 1, [int(x) // size * size for x in lo])


def children_of(base, R, lvl, lo):
    """The eight children in ascending id: bit d of k is the upper half along d."""
    h = 1 << (R - lvl - 1)
    return [cell_id(base, R, lvl + 1, [int(lo[d]) + ((k >> d) & 1) * h for d in range(3)]) for k in range(8)]


class Follow:
    """What follow() returns: values (aligned with new_ids); kind (0 stayed,
    1 new child, 2 merged parent); for "linear" per refined parent id the
    dict limiter[id] = (v, m, M, delta, alpha, (t0, t1, t2))."""


def follow(old_ids, new_ids, base, R, periodic, lengths, values, D, mode):
    """old_ids sorted ascending with values (n,), lengths (n, 3) and D (n, 3)
    aligned (D and lengths are read at the refined parents only, and only
    under "linear": they may be None otherwise)."""
    old_ids = np.asarray(old_ids, np.uint64)
    new_ids = np.asarray(new_ids, np.uint64)
    assert np.all(np.diff(old_ids.astype(np.int64)) > 0)
    val = [float(x) for x in np.asarray(values, np.float64)]
    pos = {int(c): i for i, c in enumerate(old_ids)}
    lvl, lo, _ = AM.boxes(new_ids, base, R)
    out = Follow()
    out.values = np.zeros(new_ids.size)
    out.kind = np.zeros(new_ids.size, np.int64)
    out.limiter = {}
    nbs = None
    if mode == "linear":
        nbs = [[] for _ in range(old_ids.size)]
        for c, _, nb in AM.faces(old_ids, base, R, periodic):
            nbs[int(c)].append(int(nb))

    def slopes(p):
        """The limited half-differences of the old cell at position p."""
        pid = int(old_ids[p])
        if pid in out.limiter:
            return out.limiter[pid][5]
        v = val[p]
        e = []
        for d in range(3):
            q = float(lengths[p][d]) * 0.25
            e.append(float(D[p][d]) * q)
        delta = (abs(e[0]) + abs(e[1])) + abs(e[2])
        m = min([v] + [val[k] for k in nbs[p]])
        M = max([v] + [val[k] for k in nbs[p]])
        alpha = 1.0
        if delta > 0:
            up = (M - v) / delta
            dn = (v - m) / delta
            alpha = min(1.0, min(up, dn))
        t = tuple(alpha * x for x in e)
        out.limiter[pid] = (v, m, M, delta, alpha, t)
        return t

    for i, c in enumerate(int(x) for x in new_ids):
        if c in pos:
            out.values[i] = val[pos[c]]
            continue
        l = int(lvl[i])
        par = parent_of(base, R, l, lo[i]) if l > 0 else None
        if par is not None and par in pos:
            # a new child of a refined parent
            out.kind[i] = 1
            v = val[pos[par]]
            if mode in (None, "off", "mean"):
                out.values[i] = v
            elif mode == "sum":
                out.values[i] = v * 0.125
            else:
                assert mode == "linear", mode
                t = slopes(pos[par])
                h = 1 << (R - l)
                for d in range(3):
                    s = 1.0 if (int(lo[i][d]) // h) & 1 else -1.0
                    v = v + s * t[d]
                out.values[i] = v
            continue
        # the parent of a merged family: its eight children in ascending id
        out.kind[i] = 2
        ch = children_of(base, R, l, lo[i])
        assert all(k in pos for k in ch), (c, ch)
        assert ch == sorted(ch)
        acc = 0.0
        if mode in (None, "off"):
            pass  # default-constructed
        elif mode == "sum":
            for k in ch:
                acc = acc + val[pos[k]]
        else:
            for k in ch:
                acc = acc + val[pos[k]] / 8.0
        out.values[i] = acc
    return out
