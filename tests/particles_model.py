"""The particle step in plain Python over the oracle (a helper, not a test).

One global address space: every leaf of ``oracle.Grid`` owns a list of
particle records (K doubles, 0..2 the position); a step visits the cells in
ascending id, exactly as ``Dccrg.particles_step`` is specified:

- ``x' = real_coordinate(x + v dt)`` (two separately rounded operations),
  stored back;
- the particle stays when the smallest leaf at ``x'`` is its cell, is appended
  to that leaf when it is in ``neighbors_of`` of its cell, and is lost otherwise;
- a cell ends with its stayers in their previous order, then the arrivals
  ordered by (source cell id, index in the source cell).

The arithmetic restates Cartesian_Geometry::get_real_coordinate, get_indices
(dccrg_cartesian_geometry.hpp:521-607) and Dccrg::get_existing_cell
(dccrg.hpp:6316-6336, 11275-11308) with numpy float64 operations, one IEEE
operation per numpy call, so a device result can be compared bitwise.
"""
import numpy as np


class ParticleModel:
    def __init__(self, o, start=(0.0, 0.0, 0.0), l0=(1.0, 1.0, 1.0), K=3):
        self.o = o
        self.K = int(K)
        self.start = np.asarray(start, np.float64)
        self.l0 = np.asarray(l0, np.float64)
        o.set_geometry(self.start, self.l0)
        self.R = o.R
        self.periodic = np.asarray(o.periodic, bool)
        length = np.asarray(o.length, np.uint64)
        self.end = self.start + length.astype(np.float64) * self.l0  # get_end
        self.cell_len = self.l0 / np.float64(1 << self.R)
        self.glen = length << np.uint64(self.R)
        self.leaves = np.sort(o.cells()[0])
        self.cells = {int(c): np.zeros((0, self.K)) for c in self.leaves}
        self._nof = {}

    # ---- geometry ---------------------------------------------------------
    def real_coordinate(self, x):
        """get_real_coordinate of (n, 3) coordinates."""
        x = np.asarray(x, np.float64).reshape(-1, 3)
        out = np.full(x.shape, np.nan)
        for d in range(3):
            c, s, e = x[:, d], self.start[d], self.end[d]
            inside = (c >= s) & (c <= e)
            r = np.full(c.shape, np.nan)
            r[inside] = c[inside]
            if self.periodic[d]:
                L = e - s
                lo = ~inside & (c < s)
                hi = ~inside & ~lo  # (a NaN stays one: every operation on it gives NaN)
                with np.errstate(invalid="ignore"):
                    dist = s - c[lo]
                    r[lo] = c[lo] + L * np.ceil(dist / L)
                    dist = c[hi] - e
                    r[hi] = c[hi] - L * np.ceil(dist / L)
            out[:, d] = r
        return out

    def locate(self, x):
        """get_existing_cell(coordinate) of (n, 3) coordinates: the smallest
        leaf there, 0 (error_cell) otherwise."""
        c = self.real_coordinate(x)
        n = c.shape[0]
        ok = np.ones(n, bool)
        ind = np.zeros((n, 3), np.uint64)
        for d in range(3):
            with np.errstate(invalid="ignore"):
                inside = (c[:, d] >= self.start[d]) & (c[:, d] <= self.end[d])
            q = np.floor((c[inside, d] - self.start[d]) / self.cell_len[d])
            ind[inside, d] = q.astype(np.uint64)
            ok &= inside
            ok &= ind[:, d] < self.glen[d]  # the grid's end indexes one past the last cell
        out = np.zeros(n, np.uint64)
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

    def neighbors_of(self, cell):
        s = self._nof.get(cell)
        if s is None:
            s = self._nof[cell] = set(int(i) for i in self.o.neighbors_of(cell)[0])
        return s

    # ---- particles ----------------------------------------------------------
    def set(self, cell, records):
        self.cells[int(cell)] = np.ascontiguousarray(records, np.float64).reshape(-1, self.K).copy()

    def total(self):
        return sum(a.shape[0] for a in self.cells.values())

    def step(self, velocity=None, dt=1.0):
        """Returns dict(stayed, moved, lost, lost_known): lost_known counts the
        lost particles whose destination exists (not a neighbor)."""
        ids = [c for c in sorted(self.cells) if self.cells[c].shape[0]]
        stats = dict(stayed=0, moved=0, lost=0, lost_known=0)
        if not ids:
            return stats
        rec = np.concatenate([self.cells[c] for c in ids])
        cnt = np.array([self.cells[c].shape[0] for c in ids])
        src = np.repeat(np.array(ids, np.uint64), cnt)
        v = rec[:, 3:6] if velocity is None else np.asarray(velocity, np.float64)[None, :]
        step = v * np.float64(dt)
        rec[:, 0:3] = self.real_coordinate(rec[:, 0:3] + step)
        dst = self.locate(rec[:, 0:3])
        stay = dst == src
        new = {}
        first = np.concatenate([[0], np.cumsum(cnt)])
        for k, c in enumerate(ids):
            sl = slice(first[k], first[k + 1])
            new[c] = [rec[sl][stay[sl]]]
        stats["stayed"] = int(stay.sum())
        # movers in (source id, index) order: rec is already in that order
        for p in np.flatnonzero(~stay):
            s, d = int(src[p]), int(dst[p])
            if d != 0 and d in self.neighbors_of(s):
                new.setdefault(d, [np.zeros((0, self.K))]).append(rec[p:p + 1])
                stats["moved"] += 1
            else:
                stats["lost"] += 1
                stats["lost_known"] += int(d != 0)
        for c in self.cells:
            parts = new.get(c)
            self.cells[c] = np.concatenate(parts) if parts else np.zeros((0, self.K))
        return stats


def seeded_particles(ids, centers, lengths, rng, max_per_cell, K=3, vmax=None):
    """Per cell 0..max_per_cell records inside the cell: uniform positions,
    doubles 3.. uniform in [-vmax, vmax] (a velocity when K >= 6) or tags."""
    out = {}
    for c, ctr, ln in zip(ids, centers, lengths):
        n = int(rng.integers(0, max_per_cell + 1))
        r = np.zeros((n, K))
        r[:, 0:3] = (ctr - ln / 2) + ln * rng.random((n, 3))
        if K > 3:
            r[:, 3:] = rng.random((n, K - 3)) * 2 - 1
            if vmax is not None:
                r[:, 3:6] *= np.asarray(vmax)
        out[int(c)] = r
    return out
