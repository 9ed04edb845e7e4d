"""Poisson_Solve (tests/poisson/poisson_solve.hpp) on a refined grid with a
Stretched_Cartesian_Geometry, NumPy only (a helper, not a test).

It knows nothing of the library: the faces come from
advection_model.faces (leaves painted into an array of finest cells), the
lengths and centers from stretched_model.cell_geometry (pinned to the
reference by test_stretched_ref_cpu.py).  Restated here in fp64, one rounded
operation per Python operation in the reference's operand order:

* cache(): the classification and the kept / dropped face neighbors of
  cache_system_info 836-957 and the factors of set_scaling_factor 696-819;
* solve(): initialize_solver 986-1051 and the BiCG loop of solve 251-522 over
  each cell's kept neighbors (global sums in ascending id order).

Cells are positions in the id list given; directions are 0..5 = -x, +x, -y,
+y, -z, +z and the factor columns follow them (f_x_neg, f_x_pos, ...).

poisson1d_stretched(n) is the scenario of tests/poisson/poisson1d_stretched.cpp
(:176-307) on this model: the stretched and the evenly spaced grid of n x 1 x 1
periodic cells, their 2-norms against the analytic solution.
"""
import math

import numpy as np

import advection_model as AM
import stretched_model as SM

SOLVE, BOUNDARY, SKIP = 0, 1, 2  # poisson_solve.hpp:146-150
FACTORS = ("scaling_factor", "f_x_neg", "f_x_pos", "f_y_neg", "f_y_pos", "f_z_neg", "f_z_pos")
STATE = ("solution", "best_solution", "p0", "p1", "r0", "r1", "A_dot_p0")


def geometry(coords, base, R, ids):
    """(levels, centers (n, 3), lengths (n, 3)) of cells by id."""
    lvl, lo, _ = AM.boxes(ids, base, R)
    g = SM.cell_geometry(coords, R, lvl, lo)
    return lvl, g["center"], g["length"]


def even_coords(start, l0, base):
    """The coordinates start + i * l0 of an evenly spaced grid (exact, and the
    stretched length bitwise l0 * 2^-level, when l0 is a power of two)."""
    return [np.float64(start[d]) + np.arange(base[d] + 1, dtype=np.float64) * np.float64(l0[d]) for d in range(3)]


def fallback_lengths(coords, levels):
    """What a consumer sees that takes each dimension's start and first cell
    length for an evenly spaced grid: l0 * (1 / 2^level) (Cartesian get_length)."""
    l0 = np.array([c[1] - c[0] for c in coords], np.float64)
    return l0[None, :] * (1.0 / np.float64(2.0) ** np.asarray(levels))[:, None]


class Cache:
    """What cache() returns: type (n,), f (n, 6), sf (n,), and kept, the kept
    faces as rows (cell, dir, neighbor, finer) sorted by cell, dir, neighbor."""


def cache(ids, base, R, periodic, levels, lengths, classes):
    ids = np.asarray(ids, np.uint64)
    n = ids.size
    F = AM.faces(ids, base, R, periodic)
    cls = np.asarray(classes, np.int64)
    L = np.asarray(lengths, np.float64)
    first = np.searchsorted(F[:, 0], np.arange(n + 1))
    out = Cache()
    out.type = cls.astype(np.int32).copy()
    out.f = np.zeros((n, 6))
    out.sf = np.zeros(n)
    kept_rows = []
    for c in range(n):
        t = int(cls[c])
        if t == SKIP:  # 896-898
            continue
        kept = []
        for c_, dr, nb in F[first[c]:first[c + 1]]:
            nt = int(cls[nb])
            if nt == SKIP:  # 922-924
                continue
            if t == BOUNDARY and nt == BOUNDARY:  # 926-931
                continue
            kept.append((int(dr), int(nb)))
        if not kept:  # 953-957
            out.type[c] = SKIP
            continue
        # set_scaling_factor 710-816
        ch = [float(L[c, d]) / 2.0 for d in range(3)]
        pos = [+2 * ch[d] for d in range(3)]
        neg = [-2 * ch[d] for d in range(3)]
        for dr, nb in kept:
            d = dr >> 1
            nh = float(L[nb, d]) / 2.0
            if dr & 1:
                pos[d] = ch[d] + nh
            else:
                neg[d] = -1.0 * (ch[d] + nh)
        tot = [pos[d] - neg[d] for d in range(3)]
        f = [0.0] * 6
        for dr, nb in kept:
            d = dr >> 1
            if dr & 1:
                f[dr] = +2.0 / (pos[d] * tot[d])
            else:
                f[dr] = -2.0 / (neg[d] * tot[d])
        out.f[c] = f
        out.sf[c] = -f[1] - f[0] - f[3] - f[2] - f[5] - f[4]  # 809-816
        for dr, nb in kept:
            kept_rows.append((c, dr, nb, 1 if levels[nb] > levels[c] else 0))
    out.kept = np.array(kept_rows, np.int64).reshape(-1, 4)
    return out


def factor_table(ch):
    """(n, 7) in FACTORS' order."""
    return np.concatenate([ch.sf[:, None], ch.f], axis=1)


def _apply(ch, sel, x, transpose):
    """scaling_factor * x + sum over kept neighbors of multiplier * x[nb] per
    cell (290-339; transpose: 421-467, the neighbor's factor toward the cell)."""
    c, dr, nb, finer = (ch.kept[:, k] for k in range(4))
    mul = ch.f[nb, dr ^ 1] if transpose else ch.f[c, dr]
    mul = np.where(finer == 1, mul / 4.0, mul)
    acc = ch.sf * x
    np.add.at(acc, c, mul * x[nb])  # in row order: per cell by direction, then neighbor
    return np.where(sel, acc, 0.0)


def _sum(v):
    s = 0.0
    for x in v.tolist():
        s += x
    return s


def solve(ch, rhs, solution, max_iterations=1000, min_iterations=0, stop_residual=1e-15, p_of_norm=2.0,
          stop_after_residual_increase=10.0):
    """Returns (state dict of STATE arrays, iterations, smallest residual)."""
    sel = ch.type == SOLVE
    info = ch.type != SKIP  # cell_info: every cell that kept a neighbor
    rhs = np.asarray(rhs, np.float64)
    sol = np.array(solution, np.float64)
    n = sol.size
    best, ap0 = np.zeros(n), np.zeros(n)
    # initialize_solver 986-1051: r0 = rhs - A . solution, subtracting term by term
    c, dr, nb, finer = (ch.kept[:, k] for k in range(4))
    mul = np.where(finer == 1, ch.f[c, dr] / 4.0, ch.f[c, dr])
    r0 = rhs - ch.sf * sol
    np.subtract.at(r0, c, mul * sol[nb])
    r0 = np.where(sel, r0, 0.0)
    p0, p1, r1 = r0.copy(), r0.copy(), r0.copy()
    dot_r = _sum((r0 * r1)[sel])
    residual_min = np.finfo(np.float64).max
    iteration = 0
    while True:
        iteration += 1
        ap0 = _apply(ch, sel, p0, False)
        dot_p = _sum((p1 * ap0)[sel])
        if dot_p == 0:
            break
        alpha = dot_r / dot_p
        sol = np.where(sel, sol + alpha * p0, sol)
        residual = _sum((np.abs(r0) ** p_of_norm)[info]) ** (1.0 / p_of_norm)  # get_residual 677-687
        if residual_min > residual:
            residual_min = residual
            best = np.where(sel, sol, best)
        if residual <= stop_residual and iteration >= min_iterations:
            break
        if residual >= stop_after_residual_increase * residual_min and iteration >= min_iterations:
            break
        r0 = np.where(sel, r0 - alpha * ap0, r0)
        r1 = np.where(sel, r1 - alpha * _apply(ch, sel, p1, True), r1)
        if dot_r == 0:
            break
        old = dot_r
        dot_r = _sum((r0 * r1)[sel])
        beta = dot_r / old
        p0 = np.where(sel, r0 + beta * p0, p0)
        p1 = np.where(sel, r1 + beta * p1, p1)
        if iteration >= max_iterations:
            break
    sol = np.where(sel, best, sol)  # 514-519
    state = dict(solution=sol, best_solution=best, p0=p0, p1=p1, r0=r0, r1=r1, A_dot_p0=ap0)
    return state, iteration, residual_min


# ---- tests/poisson/poisson1d_stretched.cpp ---------------------------------------
STRETCHED1D_SIZES = tuple(8 << k for k in range(8))  # 8 ... 1024
STRETCHED1D_SOLVER = (10, 0, 1e-5, 2.0, 10.0)


def stretched1d_coords(n):
    """:205-255: [0, 2 pi] in four equal cells, then every cell divided 1:3
    with the smaller part toward 0 in the first and third quarter, toward
    2 pi in the others, until there are n cells."""
    pi = math.pi
    x = [0.0, pi / 2, pi, 3 * pi / 2, 2 * pi]
    ratio = 3.0
    while len(x) < n:
        new = [x[0]]
        for lo, hi in zip(x[:-1], x[1:]):
            middle = (hi + lo) / 2
            if middle < pi / 2 or (middle >= pi and middle < 3 * pi / 2):
                mid = hi - (hi - lo) * ratio / (ratio + 1)
            else:
                mid = lo + (hi - lo) * ratio / (ratio + 1)
            new += [mid, hi]
        x = new
    assert len(x) == n + 1
    return [np.array(x), np.array([0.0, 1.0]), np.array([0.0, 1.0])]


def poisson1d_stretched(n):
    """One size of the scenario on the model: dict(stretched=..., reference=...)
    of (2-norm against -sin(center), iterations, residual, solution)."""
    base, periodic = (n, 1, 1), (True, True, True)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    out = {}
    for name, coords in (("stretched", stretched1d_coords(n)),
                         ("reference", None)):
        if coords is None:  # Cartesian_Geometry :196-203
            h = 2 * math.pi / n
            ctr = np.array([0.0 + float(i) * h / 1.0 + (h * 1.0) / 2 for i in range(n)])
            L = np.tile(np.array([h * 1.0, 1.0, 1.0]), (n, 1))
            lvl = np.zeros(n, np.int64)
        else:
            lvl, c3, L = geometry(coords, base, 0, ids)
            ctr = c3[:, 0]
        ch = cache(ids, base, 0, periodic, lvl, L, np.zeros(n, np.int64))
        st, it, res = solve(ch, np.sin(ctr), np.zeros(n), *STRETCHED1D_SOLVER)
        norm = _sum(np.abs(st["solution"] - (-np.sin(ctr))) ** 2.0) ** (1.0 / 2.0)
        out[name] = (norm, it, res, st["solution"])
    return out
