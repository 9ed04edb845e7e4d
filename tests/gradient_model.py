"""The cell-centred gradient of dccrgx_gradient (include/dccrgx.h) on a refined
grid, NumPy only (a helper, not a test).

It knows nothing of the library: the faces come from advection_model.faces
(leaves painted into an array of finest cells), the lengths from
stretched_model.cell_geometry or the Cartesian expression l0 * (1 / 2^level),
exactly as poisson_stretched_model obtains them.  The header's contract is
restated in fp64, one rounded operation per Python operation; the four values
of a finer group are summed with math.fsum.

Cells are positions in the id list given; directions are 0..5 = -x, +x, -y,
+y, -z, +z.

gradient() returns per cell and dimension
* grad:  scale * the gradient,
* finer: whether a group of four finer cells took part (only then the order
  of a sum is the kernel's own),
* M:     the magnitude |a| (|v_pos|+ + |v_c|) + |b| (|v_c| + |v_neg|+), or
  its one-sided form (|v|+ + |v_c|) / h; |v|+ is the mean of the absolute
  values for a group.  Every rounding error of the contract's operations is
  a fraction of 2^-52 M.
* both:  whether the cell has a neighbor on both sides of the dimension.
"""
import math

import numpy as np

import advection_model as AM
import poisson_stretched_model as PM


def cartesian_lengths(l0, levels):
    """l0 * (1 / 2^level) per cell and dimension (Cartesian get_length; what
    a grid holding only a file block without coordinates sees, too)."""
    return np.asarray(l0, np.float64)[None, :] * (1.0 / np.float64(2.0) ** np.asarray(levels))[:, None]


def stretched_lengths(coords, base, R, ids):
    return PM.geometry(coords, base, R, ids)[2]


def levels(ids, base, R):
    return AM.boxes(ids, base, R)[0]


class Gradient:
    """What gradient() returns: grad, M (n, 3) float64; finer, both (n, 3) bool."""


def gradient(ids, base, R, periodic, lengths, values, scale=1.0):
    ids = np.asarray(ids, np.uint64)
    n = ids.size
    F = AM.faces(ids, base, R, periodic)
    L = np.asarray(lengths, np.float64)
    val = [float(x) for x in np.asarray(values, np.float64)]
    scale = float(scale)
    sides = [[[] for _ in range(6)] for _ in range(n)]
    for c, dr, nb in F:
        sides[int(c)][int(dr)].append(int(nb))
    out = Gradient()
    out.grad = np.zeros((n, 3))
    out.M = np.zeros((n, 3))
    out.finer = np.zeros((n, 3), bool)
    out.both = np.zeros((n, 3), bool)

    def side(c, d, nbs):
        """(h, v, |v|+, finer) of one side."""
        hc = float(L[c, d]) / 2.0
        h = hc + float(L[nbs[0], d]) / 2.0
        if len(nbs) == 1:
            return h, val[nbs[0]], abs(val[nbs[0]]), False
        assert len(nbs) == 4, "a face has one neighbor or four finer ones"
        v = math.fsum(val[k] for k in nbs) / 4.0
        return h, v, math.fsum(abs(val[k]) for k in nbs) / 4.0, True

    for c in range(n):
        vc = val[c]
        for d in range(3):
            neg, pos = sides[c][2 * d], sides[c][2 * d + 1]
            grad = mag = 0.0
            finer = False
            if neg and pos:
                h_neg, v_neg, m_neg, f0 = side(c, d, neg)
                h_pos, v_pos, m_pos, f1 = side(c, d, pos)
                finer = f0 or f1
                tot = h_pos + h_neg
                a = h_neg / (h_pos * tot)
                b = h_pos / (h_neg * tot)
                t_pos = a * (v_pos - vc)
                t_neg = b * (vc - v_neg)
                grad = t_pos + t_neg
                mag = abs(a) * (m_pos + abs(vc)) + abs(b) * (abs(vc) + m_neg)
            elif pos:
                h_pos, v_pos, m_pos, finer = side(c, d, pos)
                grad = (v_pos - vc) / h_pos
                mag = (m_pos + abs(vc)) / h_pos
            elif neg:
                h_neg, v_neg, m_neg, finer = side(c, d, neg)
                grad = (vc - v_neg) / h_neg
                mag = (abs(vc) + m_neg) / h_neg
            out.grad[c, d] = scale * grad
            out.M[c, d] = mag
            out.finer[c, d] = finer
            out.both[c, d] = bool(neg) and bool(pos)
    return out
