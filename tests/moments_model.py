"""Particle moments and the Boris kick in plain NumPy (a helper, not a test).

``MomentsModel`` stands for ``dccrgx_particles_deposit_moments``: over
``deposit_model.DepositModel`` it forms, with the shares W of
``DepositModel.shares`` and one IEEE operation per NumPy call in the header's
order, the terms ((q u) v) W of every moment, so the terms are bitwise the
device's and only the order of a sum differs.  Sums are ``math.fsum``.

``boris`` restates the formulas of ``dccrgx_particles_boris`` operation by
operation; the device is held to it bitwise.
"""
import math

import numpy as np

RHO_J_P = [(None, None), (3, None), (4, None), (5, None),
           (3, 3), (3, 4), (3, 5), (4, 4), (4, 5), (5, 5)]  # charge, current, the six of the pressure tensor


def _column(rec, k):
    return np.ones(rec.shape[0]) if k is None or k < 0 else rec[:, k]


def moment_values(rec, weight, u, v):
    """m(p) = (q u) v of the records rec (n, K): two rounded products."""
    qu = _column(rec, weight) * _column(rec, u)
    return qu * _column(rec, v)


class MomentsModel:
    def __init__(self, dm):
        self.dm = dm
        self.pm = dm.pm
        self._shares = {}

    def shares(self, s, shape):
        """DepositModel.shares, kept: they depend on the positions only (drop
        the model when the records move)."""
        sh = self._shares.get((s, shape))
        if sh is None:
            sh = self._shares[(s, shape)] = self.dm.shares(s, shape)
        return sh

    def moments(self, shape, weight, moments):
        """For each (u, v) of `moments`: {cell: (fsum of the terms, sum of
        |term|, number of non-zero terms)} over every leaf."""
        terms = {c: [[] for _ in moments] for c in self.pm.cells}
        for s, rec in self.pm.cells.items():
            if not rec.shape[0]:
                continue
            m = [moment_values(rec, weight, u, v) for u, v in moments]
            for c, w in self.shares(s, shape):
                for j in range(len(moments)):
                    terms[c][j].append(m[j] * w)
        outs = [{} for _ in moments]
        for c, per in terms.items():
            for j, parts in enumerate(per):
                t = np.concatenate(parts) if parts else np.zeros(0)
                outs[j][c] = (np.float64(math.fsum(t)), np.float64(math.fsum(np.abs(t))), int(np.count_nonzero(t)))
        return outs

    def totals(self, weight, moments):
        """For each moment (sum over all records of m(p), sum of |m(p)|)."""
        out = []
        for u, v in moments:
            m = [moment_values(rec, weight, u, v) for rec in self.pm.cells.values() if rec.shape[0]]
            m = np.concatenate(m) if m else np.zeros(0)
            out.append((math.fsum(m), math.fsum(np.abs(m))))
        return out


def boris(rec, e_first, b_first, weight, factor):
    """The records rec (n, K) after dccrgx_particles_boris: a copy with the
    new doubles 3..5; every operation one NumPy call, in the header's order."""
    out = rec.copy()
    n = rec.shape[0]
    factor = np.float64(factor)
    h = factor * rec[:, weight] if weight is not None and weight >= 0 else np.full(n, factor)
    v = [rec[:, 3 + j] for j in range(3)]
    hE = [h * rec[:, e_first + j] for j in range(3)]
    vm = [v[j] + hE[j] for j in range(3)]
    t = [h * rec[:, b_first + j] for j in range(3)]
    t2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
    den = np.float64(1.0) + t2
    s = [(np.float64(2.0) * t[j]) / den for j in range(3)]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    c = cross(vm, t)
    vp = [vm[j] + c[j] for j in range(3)]
    d = cross(vp, s)
    for j in range(3):
        vq = vm[j] + d[j]
        out[:, 3 + j] = vq + hE[j]
    return out


def accelerate(rec, first, weight, factor):
    """dccrgx_particles_accelerate's update (the header's order)."""
    out = rec.copy()
    factor = np.float64(factor)
    k = factor * rec[:, weight] if weight is not None and weight >= 0 else np.full(rec.shape[0], factor)
    for j in range(3):
        term = k * rec[:, first + j]
        out[:, 3 + j] = rec[:, 3 + j] + term
    return out
