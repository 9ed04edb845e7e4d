"""Charge deposition and field gather in plain NumPy (a helper, not a test).

One global address space over ``oracle.Grid`` and
``particles_model.ParticleModel``: a record p held by leaf s gives leaf c the
share W(p, c) of ``dccrgx_particles_deposit`` / ``dccrgx_particles_gather``
(include/dccrgx.h), formed with one IEEE operation per NumPy call in the
header's order, so the terms q W and W F are bitwise those of the device and
only the order of a sum differs.  Sums are ``math.fsum`` (correctly rounded),
so the model's own error is half a unit in the last place of the sum.
"""
import math

import numpy as np


class DepositModel:
    def __init__(self, pm):
        self.pm = pm
        o = pm.o
        ids = pm.leaves
        b = o.mapping.batch(ids)
        fine = np.float64(1 << pm.R)
        self.box = {}
        for c, lvl, ind in zip(ids, b["level"], b["indices"]):
            along = ind.astype(np.float64) * pm.l0
            lo = pm.start + along / fine
            L = pm.l0 * (np.float64(1.0) / np.float64(1 << int(lvl)))
            self.box[int(c)] = (lo, L, lo + L)
        self.period = np.asarray(o.length, np.uint64).astype(np.float64) * pm.l0
        self._recv = {}

    # ---- the weight -----------------------------------------------------
    def candidates(self, cell):
        """The cell, then the distinct other leaves of its neighbors_of, ascending."""
        r = self._recv.get(cell)
        if r is None:
            r = self._recv[cell] = [cell] + sorted(self.pm.neighbors_of(cell) - {cell})
        return r

    def volume(self, cell):
        L = self.box[cell][1]
        return (L[0] * L[1]) * L[2]

    def weight(self, x, s, c):
        """W(p, c) of the records at x (n, 3) held by leaf s (shape 1)."""
        lo_s, L_s, hi_s = self.box[s]
        lo_c, _, hi_c = self.box[c]
        f = []
        for d in range(3):
            xc = np.minimum(np.maximum(x[:, d], lo_s[d]), hi_s[d])
            half = L_s[d] / np.float64(2)
            a = xc - half
            b = xc + half

            def overlap(k):
                shift = np.float64(k) * self.period[d]
                top = np.minimum(b, hi_c[d] + shift)
                bottom = np.maximum(a, lo_c[d] + shift)
                return np.maximum(np.float64(0), top - bottom)

            o = overlap(0)
            if self.pm.periodic[d]:
                lower = overlap(-1) + o
                o = lower + overlap(1)
            f.append(o / L_s[d])
        return (f[0] * f[1]) * f[2]

    def shares(self, s, shape):
        """[(c, W of every record of s for c)] over the candidates of s."""
        rec = self.pm.cells[s]
        if shape == 0:
            return [(s, np.ones(rec.shape[0]))]
        return [(c, self.weight(rec[:, 0:3], s, c)) for c in self.candidates(s)]

    # ---- deposit ----------------------------------------------------------
    def deposit(self, shape=1, weight=3, per_volume=False, volumes=None):
        """{cell: (sum, sum of |term|, number of non-zero terms, volume)} over
        every leaf; the sum is divided by the volume with per_volume
        (`volumes`: {cell: V} instead of the Cartesian (lx ly) lz)."""
        return self.deposit_many(shape, [weight], per_volume, volumes)[0]

    def deposit_many(self, shape, weights, per_volume=False, volumes=None):
        """deposit() for each of several weight doubles; the shares are formed once."""
        outs = [{} for _ in weights]
        for c in self.pm.cells:
            terms = [[] for _ in weights]
            for s in ([c] if shape == 0 else self.candidates(c)):
                rec = self.pm.cells[s]
                if not rec.shape[0]:
                    continue
                w = np.ones(rec.shape[0]) if shape == 0 else self.weight(rec[:, 0:3], s, c)
                for k, weight in enumerate(weights):
                    q = np.ones(rec.shape[0]) if weight is None or weight < 0 else rec[:, weight]
                    terms[k].append(q * w)
            for k in range(len(weights)):
                t = np.concatenate(terms[k]) if terms[k] else np.zeros(0)
                total = np.float64(math.fsum(t))
                V = np.float64(1)
                if per_volume:
                    V = np.float64(volumes[c]) if volumes is not None else self.volume(c)
                    total = total / V
                outs[k][c] = (total, np.float64(math.fsum(np.abs(t))), int(np.count_nonzero(t)), V)
        return outs

    # ---- gather -------------------------------------------------------------
    def gather(self, fields, shape=1):
        """fields: a list of {cell: value}.  {cell: (values (n, nf), sums of
        |W F| (n, nf), number of candidates with W > 0 (n,))} for the records
        of every leaf."""
        out = {}
        nf = len(fields)
        for s, rec in self.pm.cells.items():
            n = rec.shape[0]
            val, mag, cnt = np.zeros((n, nf)), np.zeros((n, nf)), np.zeros(n, np.int64)
            if n:
                sh = self.shares(s, shape)
                cnt = sum((w > 0).astype(np.int64) for _, w in sh)
                for j, F in enumerate(fields):
                    terms = np.stack([w * np.float64(F[c]) for c, w in sh], axis=1)
                    val[:, j] = [math.fsum(r) for r in terms]
                    mag[:, j] = [math.fsum(r) for r in np.abs(terms)]
            out[s] = (val, mag, cnt)
        return out

    def apply_gather(self, fields, first_double, shape=1):
        """The gather stored into the model's records, as the device does."""
        res = self.gather(fields, shape)
        for s, (val, _, _) in res.items():
            self.pm.cells[s][:, first_double:first_double + len(fields)] = val
        return res
