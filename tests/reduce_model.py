"""NumPy model of dccrgx_field_reduce and dccrgx_particles_reduce.

The terms are formed in the contract's order, one IEEE operation per step
(NumPy float64 arithmetic rounds each product on its own).  A sum is the
exactly rounded sum of the terms (math.fsum); the extrema are exact.  Beside
the value the model gives what the tolerance of a sum needs: the number of
terms k and the sum of their magnitudes S, for

    |got - exact| <= gamma(k - 1) * S,   gamma(m) = m u / (1 - m u),  u = 2^-53,

which holds for the sum of k terms in any order and any tree.  The model
imports nothing of the product."""
import math

import numpy as np

U = 2.0 ** -53
OPS = ("sum", "min", "max", "max_abs")
EMPTY = {"sum": 0.0, "min": math.inf, "max": -math.inf, "max_abs": 0.0}


def gamma(m):
    return m * U / (1 - m * U) if m > 0 else 0.0


class Result:
    """value, and for a sum the number of terms k, the sum of their
    magnitudes S and the bound gamma(k - 1) * S (0.0 for an extremum)."""

    def __init__(self, value, k, S, terms=None):
        self.value, self.k, self.S, self.terms = np.float64(value), k, S, terms
        self.bound = gamma(k - 1) * S

    def error(self, got):
        """|got - exact| of a sum, rounded once."""
        return abs(math.fsum(self.terms + [-float(got)]))


def reduce_terms(op, t):
    """One operation over the float64 terms t (already formed)."""
    t = np.asarray(t, np.float64)
    if op == "sum":
        return Result(math.fsum(t.tolist()), t.size, math.fsum(np.abs(t).tolist()), t.tolist())
    if t.size == 0:
        return Result(EMPTY[op], 0, 0.0)
    if op == "min":
        return Result(t.min(), t.size, 0.0)
    if op == "max":
        return Result(t.max(), t.size, 0.0)
    assert op == "max_abs"
    return Result(np.abs(t).max(), t.size, 0.0)


def field_reduce(terms, n_cells, volumes=None):
    """terms: (op, a, b) with a, b float64 arrays over the n_cells cells or
    None for 1.0; volumes: (lx ly) lz per cell for by_volume, else None.
    t = a * b, and for a sum by volume t * V."""
    one = np.ones(n_cells, np.float64)
    out = []
    for op, a, b in terms:
        t = (one if a is None else np.asarray(a, np.float64)) * (one if b is None else np.asarray(b, np.float64))
        if volumes is not None and op == "sum":
            t = t * np.asarray(volumes, np.float64)
        out.append(reduce_terms(op, t))
    return out


def volumes(lengths):
    """(lx * ly) * lz per cell from (n, 3) lengths."""
    L = np.asarray(lengths, np.float64)
    return (L[:, 0] * L[:, 1]) * L[:, 2]


def particles_reduce(terms, records, weight=-1):
    """terms: (op, u, v) with u, v doubles of the record or -1 / None;
    records: (N, K) float64; m = (q * u) * v."""
    R = np.asarray(records, np.float64)
    N = R.shape[0]
    one = np.ones(N, np.float64)
    q = one if weight in (-1, None) else R[:, weight]
    out = []
    for op, u, v in terms:
        uu = one if u in (-1, None) else R[:, u]
        vv = one if v in (-1, None) else R[:, v]
        out.append(reduce_terms(op, (q * uu) * vv))
    return out
