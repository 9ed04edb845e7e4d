"""The curl, the divergence and the axpy of dccrgx_curl, dccrgx_divergence and
dccrgx_field_axpy (include/dccrgx.h) on a refined grid, NumPy only (a helper,
not a test).

The derivative D_d(F_j) of the contract is gradient_model.gradient of F_j at
scale 1.0, component d; on top of it the contract's steps are restated one
rounded fp64 operation per NumPy operation:

    curl:        r_k = D_d1(F_d2) - D_d2(F_d1), (k, d1, d2) cyclic;
                 t_k = scale * r_k;  out_k = t_k  or  prev_k + t_k
    divergence:  r = (D_0(F_0) + D_1(F_1)) + D_2(F_2);  t = scale * r;
                 out = t  or  prev + t
    axpy:        y + (a * x)

Besides the values each returns per output
* M:     the sum of the magnitudes gradient_model returns for the derivatives
         that took part (every rounding of the output is a fraction of
         2^-52 |scale| M, a previous content's own rounding apart),
* finer: whether a group of four finer cells took part in any of them (only
         then the order of a sum is the kernel's own).
"""
import numpy as np

import gradient_model as GM

NEXT = (1, 2, 0)


class Result:
    """value, M float64 and finer bool: (n, 3) for a curl, (n,) for a divergence."""


def derivatives(ids, base, R, periodic, lengths, fields):
    """gradient_model.gradient at scale 1.0 of each of the three fields."""
    assert len(fields) == 3
    return [GM.gradient(ids, base, R, periodic, lengths, f, 1.0) for f in fields]


def curl_of(G, scale=1.0, prev=None):
    """The curl from the three fields' gradients G (derivatives())."""
    n = G[0].grad.shape[0]
    scale = np.float64(scale)
    out = Result()
    out.value = np.zeros((n, 3))
    out.M = np.zeros((n, 3))
    out.finer = np.zeros((n, 3), bool)
    for k in range(3):
        d1 = NEXT[k]
        d2 = NEXT[d1]
        r = G[d2].grad[:, d1] - G[d1].grad[:, d2]
        t = scale * r
        out.value[:, k] = t if prev is None else np.asarray(prev[k], np.float64) + t
        out.M[:, k] = G[d2].M[:, d1] + G[d1].M[:, d2]
        out.finer[:, k] = G[d2].finer[:, d1] | G[d1].finer[:, d2]
    return out


def divergence_of(G, scale=1.0, prev=None):
    scale = np.float64(scale)
    out = Result()
    r = (G[0].grad[:, 0] + G[1].grad[:, 1]) + G[2].grad[:, 2]
    t = scale * r
    out.value = t if prev is None else np.asarray(prev, np.float64) + t
    out.M = G[0].M[:, 0] + G[1].M[:, 1] + G[2].M[:, 2]
    out.finer = G[0].finer[:, 0] | G[1].finer[:, 1] | G[2].finer[:, 2]
    return out


def curl(ids, base, R, periodic, lengths, fields, scale=1.0, prev=None):
    return curl_of(derivatives(ids, base, R, periodic, lengths, fields), scale, prev)


def divergence(ids, base, R, periodic, lengths, fields, scale=1.0, prev=None):
    return divergence_of(derivatives(ids, base, R, periodic, lengths, fields), scale, prev)


def axpy(y, a, x):
    p = np.float64(a) * np.asarray(x, np.float64)
    return np.asarray(y, np.float64) + p
