"""NumPy model of dccrgx_particles_remove (include/dccrgx.h), per cell id as
ParticleModel holds its cells (a helper, not a test).  Every comparison and
operation is the one the header names, in its order: the verdicts, the kept
records, the rescaled weights and the order of the removed records compare
bitwise with the device.  A tally's sum is taken in index order here and in
an unspecified order on the device: bitwise where every partial sum is exact."""
import math

import numpy as np

import particles_create_model as PC

CHANCE_BLOCK = 0xFFFFFFFE
MODES = {"keep": 0, "drop": 1}
KEPT, BY_MASK, BY_TEST, BY_CHANCE = 0, 1, 2, 3


def chance_uniform(cid, i, seed):
    """u of the records with indices i of cell cid."""
    return PC.block_uniforms(np.full(np.shape(i), cid, np.uint64), i, CHANCE_BLOCK, seed)[0]


def verdicts(cid, rec, tests=(), mask=None, p=None, seed=0):
    """The stage (KEPT, BY_MASK, BY_TEST, BY_CHANCE) of every record of cell
    cid.  mask: the cell's mask value or None; p: the cell's p_c, or None for
    an inactive chance stage."""
    rec = np.asarray(rec, np.float64)
    n = rec.shape[0]
    v = np.zeros(n, np.int64)
    if mask is not None and np.float64(mask) != 0.0:
        v[:] = BY_MASK
    for j, mode, lo, hi in tests:
        mode = MODES[mode] if isinstance(mode, str) else int(mode)
        x = rec[:, int(j)]
        with np.errstate(invalid="ignore"):
            inside = (np.float64(lo) <= x) & (x < np.float64(hi))
        gone = inside if mode == 1 else ~inside
        v[(v == KEPT) & gone] = BY_TEST
    if p is not None and n:
        u = chance_uniform(cid, np.arange(n), seed)
        with np.errstate(invalid="ignore"):
            v[(v == KEPT) & (u < np.float64(p))] = BY_CHANCE
    return v


def moment(rec, weight, u, v):
    """m = (q * u) * v of every record, each product rounded."""
    rec = np.asarray(rec, np.float64)
    one = np.ones(rec.shape[0])
    q = one if weight == -1 else rec[:, weight]
    qu = q * (one if u == -1 else rec[:, u])
    return qu * (one if v == -1 else rec[:, v])


def remove(cells, K, tests=(), mask=None, prob=0.0, prob_field=None, seed=0, rescale=False, weight=-1, tally=(),
           into=None):
    """cells: {id: (n, K) array}, changed in place.  mask / prob_field: {id:
    value} or None.  tally: ((u, v), {id: value}) pairs, the dicts changed in
    place (only cells that lose a record).  into: {id: array}, changed in place.  Returns
    (stats dict, [per tally {id: (removed records k, sum |m|, the exactly
    rounded sum of m)}]): reduce_model's bound gamma(k - 1) sum |m| holds for
    a sum of the k terms in any order."""
    if rescale and weight == -1:
        raise ValueError("rescale needs a weight")
    active = prob_field is not None or np.float64(prob) != 0.0
    stats = np.zeros(4, np.int64)
    mags = [dict() for _ in tally]
    for cid in sorted(cells):
        rec = cells[cid]
        p = None
        if active:
            p = np.float64(prob) if prob_field is None else np.float64(prob) * np.float64(prob_field[cid])
        v = verdicts(cid, rec, tests, None if mask is None else mask[cid], p, seed)
        stats += np.bincount(v, minlength=4)
        keep = v == KEPT
        gone = rec[~keep]
        if gone.shape[0]:
            for t, ((fu, fv), fld) in enumerate(tally):
                m = moment(gone, weight, fu, fv)
                s = np.float64(0)
                for x in m:
                    s = s + x
                fld[cid] = np.float64(fld[cid]) + s
                mags[t][cid] = (gone.shape[0], float(np.sum(np.abs(m))), math.fsum(m))
            if into is not None:
                into[cid] = np.concatenate([into[cid].reshape(-1, K), gone])
        kept = rec[keep].copy()
        if rescale and p is not None and 0.0 < p < 1.0 and kept.shape[0]:
            rest = np.float64(1.0) - p
            kept[:, weight] = kept[:, weight] / rest
        cells[cid] = kept
    return dict(kept=int(stats[0]), by_mask=int(stats[1]), by_test=int(stats[2]), by_chance=int(stats[3])), mags
