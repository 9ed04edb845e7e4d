"""NumPy model of dccrgx_particles_create (include/dccrgx.h): Philox4x32-10,
the two uniforms of a block, the counts, the positions with their clamp and
the recipe, vectorised over (cell, index).  Every operation is the one the
header names, in its order, so everything but the normals (log and cos are
library functions on both sides) compares bitwise with the device."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
KINDS = {"const": 0, "uniform": 1, "normal": 2}
TWO_PI = 6.283185307179586


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays holding 32-bit values) of the
    blocks with counter words c0..c3 (broadcast) under the key (k0, k1)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    m = np.uint64(MASK)
    s = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # 32 x 32 bits: no overflow
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> s) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> s) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & m, n2, p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(hi, lo):
    """53 bits of two words as a double in [0, 1)."""
    bits = (np.asarray(hi, np.uint64) << np.uint64(21)) | (np.asarray(lo, np.uint64) >> np.uint64(11))
    return bits.astype(np.float64) * 2.0 ** -53


def block_uniforms(ids, i, j, seed):
    """(first, second) of block j of record i of the cells ids."""
    ids = np.asarray(ids, np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(ids & np.uint64(MASK), ids >> np.uint64(32), i, j, seed & MASK, seed >> 32)
    return uniform(w[0], w[1]), uniform(w[2], w[3])


def counts(ids, count, field=None, random=False, seed=0):
    """n_c of every cell; ValueError names the first refused cell."""
    ids = np.asarray(ids, np.uint64)
    v = np.full(ids.size, np.float64(count)) if field is None else np.float64(count) * np.asarray(field, np.float64)
    bad = ~(v >= 0.0) | (v >= 2.0 ** 31)
    if bad.any():
        raise ValueError(f"the count of cell {int(ids[np.argmax(bad)])} is NaN, negative or at least 2^31")
    if random:
        u, _ = block_uniforms(ids, MASK, MASK, seed)
        v = v + u
    return np.floor(v).astype(np.int64)


def position(center, length, u):
    """x = center + (u - 0.5) L clamped to [lo, pred(hi)]."""
    center, length, u = (np.asarray(a, np.float64) for a in (center, length, u))
    h = u - 0.5
    off = h * length
    x = center + off
    half = length / 2
    lo = center - half
    hi = center + half
    return np.minimum(np.maximum(x, lo), np.nextafter(hi, -np.inf))


def normal_z(first, second):
    w = 1.0 - first
    t = -2.0 * np.log(w)
    r = np.sqrt(t)
    theta = TWO_PI * second
    return r * np.cos(theta)


def _spec(spec):
    spec = tuple(spec)
    opts = {}
    if spec and isinstance(spec[-1], dict):
        opts, spec = spec[-1], spec[:-1]
    kind = KINDS[spec[0]] if isinstance(spec[0], str) else int(spec[0])
    a = np.float64(spec[1])
    b = np.float64(spec[2]) if len(spec) > 2 else np.float64(0)
    return kind, a, b, opts.get("base_field"), opts.get("spread_field")


def records(ids, n, centers, lengths, K, recipe=None, seed=0, with_z=False):
    """{id: (n_c, K) array} of the new records of the cells ids (n_c = n[k],
    centers / lengths (len(ids), 3) as Dccrg.geometry gives them).  recipe:
    {j: ("const", a) | ("uniform", a, b) | ("normal", a, b)}, each optionally
    followed by {"base_field": values per cell, "spread_field": values per
    cell}.  with_z: also {id: {j: (z, spread)}} for the normal doubles."""
    ids = np.asarray(ids, np.uint64)
    n = np.asarray(n, np.int64)
    centers, lengths = np.asarray(centers, np.float64), np.asarray(lengths, np.float64)
    cell = np.repeat(np.arange(ids.size), n)
    first_of = np.concatenate(([0], np.cumsum(n)))
    i = np.arange(cell.size) - first_of[cell]
    cid = ids[cell]
    out = np.zeros((cell.size, K))
    b0 = block_uniforms(cid, i, 0, seed)
    b1 = block_uniforms(cid, i, 1, seed)
    for d, u in enumerate((b0[0], b0[1], b1[0])):
        out[:, d] = position(centers[cell, d], lengths[cell, d], u)
    zs = {}
    for j, spec in (recipe or {}).items():
        kind, a, b, fa, fb = _spec(spec)
        base = np.full(cell.size, a) if fa is None else a * np.asarray(fa, np.float64)[cell]
        if kind == 0:
            out[:, j] = base
            continue
        spread = np.full(cell.size, b) if fb is None else b * np.asarray(fb, np.float64)[cell]
        u1, u2 = block_uniforms(cid, i, j, seed)
        z = u1 if kind == 1 else normal_z(u1, u2)
        sz = spread * z
        out[:, j] = base + sz
        if kind == 2:
            zs[j] = (z, spread)
    res = {int(c): out[first_of[k]:first_of[k + 1]] for k, c in enumerate(ids)}
    if not with_z:
        return res
    zz = {int(c): {j: (z[first_of[k]:first_of[k + 1]], s[first_of[k]:first_of[k + 1]]) for j, (z, s) in zs.items()}
          for k, c in enumerate(ids)}
    return res, zz
