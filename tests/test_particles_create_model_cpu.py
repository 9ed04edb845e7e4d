"""The NumPy model of dccrgx_particles_create (tests/particles_create_model.py)
against the known answers of Philox4x32-10 and its own properties, and the
call's presence in the native library.  No GPU."""
import ctypes

import numpy as np

import dccrg_amd
import particles_create_model as PC
from test_gpu_particles_deposit import ODD_L0, ODD_START

# shared with tests/test_gpu_particles_create.py
STATS_SEED, STATS_CELLS, STATS_PER_CELL = 20261, 512, 512  # N = 2^18 normals
ROUND_SEED = 77


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    f = 0xFFFFFFFF
    assert _hex(PC.philox4x32_10(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(PC.philox4x32_10(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(PC.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over the counter: the same words
    w = PC.philox4x32_10(np.array([0, 0x243F6A88]), np.array([0, 0x85A308D3]), np.array([0, 0x13198A2E]),
                         np.array([0, 0x03707344]), 0, 0)
    assert _hex(x[0] for x in w) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


def test_uniforms_are_in_the_unit_interval_and_use_53_bits():
    assert PC.uniform(0, 0) == 0.0
    assert PC.uniform(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert PC.uniform(0, 1 << 11) == 2.0 ** -53 and PC.uniform(0, (1 << 11) - 1) == 0.0
    assert PC.uniform(0x80000000, 0) == 0.5
    u1, u2 = PC.block_uniforms(np.arange(1, 2001, dtype=np.uint64), 3, 5, 99)
    for u in (u1, u2):
        assert np.all((u >= 0) & (u < 1))
        bits = (u * 2.0 ** 53).astype(np.uint64)
        assert np.all(bits.astype(np.float64) == u * 2.0 ** 53)
        for b in (0, 20, 21, 52):  # the lowest bit, both sides of the seam of the two words, the highest
            frac = np.mean((bits >> np.uint64(b)) & np.uint64(1))
            assert 0.4 < frac < 0.6, (b, frac)
    assert not np.array_equal(u1, u2)


def _odd_cells():
    from oracle import oracle as O
    from helpers import random_refines

    o = O.Grid((8, 6, 4), 2, (True, True, False), 1, 1)
    o.set_geometry(ODD_START, ODD_L0)
    rng = np.random.default_rng(0)
    for _ in range(2):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        for c in random_refines(ids, lv, 2, rng, 0.1):
            o.refine_completely(c)
        o.stop_refining()
    ids, _ = o.cells()
    ctr, ln = o.geometry(ids)
    return np.asarray(ids, np.uint64), ctr, ln


def test_clamp_keeps_the_corners_inside():
    ids, ctr, ln = _odd_cells()
    lo, hi = ctr - ln / 2, ctr + ln / 2
    x0 = PC.position(ctr, ln, np.zeros_like(ctr))
    assert np.array_equal(x0, lo)  # (0 - 0.5) L is exactly -(L / 2)
    top = 1.0 - 2.0 ** -53
    x1 = PC.position(ctr, ln, np.full_like(ctr, top))
    assert np.all((x1 >= lo) & (x1 < hi))
    raw = ctr + (top - 0.5) * ln
    assert np.any(raw >= hi), "no cell of this geometry rounds up to hi: the clamp is not exercised"
    assert np.array_equal(x1[raw >= hi], np.nextafter(hi, -np.inf)[raw >= hi])
    assert np.array_equal(x1[raw < hi], raw[raw < hi])
    # around zero: pred(0) is the negative denormal
    assert PC.position(-1.0, 2.0, top) < 1.0 and PC.position(-0.5, 1.0, top) < 0.0


RECIPE = {3: ("const", 2.5), 4: ("uniform", -1.0, 2.0), 6: ("normal", 0.5, 3.0)}


def test_partition_independence_of_the_model():
    ids, ctr, ln = _odd_cells()
    rng = np.random.default_rng(3)
    n = rng.integers(0, 7, ids.size)
    whole = PC.records(ids, n, ctr, ln, 7, RECIPE, seed=5)
    h = ids.size // 3
    perm = rng.permutation(ids.size)  # another order and another split: the slot does not matter
    a, b = perm[:h], perm[h:]
    parts = {}
    for p in (a, b):
        parts.update(PC.records(ids[p], n[p], ctr[p], ln[p], 7, RECIPE, seed=5))
    assert sorted(parts) == sorted(whole)
    for c in whole:
        assert whole[c].shape == parts[c].shape
        assert np.array_equal(whole[c].view(np.uint64), parts[c].view(np.uint64)), c
    other = PC.records(ids, n, ctr, ln, 7, RECIPE, seed=6)
    assert any(not np.array_equal(whole[c], other[c]) for c in whole if whole[c].size)
    # inside their cells, the constant constant, the uniform in its range
    for k, c in enumerate(ids):
        r = whole[int(c)]
        assert np.all((r[:, 0:3] >= ctr[k] - ln[k] / 2) & (r[:, 0:3] < ctr[k] + ln[k] / 2))
        assert np.all(r[:, 3] == 2.5) and np.all(r[:, 5] == 0.0) and np.all((r[:, 4] >= -1.0) & (r[:, 4] < 1.0))


def stats_model_normals():
    ids = np.arange(1, STATS_CELLS + 1, dtype=np.uint64)
    n = np.full(ids.size, STATS_PER_CELL)
    one = np.ones((ids.size, 3))
    recs = PC.records(ids, n, one, one, 4, {3: ("normal", 0.0, 1.0)}, seed=STATS_SEED)
    return np.concatenate([recs[int(c)][:, 3] for c in ids])


def test_the_statistics_seed_meets_the_gpu_tests_bounds():
    z = stats_model_normals()
    N = z.size
    assert N == 2 ** 18
    mean = z.sum() / N
    var = (z * z).sum() / N - mean * mean
    print("model normals: mean", mean, "variance", var)
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1.0) <= 5 * np.sqrt(2.0 / N)


def test_random_rounding_total_of_the_model():
    ids = np.arange(1, 513, dtype=np.uint64)
    n = PC.counts(ids, 1.0, np.full(512, 0.5), random=True, seed=ROUND_SEED)
    assert set(np.unique(n)) == {0, 1}
    assert abs(int(n.sum()) - 256) <= 5 * np.sqrt(512 * 0.25)
    assert np.array_equal(PC.counts(ids, 2.75), np.full(512, 2))
    for bad in (np.nan, -1.0, 2.0 ** 31):
        f = np.ones(512)
        f[17] = bad
        try:
            PC.counts(ids, 1.0, f)
        except ValueError as e:
            assert "cell 18 " in str(e)
        else:
            raise AssertionError("not refused")


def test_particles_create_is_exported():
    assert hasattr(dccrg_amd.lib(), "dccrgx_particles_create")
    assert "dccrgx_particles_create" in dccrg_amd.header_symbols()


def test_null_grid_is_rejected_without_gpu():
    L = dccrg_amd.lib()
    made = ctypes.c_uint64(7)
    rc = L.dccrgx_particles_create(None, 0, 3, -1, 1.0, 0, None, None, 0, ctypes.byref(made))
    assert rc == dccrg_amd._lib.EINVAL
