"""The model of dccrgx_particles_remove (tests/particles_remove_model.py) on
cases worked by hand, the chance stage's share, and the export."""
import ctypes

import numpy as np

import dccrg_amd
import particles_create_model as PC
import particles_remove_model as RM

INF = np.inf
NAN = np.nan


def _recs(rows):
    return np.array(rows, np.float64).reshape(-1, len(rows[0]))


def test_mask_nan_absorbs_and_negative_zero_does_not():
    r = _recs([[0, 0, 0, 1.0], [0, 0, 0, 2.0]])
    cells = {1: r.copy(), 2: r.copy(), 3: r.copy(), 4: r.copy()}
    st, _ = RM.remove(cells, 4, mask={1: NAN, 2: -0.0, 3: 0.0, 4: 1e-300})
    assert [cells[c].shape[0] for c in (1, 2, 3, 4)] == [0, 2, 2, 0]
    assert st == dict(kept=4, by_mask=4, by_test=0, by_chance=0)


def test_intervals_nan_empty_and_one_sided():
    r = _recs([[0.5, 0, 0, -1.0], [1.0, 0, 0, 0.0], [2.0, 0, 0, 1.0], [NAN, 0, 0, NAN], [INF, 0, 0, 3.0]])
    # keep inside [1, 2): 1.0 is in, 2.0 is not, NaN is not in and goes
    cells = {7: r.copy()}
    st, _ = RM.remove(cells, 4, tests=[(0, "keep", 1.0, 2.0)])
    assert np.array_equal(cells[7][:, 0], [1.0]) and st["by_test"] == 4
    # drop inside: NaN is not in and stays
    cells = {7: r.copy()}
    RM.remove(cells, 4, tests=[(0, "drop", 1.0, 2.0)])
    assert np.array_equal(cells[7][:, 3], [-1.0, 1.0, NAN, 3.0], equal_nan=True)
    # lo == hi: the empty interval; keep removes all, drop none
    cells = {7: r.copy()}
    assert RM.remove(cells, 4, tests=[(0, "keep", 1.0, 1.0)])[0]["kept"] == 0
    cells = {7: r.copy()}
    assert RM.remove(cells, 4, tests=[(0, "drop", 1.0, 1.0)])[0]["kept"] == 5
    # one-sided: x >= 1 is dropped, +inf < +inf is false so inf stays under (1, inf) but goes under keep (-inf, 1)
    cells = {7: r.copy()}
    RM.remove(cells, 4, tests=[(0, "drop", 1.0, INF)])
    assert np.array_equal(cells[7][:, 0], [0.5, NAN, INF], equal_nan=True)
    cells = {7: r.copy()}
    RM.remove(cells, 4, tests=[(3, "keep", -INF, 1.0)])
    assert np.array_equal(cells[7][:, 3], [-1.0, 0.0])


def test_the_first_stage_that_holds_counts():
    r = _recs([[0, 0, 0, 5.0], [0, 0, 0, -5.0]])
    cells = {1: r.copy(), 2: r.copy()}
    # cell 1 is masked (both by mask although the test and chance would take them too);
    # in cell 2 the test takes 5.0, chance (p = 1) the other
    st, _ = RM.remove(cells, 4, mask={1: 1.0, 2: 0.0}, tests=[(3, "drop", 0.0, INF)], prob=1.0)
    assert st == dict(kept=0, by_mask=2, by_test=1, by_chance=1)
    cells = {1: r.copy(), 2: r.copy()}
    st, _ = RM.remove(cells, 4, mask={1: 1.0, 2: 0.0}, tests=[(3, "drop", 0.0, INF)], prob=-1.0)
    assert st == dict(kept=1, by_mask=2, by_test=1, by_chance=0)
    st, _ = RM.remove({1: r.copy()}, 4, prob=NAN)
    assert st["kept"] == 2


def test_chance_uses_the_index_before_the_call():
    rng = np.random.default_rng(1)
    r = rng.random((40, 4))
    u = RM.chance_uniform(9, np.arange(40), seed=5)
    assert np.array_equal(u, PC.block_uniforms(np.full(40, 9, np.uint64), np.arange(40), 0xFFFFFFFE, 5)[0])
    cells = {9: r.copy()}
    gone_by_test = r[:, 0] < 0.5
    st, _ = RM.remove(cells, 4, tests=[(0, "drop", -INF, 0.5)], prob=0.5, seed=5)
    keep = ~gone_by_test & ~(u < 0.5)
    assert np.array_equal(cells[9], r[keep]) and st["by_chance"] == int(np.sum(~gone_by_test & (u < 0.5)))
    assert 0 < st["by_chance"] < 40 - int(gone_by_test.sum())


def test_rescale_is_one_difference_and_one_quotient():
    r = _recs([[0, 0, 0, 3.0, 7.0]] * 30)
    cells = {4: r.copy(), 5: r.copy(), 6: r.copy()}
    pf = {4: 0.1, 5: 0.0, 6: 10.0}
    st, _ = RM.remove(cells, 5, prob=0.7, prob_field=pf, seed=3, rescale=True, weight=3)
    p4 = np.float64(0.7) * np.float64(0.1)
    assert cells[4].shape[0] > 0 and np.all(cells[4][:, 3] == np.float64(3.0) / (np.float64(1.0) - p4))
    assert np.all(cells[4][:, 4] == 7.0)
    assert cells[5].shape[0] == 30 and np.all(cells[5][:, 3] == 3.0)  # p = 0: nothing rescaled
    assert cells[6].shape[0] == 0  # p >= 1
    # a record a test removes is not rescaled; one the chance stage keeps is, also when a test saw it first
    cells = {4: r.copy()}
    RM.remove(cells, 5, tests=[(4, "keep", 0.0, 10.0)], prob=0.25, seed=3, rescale=True, weight=3)
    assert np.all(cells[4][:, 3] == 4.0)


def test_tally_products_and_cells_without_a_removed_record():
    r = _recs([[0, 0, 0, 2.0, 3.0, 5.0], [0, 0, 0, 4.0, -1.0, 0.5], [0, 0, 0, 8.0, 1.0, 1.0]])
    cells = {1: r.copy(), 2: r.copy()}
    Q, P, E = {1: 1.0, 2: -0.0}, {1: 0.0, 2: -0.0}, {1: 0.25, 2: -0.0}
    st, mags = RM.remove(cells, 6, tests=[(3, "keep", 8.0, INF)], mask={1: 0.0, 2: 0.0}, weight=3,
                         tally=[((-1, -1), Q), ((4, -1), P), ((4, 5), E)])
    # removed: q = 2 and q = 4.  2 + 4;  2 * 3 + 4 * -1;  (2 * 3) * 5 + (4 * -1) * 0.5
    assert (Q[1], P[1], E[1]) == (7.0, 2.0, 28.25) and (Q[2], P[2], E[2]) == (6.0, 2.0, 28.0)
    assert mags[1][1] == (2, 10.0, 2.0) and mags[2][2] == (2, 32.0, 28.0)
    # nothing removed: the cell's bits stay (-0.0 + 0.0 would be +0.0)
    cells = {2: r.copy()}
    Z = {2: -0.0}
    RM.remove(cells, 6, tests=[(3, "keep", 0.0, INF)], weight=3, tally=[((-1, -1), Z)])
    assert np.signbit(Z[2])
    # weight -1: q = 1, a count
    cells = {2: r.copy()}
    Z = {2: 10.0}
    RM.remove(cells, 6, prob=2.0, tally=[((-1, -1), Z)])
    assert Z[2] == 13.0


def test_into_appends_in_source_order():
    r = _recs([[k, 0, 0, k % 2] for k in range(8)])
    cells = {3: r.copy(), 4: r[:0].copy()}
    into = {3: _recs([[100.0, 0, 0, 0]]), 4: r[:0].copy()}
    st, _ = RM.remove(cells, 4, tests=[(3, "drop", 1.0, 2.0)], into=into)
    assert np.array_equal(cells[3][:, 0], [0, 2, 4, 6]) and np.array_equal(into[3][:, 0], [100, 1, 3, 5, 7])
    assert into[4].shape == (0, 4) and st == dict(kept=4, by_mask=0, by_test=4, by_chance=0)


def test_chance_share():
    n, p, seed = 12_000, 0.3, 0xABCDEF
    cells = {c: np.zeros((n // 4, 3)) for c in (11, 12, 13, 1 << 40)}
    st, _ = RM.remove(cells, 3, prob=p, seed=seed)
    assert st["kept"] + st["by_chance"] == n
    assert abs(st["by_chance"] - n * p) <= 5 * np.sqrt(n * p * (1 - p))
    again = {c: np.zeros((n // 4, 3)) for c in cells}
    RM.remove(again, 3, prob=p, seed=seed + 1)
    assert any(cells[c].shape != again[c].shape for c in cells)


def test_particles_remove_is_exported():
    assert hasattr(dccrg_amd.lib(), "dccrgx_particles_remove")
    assert "dccrgx_particles_remove" in dccrg_amd.header_symbols()


def test_null_grid_is_rejected_without_gpu():
    st = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    one_i, one_d = (ctypes.c_int * 2)(), (ctypes.c_double * 2)()
    rc = dccrg_amd.lib().dccrgx_particles_remove(None, 0, 3, one_i, one_d, 0, -1, -1, 0.0, 0, 0, -1, one_i, one_i, 0,
                                                 -1, st)
    assert rc != 0 and list(st) == [7, 7, 7, 7]
