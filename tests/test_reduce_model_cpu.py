"""tests/reduce_model.py against hand-written cases, and the tolerance the GPU
tests hold a sum to:

    |got - exact| <= gamma(k - 1) * sum |t_i|,  gamma(m) = m u / (1 - m u),  u = 2^-53.

The bound is not vacuous and not too tight: a plain left-to-right float64 loop
and np.sum (pairwise) over 17 408 random values in [-1, 1) stay inside it, and
a perturbation of one term by 2^-40 relative leaves it.

On the perturbation: with k = 17 408 terms gamma(k - 1) is 1.93e-12, more than
2^-40 = 9.09e-13, and sum |t_i| is at least the perturbed term's magnitude, so
over those 17 408 values no relative perturbation of 2^-40 of one term can leave
the bound (asserted below: it is 5.4e-5 of the bound for the largest term).
gamma(k - 1) < 2^-40 needs k <= 8192.  The perturbation is therefore shown
where it can show something: on 4 096 terms of which one dominates (1e16 among
ones, the GPU tests' large dynamic range), where the same bound formula gives
4.5e3 and the perturbation is 9.1e3."""
import math

import numpy as np

import reduce_model as RM


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_hand_written_cases():
    a = np.array([1.5, -2.0, 0.25, -0.125])
    b = np.array([2.0, 3.0, -4.0, 8.0])
    r = RM.field_reduce([("sum", a, b), ("min", a, b), ("max", a, b), ("max_abs", a, b), ("sum", a, None),
                         ("max_abs", None, b), ("sum", None, None), ("min", a, a)], 4)
    # a * b = 3, -6, -1, -1
    assert [float(x.value) for x in r] == [-5.0, -6.0, 3.0, 6.0, -0.375, 8.0, 4.0, 0.015625]
    assert r[0].k == 4 and r[0].S == 11.0 and r[0].bound == RM.gamma(3) * 11.0
    assert r[1].bound == 0.0
    # by volume: only the sums
    V = np.array([0.5, 2.0, 1.0, 4.0])
    rv = RM.field_reduce([("sum", a, b), ("max", a, b), ("sum", None, None)], 4, V)
    assert [float(x.value) for x in rv] == [1.5 - 12.0 - 1.0 - 4.0, 3.0, 7.5]


def test_a_cancelling_pair_and_the_order_of_the_products():
    # fsum: 1e16 + 1 - 1e16 is 1, which no float64 left-to-right order gives
    t = np.array([1e16, 1.0, -1e16])
    assert float(RM.reduce_terms("sum", t).value) == 1.0
    assert (1e16 + 1.0) - 1e16 != 1.0
    # (q * u) * v is not q * (u * v): the model keeps the contract's order
    rec = np.zeros((1, 7))
    rec[0, 3:] = [0.1, 0.7, 0.3, 3.0]
    m = RM.particles_reduce([("sum", 3, 4)], rec, weight=6)[0].value
    assert _bits(m) == _bits((np.float64(3.0) * np.float64(0.1)) * np.float64(0.7))
    assert _bits(m) != _bits(np.float64(3.0) * (np.float64(0.1) * np.float64(0.7)))


def test_empty_and_one_element():
    e = RM.field_reduce([(op, None, None) for op in RM.OPS], 0)
    assert [float(x.value) for x in e] == [0.0, math.inf, -math.inf, 0.0]
    assert not np.signbit(e[0].value) and not np.signbit(e[3].value) and all(x.bound == 0.0 for x in e)
    a = np.array([-0.3])
    one = RM.field_reduce([(op, a, a) for op in RM.OPS], 1, np.array([0.7]))
    sq = np.float64(-0.3) * np.float64(-0.3)
    assert _bits(one[0].value) == _bits(sq * np.float64(0.7)) and one[0].bound == 0.0  # gamma(0) = 0: bitwise
    assert all(_bits(x.value) == _bits(sq) for x in one[1:])
    rec = np.zeros((0, 7))
    assert [float(x.value) for x in RM.particles_reduce([(op, 3, None) for op in RM.OPS], rec)] == [
        0.0, math.inf, -math.inf, 0.0]


def test_particles_terms():
    rec = np.array([[0, 0, 0, 1.0, -2.0, 0.5, 2.0], [0, 0, 0, -3.0, 1.0, 0.25, -1.0]])
    r = RM.particles_reduce([("sum", None, None), ("sum", 3, None), ("sum", 3, 3), ("max_abs", 4, None)], rec, weight=6)
    assert [float(x.value) for x in r] == [1.0, 5.0, 2.0 - 9.0, 4.0]
    r = RM.particles_reduce([("sum", -1, -1), ("max_abs", 3, -1), ("min", 3, 4)], rec)
    assert [float(x.value) for x in r] == [2.0, 3.0, -3.0]


def _loop_sum(t):
    acc = np.float64(0.0)
    for x in t:
        acc = acc + x
    return acc


def test_the_bound_is_neither_vacuous_nor_too_tight():
    t = np.random.default_rng(17408).random(17408) * 2 - 1
    r = RM.reduce_terms("sum", t)
    assert r.k == 17408 and r.bound == RM.gamma(17407) * r.S
    for got in (_loop_sum(t), np.sum(t)):
        err = abs(math.fsum(t.tolist() + [-float(got)]))
        print(f"error {err:.3e} of the bound {r.bound:.3e}")
        assert err <= r.bound
    # here a 2^-40 relative perturbation of one term cannot leave: gamma(17407) > 2^-40 and S >= |t_i|
    assert RM.gamma(17407) > 2.0 ** -40 > RM.gamma(8191)
    i = int(np.argmax(np.abs(t)))
    assert abs(t[i]) * 2.0 ** -40 < 1e-4 * r.bound
    # where one term dominates 4 096 of them the same perturbation leaves the same bound
    d = np.ones(4096)
    d[1234] = 1e16
    rd = RM.reduce_terms("sum", d)
    for got in (_loop_sum(d), np.sum(d)):
        assert abs(math.fsum(d.tolist() + [-float(got)])) <= rd.bound
    p = d.copy()
    p[1234] = d[1234] * (1 + 2.0 ** -40)
    for got in (_loop_sum(p), np.sum(p)):
        assert abs(math.fsum(d.tolist() + [-float(got)])) > rd.bound
