"""The moments and Boris models (tests/moments_model.py) on the CPU.

The moments model forms the terms of dccrgx_particles_deposit_moments over the
deposit model's shares: its charge moment is the deposit model's sum to the
bit, and on a periodic grid every moment summed over the cells is the moment
summed over the records.  The Boris model with B = 0 is two accelerate
updates to the bit; with E = 0 it is a rotation: |v| is kept and the angle
about B is 2 atan(h B).  The two C entry points are declared and exported."""
import math

import numpy as np
import pytest

from moments_model import RHO_J_P, MomentsModel, accelerate, boris
from test_deposit_model_cpu import _model
from test_gpu_particles_deposit import _share_tol

EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def periodic_refined():
    pm, dm = _model((4, 4, 4), 2, (True, True, True), 2, 71, K=10)
    return pm, dm, MomentsModel(dm)


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("weight", [6, None])
def test_charge_moment_is_the_deposit_model_bitwise(periodic_refined, shape, weight):
    pm, dm, mm = periodic_refined
    assert pm.total() > 100
    got = mm.moments(shape, weight, [(3, 4), (None, None)])[1]
    exp = dm.deposit(shape, weight)
    for c, (total, mag, cnt, _) in exp.items():
        assert got[c][0].tobytes() == np.float64(total).tobytes(), c
        assert got[c][1].tobytes() == np.float64(mag).tobytes() and got[c][2] == cnt, c


@pytest.mark.parametrize("weight", [6, None])
def test_moments_are_conserved_on_a_periodic_grid(periodic_refined, weight):
    """sum_c of a moment = sum_p m(p) sum_c W(p, c): each cell's fsum is within
    half a unit of its exact sum (at most EPS sum|term|), the outer fsums two
    half units more, and sum_c W is 1 within the share tolerance."""
    pm, dm, mm = periodic_refined
    outs = mm.moments(1, weight, RHO_J_P)
    for (total, mag), out in zip(mm.totals(weight, RHO_J_P), outs):
        cells = math.fsum(v[0] for v in out.values())
        bound = sum(EPS * v[1] for v in out.values()) + (2 * EPS + _share_tol(pm)) * mag
        assert mag > 0 and abs(cells - total) <= bound, (cells, total, bound)
    ngp = mm.moments(0, weight, RHO_J_P)
    for (total, mag), out in zip(mm.totals(weight, RHO_J_P), ngp):
        assert abs(math.fsum(v[0] for v in out.values()) - total) <= 2 * EPS * mag


def _records(rng, n, K=13):
    rec = rng.random((n, K)) * 2 - 1
    rec[:, 3:6] = np.where(np.abs(rec[:, 3:6]) < 1e-3, 0.5, rec[:, 3:6])  # no zero velocities
    return rec


@pytest.mark.parametrize("weight", [6, None])
def test_boris_without_b_is_two_accelerates(weight):
    rec = _records(np.random.default_rng(72), 5000)
    rec[:, 10:13] = 0.0
    rec[::2, 10:13] = -0.0
    want = accelerate(accelerate(rec, 7, weight, 0.37), 7, weight, 0.37)
    got = boris(rec, 7, 10, weight, 0.37)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_boris_without_e_keeps_the_speed():
    """(16 2^-52 relative bounds the model's own rounding: some twenty
    operations of half a unit each on the way from v to v'.)"""
    rng = np.random.default_rng(73)
    n = 200000
    rec = _records(rng, n)
    rec[:, 7:10] = 0.0
    b = rng.standard_normal((n, 3))
    b *= (10.0 ** rng.uniform(-3, np.log10(5.0), n) / np.linalg.norm(b, axis=1))[:, None]  # |t| from 1e-3 to 5
    rec[:, 10:13] = b
    out = boris(rec, 7, 10, None, 1.0)
    v0 = np.array([math.sqrt(math.fsum(x * x for x in r)) for r in rec[:, 3:6]])
    v1 = np.array([math.sqrt(math.fsum(x * x for x in r)) for r in out[:, 3:6]])
    worst = float(np.max(np.abs(v1 - v0) / v0))
    print("worst relative change of |v|:", worst / EPS, "units of 2^-52")
    assert worst <= 16 * EPS
    assert np.array_equal(out[:, 6:].view(np.uint64), rec[:, 6:].view(np.uint64))
    assert np.array_equal(out[:, 0:3].view(np.uint64), rec[:, 0:3].view(np.uint64))


def test_boris_rotates_by_twice_atan_of_h_b():
    rng = np.random.default_rng(74)
    n = 20000
    rec = _records(rng, n)
    rec[:, 7:10] = 0.0
    rec[:, 10:12] = 0.0
    rec[:, 12] = rng.uniform(-3, 3, n)
    rec[:, 6] = rng.uniform(0.5, 2, n)
    h = 0.4 * rec[:, 6]
    out = boris(rec, 7, 10, 6, 0.4)
    x0, y0, x1, y1 = rec[:, 3], rec[:, 4], out[:, 3], out[:, 4]
    # v' = v + v x s ...: a positive h B_z turns the velocity clockwise about z
    angle = np.arctan2(x1 * y0 - y1 * x0, x0 * x1 + y0 * y1)
    assert np.max(np.abs(angle - 2 * np.arctan(h * rec[:, 12]))) <= 1e-14
    assert np.array_equal(out[:, 5].view(np.uint64), rec[:, 5].view(np.uint64))  # v_z: v + 0


def test_entry_points_are_declared_and_exported():
    import dccrg_amd

    L = dccrg_amd.lib()
    syms = dccrg_amd.header_symbols()
    for name in ("dccrgx_particles_deposit_moments", "dccrgx_particles_boris"):
        assert name in syms, name
        assert hasattr(L, name), name
    assert L.dccrgx_particles_deposit_moments(None, 0, 10, 1, 6, None, None, 1, 0) == dccrg_amd._lib.EINVAL
    assert b"null grid" in L.dccrgx_last_error()
    assert L.dccrgx_particles_boris(None, 0, 13, 7, 10, 6, 0.5) == dccrg_amd._lib.EINVAL
    assert b"null grid" in L.dccrgx_last_error()
