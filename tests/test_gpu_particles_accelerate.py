"""dccrgx_particles_accelerate (particles_accelerate_kernel,
dccrg_amd/csrc/particles.hip): record[3 + j] += (factor q) record[first + j].

The header fixes the order (factor * q, the product with the field's double,
then the sum, each rounded on its own), so the result is bitwise the NumPy
expression's; every other double, and every record of a remote copy, keeps
its bits."""
import types

import numpy as np
import pytest

from test_gpu_particles import _local_cells, _same
from test_gpu_particles_deposit import ODD_L0, ODD_START, _pair, _seed, _upload_all

pytestmark = pytest.mark.gpu

K = 10
GRID = dict(length=(4, 4, 4), R=2, periodic=(True, False, True), rounds=2, frac=0.15)


def _case(nprocs=1, seed=61):
    """Seeded records (0..5 per cell, so some cells are empty) and one local
    cell with 300 of them: a block boundary falls inside that cell."""
    g, m, fld = _pair(start=ODD_START, l0=ODD_L0, K=K, nprocs=nprocs, **GRID)
    rng = np.random.default_rng(seed)
    _seed(m, rng, 5)
    big = int(g.slot_ids()[g.n_local // 2])
    ctr, ln = m.o.geometry([big])
    r = rng.random((300, K)) * 2 - 1
    r[:, 0:3] = (ctr[0] - ln[0] / 2) + ln[0] * rng.random((300, 3))
    m.set(big, r)
    _upload_all(g, fld, m)
    counts = [m.cells[int(c)].shape[0] for c in g.slot_ids()[: g.n_local]]
    assert 0 in counts and max(counts) > 256 and sum(counts) > 2 * 256
    return g, m, fld


def _expected(rec, first, weight, factor):
    out = rec.copy()
    factor = np.float64(factor)
    k = factor * rec[:, weight] if weight is not None else np.full(rec.shape[0], factor)
    for j in range(3):
        term = k * rec[:, first + j]
        out[:, 3 + j] = rec[:, 3 + j] + term
    return out


def _check(g, m, fld, first, weight, factor):
    nl, nr = g.n_local, g.n_slots - g.n_local
    remote = fld.get(nl, nr) if nr else []
    if weight == "default":
        g.particles_accelerate(fld, first, K, factor)
        weight = None
    else:
        g.particles_accelerate(fld, first, K, factor, weight)
    after = _local_cells(g, fld, K)
    assert sorted(after) == sorted(int(c) for c in g.slot_ids()[:nl])
    for c, a in after.items():
        want = _expected(m.cells[c], first, weight, factor)
        assert _same(a, want), (c, np.argwhere(a != want)[:5])  # the velocity and every other double
        m.set(c, a)
    for x, y in zip(remote, fld.get(nl, nr) if nr else []):
        assert _same(x, y)


def test_bitwise_on_a_refined_grid(gpu):
    g, m, fld = _case()
    _check(g, m, fld, 7, 6, 0.37)
    _check(g, m, fld, 6, 9, -1.25)   # the weight past the field's doubles
    _check(g, m, fld, 7, None, 0.1)  # q = 1
    _check(g, m, fld, 6, "default", 3.0)
    g.close()


def test_remote_copies_keep_their_records(gpu):
    g, m, fld = _case(nprocs=2)
    nl, nr = g.n_local, g.n_slots - g.n_local
    assert nr > 0 and int(fld.sizes(nl, nr).sum()) > 0
    _check(g, m, fld, 7, 6, 0.37)
    g.close()


def test_empty_pool(gpu):
    g, m, fld = _pair((3, 2, 2), K=K)
    g.particles_accelerate(fld, 7, K, 1.0, 6)
    _upload_all(g, fld, m)  # every cell sized to zero records
    g.particles_accelerate(fld, 7, K, 1.0, 6)
    assert int(fld.sizes().sum()) == 0
    g.close()


def test_refusals(gpu):
    from dccrg_amd._lib import EINVAL

    g, m, fld = _pair((4, 3, 2), K=K)
    rng = np.random.default_rng(62)
    for c in m.leaves:
        m.set(c, rng.random((2, K)))
    _upload_all(g, fld, m)
    fixed = g.add_field("rho", np.float64)
    calls = [(lambda: g.particles_accelerate(fixed, 7, K, 1.0, 6), "fixed-size"),
             (lambda: g.particles_accelerate(types.SimpleNamespace(id=99), 7, K, 1.0, 6), "invalid field id"),
             (lambda: g.particles_accelerate(fld, 7, 2, 1.0), "at least 3 doubles"),
             (lambda: g.particles_accelerate(fld, 6, 9, 1.0), "not a multiple of 8")]  # 20 doubles a cell
    calls += [(lambda first=first, k=k: g.particles_accelerate(fld, first, k, 1.0), "first_double")
              for first, k in ((5, K), (3, K), (0, K), (-1, K), (8, K), (6, 8), (6, 5))]
    calls += [(lambda w=w: g.particles_accelerate(fld, 6, K, 1.0, w), "weight_double")
              for w in (0, 3, 5, 6, 7, 8, 10, -2)]
    for call, match in calls:
        with pytest.raises(Exception, match=match) as e:
            call()
        assert e.value.code == EINVAL
    for c, a in _local_cells(g, fld, K).items():
        assert _same(a, m.cells[c])  # a refused call writes nothing
    g.particles_accelerate(fld, 6, K, 1.0, 9)
    g.close()
