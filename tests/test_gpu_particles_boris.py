"""dccrgx_particles_boris (particles_boris_kernel, dccrg_amd/csrc/particles.hip)
against the NumPy restatement in tests/moments_model.py.

The header fixes every operation and its order, so the records are bitwise
the model's; every other double, and every record of a remote copy, keeps its
bits.  With B = 0 the kick is two particles_accelerate calls to the bit."""
import types

import numpy as np
import pytest

from moments_model import boris
from test_gpu_particles import REFINED, _local_cells, _same
from test_gpu_particles_deposit import ODD_L0, ODD_START, _pair, _seed, _upload_all

pytestmark = pytest.mark.gpu

K = 13  # x, v, q, E, B


def _case(nprocs=1, seed=91, zero_b=False):
    """Seeded records (0..5 per cell, so some cells are empty) and one local
    cell with 300 of them: a block boundary falls inside that cell."""
    g, m, fld = _pair(start=ODD_START, l0=ODD_L0, K=K, nprocs=nprocs, **REFINED)
    rng = np.random.default_rng(seed)
    _seed(m, rng, 5)
    big = int(g.slot_ids()[g.n_local // 2])
    ctr, ln = m.o.geometry([big])
    r = rng.random((300, K)) * 2 - 1
    r[:, 0:3] = (ctr[0] - ln[0] / 2) + ln[0] * rng.random((300, 3))
    m.set(big, r)
    if zero_b:
        for rec in m.cells.values():
            rec[:, 10:13] = 0.0
    _upload_all(g, fld, m)
    counts = [m.cells[int(c)].shape[0] for c in g.slot_ids()[: g.n_local]]
    assert 0 in counts and max(counts) > 256 and sum(counts) > 2 * 256
    return g, m, fld


def _check(g, m, fld, e_first, b_first, weight, factor):
    nl, nr = g.n_local, g.n_slots - g.n_local
    remote = fld.get(nl, nr) if nr else []
    if weight == "default":
        g.particles_boris(fld, e_first, b_first, K, factor)
        weight = None
    else:
        g.particles_boris(fld, e_first, b_first, K, factor, weight)
    after = _local_cells(g, fld, K)
    assert sorted(after) == sorted(int(c) for c in g.slot_ids()[:nl])
    changed = 0
    for c, a in after.items():
        want = boris(m.cells[c], e_first, b_first, weight, factor)
        assert _same(a, want), (c, np.argwhere(a != want)[:5])  # the velocity and every other double
        changed += int(np.any(a[:, 3:6] != m.cells[c][:, 3:6]))
        m.set(c, a)
    assert changed > 0
    for x, y in zip(remote, fld.get(nl, nr) if nr else []):
        assert _same(x, y)


def test_bitwise_on_a_refined_grid(gpu):
    g, m, fld = _case()
    _check(g, m, fld, 7, 10, 6, 0.37)
    _check(g, m, fld, 10, 7, 6, -1.25)   # B before E in the record
    _check(g, m, fld, 6, 9, 12, 2.5)     # the weight past both, a strong rotation
    _check(g, m, fld, 7, 10, None, 0.1)  # q = 1
    _check(g, m, fld, 6, 10, "default", 3.0)
    g.close()


def test_remote_copies_keep_their_records(gpu):
    g, m, fld = _case(nprocs=2)
    nl, nr = g.n_local, g.n_slots - g.n_local
    assert nr > 0 and int(fld.sizes(nl, nr).sum()) > 0
    _check(g, m, fld, 7, 10, 6, 0.37)
    _check(g, m, fld, 7, 10, None, 0.37)
    g.close()


@pytest.mark.parametrize("weight", [6, None])
def test_zero_b_is_two_accelerate_calls(gpu, weight):
    """B gathered as zeros: the rotation adds exact zeros, so the kick is
    v + hE + hE, what two particles_accelerate calls leave in a second pool."""
    g, m, fld = _case(seed=92, zero_b=True)
    twin = g.add_variable_field("twin", np.float64, True)
    _upload_all(g, twin, m)
    g.particles_boris(fld, 7, 10, K, 0.37, weight)
    for _ in range(2):
        g.particles_accelerate(twin, 7, K, 0.37, weight)
    a, b = _local_cells(g, fld, K), _local_cells(g, twin, K)
    moved = 0
    for c in a:
        assert _same(a[c], b[c]), c
        moved += int(np.any(a[c][:, 3:6] != m.cells[c][:, 3:6]))
    assert moved > 0
    g.close()


def test_empty_pool(gpu):
    g, m, fld = _pair((3, 2, 2), K=K)
    g.particles_boris(fld, 7, 10, K, 1.0, 6)
    _upload_all(g, fld, m)  # every cell sized to zero records
    g.particles_boris(fld, 7, 10, K, 1.0, 6)
    assert int(fld.sizes().sum()) == 0
    g.close()


def test_refusals(gpu):
    from dccrg_amd._lib import EINVAL

    g, m, fld = _pair((4, 3, 2), K=K)
    rng = np.random.default_rng(93)
    for c in m.leaves:
        m.set(c, rng.random((2, K)))
    _upload_all(g, fld, m)
    fixed = g.add_field("rho", np.float64)
    calls = [(lambda: g.particles_boris(fixed, 7, 10, K, 1.0, 6), "fixed-size"),
             (lambda: g.particles_boris(types.SimpleNamespace(id=99), 7, 10, K, 1.0, 6), "invalid field id"),
             (lambda: g.particles_boris(fld, 7, 10, 2, 1.0), "at least 3 doubles"),
             (lambda: g.particles_boris(fld, 6, 9, 12, 1.0), "not a multiple of 8")]  # 26 doubles a cell
    calls += [(lambda e=e, k=k: g.particles_boris(fld, e, 10, k, 1.0), "e_first")
              for e, k in ((5, K), (3, K), (0, K), (-1, K), (11, K), (13, K))]
    calls += [(lambda b=b, k=k: g.particles_boris(fld, 6, b, k, 1.0), "b_first")
              for b, k in ((5, K), (3, K), (-1, K), (11, K), (9, 11))]
    calls += [(lambda e=e, b=b: g.particles_boris(fld, e, b, K, 1.0), "overlap")
              for e, b in ((7, 7), (7, 9), (9, 7), (8, 10), (10, 8))]
    calls += [(lambda w=w: g.particles_boris(fld, 7, 10, K, 1.0, w), "weight_double")
              for w in (0, 3, 5, 7, 9, 10, 12, 13, -2)]
    for call, match in calls:
        with pytest.raises(Exception, match=match) as e:
            call()
        assert e.value.code == EINVAL, match
    for c, a in _local_cells(g, fld, K).items():
        assert _same(a, m.cells[c])  # a refused call writes nothing
    g.particles_boris(fld, 6, 9, K, 1.0, 12)
    g.close()
