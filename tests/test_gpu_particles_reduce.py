"""dccrgx_particles_reduce / dccrgx_particles_reduce_device
(particles_reduce_kernel, dccrg_amd/csrc/particles.hip, and reduce_fold_kernel)
against tests/reduce_model.py.

Both sides form bitwise equal terms (q u) v; only the order of a sum is the
kernel's, so a sum of k terms is held to gamma(k - 1) * sum |t_i| (see
test_gpu_field_reduce.py); extrema, empty results and sums over one record are
compared bitwise.  Records are random in [-1, 1) in every double: a reduction
locates nothing, so the positions need not lie in their cells."""
import ctypes as C
import math

import numpy as np
import pytest

import reduce_model as RM
from helpers import make_pair

pytestmark = pytest.mark.gpu

REFINED = dict(length=(4, 4, 4), R=2, periodic=(True, False, True), hood=1, rounds=2, frac=0.15)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def sixteen(K):
    """All four operations, -1 factors in either place, squares, repeats."""
    d = list(range(3, K))
    return [("sum", None, None), ("sum", 3, None), ("sum", 4, None), ("sum", 5, None), ("sum", 3, 3), ("sum", 4, 4),
            ("sum", 5, 5), ("max_abs", 3, None), ("max_abs", None, 4), ("min", 5, None), ("max", d[-1], None),
            ("min", 3, 4), ("max", d[-1], d[-2]), ("sum", None, d[-1]), ("max_abs", 5, 5), ("sum", d[-2], 3)]


class Case:
    """counts[s] random records of K doubles in slot s (remote copies
    included); the model sees the local cells' only."""

    def __init__(self, g, K, counts, seed=3):
        self.g, self.K = g, K
        rng = np.random.default_rng(seed)
        self.rec = [rng.random((int(n), K)) * 2 - 1 for n in counts]
        self.fld = g.add_variable_field("particles", np.float64, True)
        self.fld.set([r.reshape(-1) for r in self.rec])
        self.local = np.concatenate(self.rec[: g.n_local]) if g.n_local else np.zeros((0, K))

    def check(self, terms, weight):
        got = self.g.particles_reduce(self.fld, terms, self.K, weight)
        want = RM.particles_reduce(terms, self.local, -1 if weight is None else weight)
        assert got.shape == (len(terms),)
        worst = 0.0
        for t, x, r in zip(terms, got, want):
            if t[0] == "sum" and r.k > 1:
                err = r.error(x)
                worst = max(worst, err / r.bound)
                assert err <= r.bound, (t, weight, x, r.value, err, r.bound)
            else:
                assert _bits(x) == _bits(r.value), (t, weight, x, r.value)
        print(f"{len(terms)} terms over {self.local.shape[0]} records, weight {weight}: worst sum error "
              f"{worst:.4f} of its bound")
        return got

    def check_all(self):
        K = self.K
        for weight in (None, 6, K - 1):
            self.check(sixteen(K), weight)
        for t in sixteen(K)[:9:4] + [("min", None, None), ("max", 3, 3)]:
            self.check([t], 6)
        n = self.check([("sum", None, None)], None)[0]
        assert n == float(self.local.shape[0])


def _small(counts_first, K, nprocs=1, rank=0):
    g, _ = make_pair((4, 3, 2), 0, (False, False, False), 1, nprocs=nprocs, rank=rank)
    g.set_geometry((0, 0, 0), (1, 1, 1))
    rng = np.random.default_rng(7)
    counts = list(counts_first) + list(rng.integers(0, 4, g.n_slots))
    return g, counts[: g.n_slots]


@pytest.mark.parametrize("K", [7, 10])
def test_counts_that_straddle_a_wave(gpu, K):
    g, counts = _small([0, 1, 63, 64, 65, 0, 130, 2], K)
    c = Case(g, K, counts)
    assert c.local.shape[0] > 2 * 128  # more than two blocks of 128 records
    c.check_all()
    g.close()


@pytest.mark.parametrize("K", [7, 10])
def test_no_record_and_one_record(gpu, K):
    g, _ = _small([], K)
    empty = [(op, 3, None) for op in RM.OPS]
    # a field that was never set, then one whose cells are all empty
    fld = g.add_variable_field("never", np.float64, True)
    want = list(_bits([0.0, math.inf, -math.inf, 0.0]))
    assert list(_bits(g.particles_reduce(fld, empty, K, 6))) == want
    c = Case(g, K, [0] * g.n_slots)
    assert list(_bits(c.check(empty, None))) == want
    g.close()
    g, _ = _small([], K)
    counts = [0] * g.n_slots
    counts[5] = 1
    c = Case(g, K, counts)
    c.check_all()  # k == 1: every term bitwise
    g.close()


def test_refined_grid(gpu):
    r = REFINED
    g, _ = make_pair(r["length"], r["R"], r["periodic"], r["hood"], r["rounds"], r["frac"])
    g.set_geometry((0.1, -0.3, 0.2), (0.3, 0.7, 1.1))
    c = Case(g, 10, np.random.default_rng(5).integers(0, 9, g.n_slots))
    c.check_all()
    g.close()


@pytest.fixture(scope="module")
def views(gpu):
    cs = []
    for rank in (0, 1):
        r = REFINED
        g, _ = make_pair(r["length"], r["R"], r["periodic"], r["hood"], r["rounds"], r["frac"], nprocs=2, rank=rank)
        g.set_geometry((0.1, -0.3, 0.2), (0.3, 0.7, 1.1))
        assert g.n_slots > g.n_local
        # every remote copy holds records too: they must not be counted
        cs.append(Case(g, 7, np.random.default_rng(8 + rank).integers(1, 6, g.n_slots)))
    yield cs
    for c in cs:
        c.g.close()


def test_remote_copies_are_not_counted(views):
    for c in views:
        assert sum(r.shape[0] for r in c.rec) > c.local.shape[0] > 0
        c.check_all()


def test_determinism_and_the_two_forms(views):
    import torch

    c = views[0]
    g, K = c.g, c.K
    for weight in (None, 6):
        first = g.particles_reduce(c.fld, sixteen(K), K, weight)
        again = g.particles_reduce(c.fld, sixteen(K), K, weight)
        assert np.array_equal(_bits(first), _bits(again))
        t = torch.full((24,), -7.5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()  # (the library writes on its own stream)
        ret = g.particles_reduce(c.fld, sixteen(K), K, weight, out=t[4:20])
        assert ret.data_ptr() == t[4:20].data_ptr()
        g.synchronize()
        h = t.cpu().numpy()
        assert np.array_equal(_bits(h[4:20]), _bits(first)) and np.all(h[:4] == -7.5) and np.all(h[20:] == -7.5)


def test_refusals_leave_the_output_untouched(gpu):
    import torch

    from dccrg_amd._lib import EINVAL, lib

    g, counts = _small([3, 1, 2], 7)
    c = Case(g, 7, counts)
    fld, K = c.fld, 7
    fixed = g.add_field("fixed", np.float64)
    t = torch.full((16,), -7.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ok = [("sum", 3, None)]
    calls = [
        (lambda: g.particles_reduce(fld, [], K, out=t), "1 .. 16"),
        (lambda: g.particles_reduce(fld, ok * 17, K, out=torch.full((17,), -7.5, dtype=torch.float64, device="cuda")),
         "1 .. 16"),
        (lambda: g.particles_reduce(fld, [(4, 3, None)], K, out=t), "unknown reduction"),
        (lambda: g.particles_reduce(fld, [(-1, 3, None)], K, out=t), "unknown reduction"),
        (lambda: g.particles_reduce(fixed, ok, K, out=t), "variable-size"),
        (lambda: g.particles_reduce(fld, [("sum", None, None)], 2, out=t), "at least 3 doubles"),
        (lambda: g.particles_reduce(fld, ok, 10, out=t), "multiple of"),  # 7-double records read as 10
        (lambda: g.particles_reduce(fld, ok, K, 2, out=t), "weight_double"),
        (lambda: g.particles_reduce(fld, ok, K, K, out=t), "weight_double"),
        (lambda: g.particles_reduce(fld, [("sum", 2, None)], K, out=t), "factor"),
        (lambda: g.particles_reduce(fld, [("sum", 3, K)], K, out=t), "factor"),
        (lambda: g.particles_reduce(fld, [("sum", 3, -2)], K, out=t), "factor"),
    ]
    for call, match in calls:
        with pytest.raises(Exception, match=match) as e:
            call()
        assert e.value.code == EINVAL
    terms = (C.c_int * 3)(0, 3, -1)
    ptr = C.c_void_p(t.data_ptr())
    assert lib().dccrgx_particles_reduce_device(g.h, fld.id, K, -1, terms, 1, 0, None) == EINVAL
    assert lib().dccrgx_particles_reduce_device(g.h, fld.id, K, -1, None, 1, 0, ptr) == EINVAL
    assert lib().dccrgx_particles_reduce_device(g.h, 99, K, -1, terms, 1, 0, ptr) == EINVAL
    assert lib().dccrgx_particles_reduce(g.h, fld.id, K, -1, terms, 1, 0, None) == EINVAL
    host = np.full(16, -7.5)
    assert lib().dccrgx_particles_reduce(g.h, fld.id, K, 2, terms, 1, 0,
                                         host.ctypes.data_as(C.POINTER(C.c_double))) == EINVAL
    g.synchronize()
    assert np.all(t.cpu().numpy() == -7.5) and np.all(host == -7.5)
    # collective on a view of two processes that has no communicator
    v, vc = _small([2, 2], 7, nprocs=2, rank=1)
    cv = Case(v, 7, vc)
    with pytest.raises(Exception, match="communicator") as e:
        v.particles_reduce(cv.fld, ok, 7, collective=True, out=t)
    assert e.value.code == EINVAL
    v.synchronize()
    assert np.all(t.cpu().numpy() == -7.5)
    cv.check(ok, None)
    assert np.array_equal(_bits(g.particles_reduce(fld, ok, K, collective=True)), _bits(g.particles_reduce(fld, ok, K)))
    v.close()
    g.close()
