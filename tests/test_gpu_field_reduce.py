"""dccrgx_field_reduce / dccrgx_field_reduce_device (field_reduce_kernel and
reduce_fold_kernel, dccrg_amd/csrc/field_ops.hip) against
tests/reduce_model.py.

Both sides form bitwise equal terms (a * b, then * V for a sum by volume); only
the order of a sum is the kernel's.  A sum of k terms in any order and any
tree satisfies |got - exact| <= gamma(k - 1) * sum |t_i| with gamma(m) =
m u / (1 - m u), u = 2^-53 (additions of the identity are exact), which is the
tolerance; the model gives exact (fsum) and the sum of magnitudes.  Extrema,
empty results and sums over a single cell are compared bitwise.  A miss is a
bug, not noise.

The kernel takes two cells a thread as 16-byte loads when a call names at most
16 distinct fields and one cell a thread above that: MANY names 20, FEW 6."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import gradient_model as GM
import poisson_stretched_model as PM
import reduce_model as RM
import stretched_solver_cases as SC
from helpers import make_pair

pytestmark = pytest.mark.gpu

ODD_START, ODD_L0 = (0.1, -0.3, 0.2), (0.3, 0.7, 1.1)  # the gradient tests'
REFINED = dict(length=(4, 4, 4), R=2, periodic=(True, False, True), hood=1, rounds=2, frac=0.15)
REMOTE = 1e300  # in every remote-copy slot: must never be read
NF = 20

# (op, a, b): indices into the case's fields, None for 1.0
FEW = [("sum", 0, 0), ("sum", 1, 1), ("sum", 2, 2), ("sum", 3, 3), ("sum", 4, 4), ("sum", 5, 5), ("max_abs", 0, None),
       ("min", 1, None), ("max", None, 2), ("sum", 0, 1), ("min", 2, 3), ("max", 4, 5), ("max_abs", 3, 4),
       ("sum", None, None), ("sum", 5, None), ("max", 0, 0)]
MANY = [("sum", 0, 1), ("min", 2, 3), ("max", 4, 5), ("max_abs", 6, 7), ("sum", 8, 8), ("sum", 9, None),
        ("max_abs", None, 10), ("min", 11, 12), ("sum", 13, 14), ("max", 15, None), ("sum", 16, 17), ("min", 18, 19),
        ("sum", 19, 0), ("max_abs", 1, 1), ("sum", None, None), ("max", 7, 13)]
assert len(FEW) == len(MANY) == 16 and len({x for t in MANY for x in t[1:]} - {None}) == 20


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Case:
    """A grid (or a detached view), NF fields random in [-1, 1) in every local
    slot and REMOTE in the remote copies, and the model's volumes."""

    def __init__(self, g, o, volumes, seed=1, nf=NF):
        self.g = g
        self.ids = np.sort(o.cells()[0])
        self.at = np.searchsorted(self.ids, g.slot_ids())
        self.V = volumes(self.ids)
        rng = np.random.default_rng(seed)
        self.F = [rng.random(self.ids.size) * 2 - 1 for _ in range(nf)]
        self.f = [g.add_field(f"F{j}", np.float64) for j in range(nf)]
        for f, v in zip(self.f, self.F):
            self.put(f, v)

    def put(self, f, whole):
        v = np.asarray(whole, np.float64)[self.at]
        v[self.g.n_local:] = REMOTE
        f.set(v)

    def span(self, region):
        ni, nl = self.g.counts["inner"], self.g.n_local
        return {"all": (0, nl), "inner": (0, ni), "outer": (ni, nl)}[region]

    def check(self, terms, by_volume=False, region="all", F=None):
        """One call against the model over the region's cells; returns the results."""
        F = F or self.F
        lo, hi = self.span(region)
        sel = self.at[lo:hi]
        got = self.g.field_reduce([(op, None if a is None else self.f[a], None if b is None else self.f[b])
                                   for op, a, b in terms], by_volume, region)
        want = RM.field_reduce([(op, None if a is None else F[a][sel], None if b is None else F[b][sel])
                                for op, a, b in terms], hi - lo, self.V[sel] if by_volume else None)
        assert got.shape == (len(terms),)
        worst = 0.0
        for t, x, r in zip(terms, got, want):
            if t[0] == "sum" and r.k > 1:
                err = r.error(x)
                worst = max(worst, err / r.bound)
                assert err <= r.bound, (t, by_volume, region, x, r.value, err, r.bound)
            else:
                assert _bits(x) == _bits(r.value), (t, by_volume, region, x, r.value)
        print(f"{len(terms)} terms over {hi - lo} cells, by_volume={by_volume}, {region}: worst sum error "
              f"{worst:.4f} of its bound")
        return got


def _cartesian_volumes(length, R):
    return lambda ids: RM.volumes(GM.cartesian_lengths(ODD_L0, GM.levels(ids, length, R)))


def _uniform(length, seed=1, nf=NF):
    g, o = make_pair(length, 0, (False, False, False), 1)
    g.set_geometry(ODD_START, ODD_L0)
    return Case(g, o, _cartesian_volumes(length, 0), seed, nf)


def _refined(seed=0, nprocs=1, rank=0, nf=NF):
    c = REFINED
    g, o = make_pair(c["length"], c["R"], c["periodic"], c["hood"], c["rounds"], c["frac"], seed=seed, nprocs=nprocs,
                     rank=rank)
    g.set_geometry(ODD_START, ODD_L0)
    return Case(g, o, _cartesian_volumes(c["length"], c["R"]), seed + 10, nf)


def _stretched(only_block, nf=6):
    from oracle import oracle as O

    length, R = (4, 4, 4), 1
    coords = SC.uneven_coords(length, 21)
    g, o = make_pair(length, R, (True, False, True), 1, 1, 0.15)
    if only_block:
        g.set_geometry([c[0] for c in coords], [c[1] - c[0] for c in coords])
        g.set_geometry_block(O.stretched_geometry_block(coords))
        return Case(g, o, lambda ids: RM.volumes(PM.fallback_lengths(coords, GM.levels(ids, length, R))), 5, nf)
    g.set_stretched_geometry(coords)
    return Case(g, o, lambda ids: RM.volumes(GM.stretched_lengths(coords, length, R, ids)), 5, nf)


SIZES = {(1, 1, 1): 1, (4, 3, 2): 24, (9, 7, 5): 315, (32, 32, 17): 17408}


@pytest.mark.parametrize("length", list(SIZES))
def test_uniform_sizes(gpu, length):
    c = _uniform(length)
    assert c.g.n_local == SIZES[length]
    for by_volume in (False, True):
        c.check(FEW, by_volume)
        c.check(MANY, by_volume)
    # single terms, each op, products, single fields and -1 factors on their own
    for t in [("sum", 0, 1), ("min", 0, 1), ("max", 0, 1), ("max_abs", 0, 1), ("sum", 2, None), ("max_abs", None, 2),
              ("sum", None, None), ("min", None, None), ("max", 3, 3)]:
        c.check([t])
    # 16 distinct fields are the most that go two cells a thread (64 KB of LDS), 17 the fewest that go one
    c.check([("sum", 2 * j, 2 * j + 1) for j in range(8)], True)
    c.check([("sum", 2 * j, 2 * j + 1) for j in range(8)] + [("max_abs", 16, None)], True)
    # one field in every term
    c.check([("sum", 7, 7), ("min", 7, None), ("max", None, 7), ("max_abs", 7, 7), ("sum", 7, None)], True)
    assert float(c.check([("sum", None, None)])[0]) == float(SIZES[length])
    c.g.close()


def test_refined_grid_by_volume(gpu):
    c = _refined()
    g = c.g
    assert set(GM.levels(c.ids, REFINED["length"], REFINED["R"]).tolist()) == {0, 1, 2}
    for by_volume in (False, True):
        c.check(FEW, by_volume)
        c.check(MANY, by_volume)
    # the domain's volume, and the number of cells
    n = g.n_local
    vol = g.field_reduce([("sum", None, None)], True)[0]
    domain = math.prod(4 * l for l in ODD_L0)
    # (every V_c carries the two roundings of its products, `domain` two more: 4 u, with the
    # second-order terms 5 u)
    assert abs(vol - domain) <= RM.gamma(n - 1) * domain + 5 * RM.U * domain
    r = RM.field_reduce([("sum", None, None)], n, c.V[c.at[:n]])[0]
    assert r.error(vol) <= r.bound
    cnt = g.field_reduce([("sum", None, None)], False)[0]
    assert cnt == float(n) and n == c.ids.size
    g.close()


def test_stretched_geometry_by_volume(gpu):
    c = _stretched(False)
    for by_volume in (False, True):
        c.check(FEW, by_volume)
    c.g.close()


def test_file_block_without_coordinates(gpu):
    from dccrg_amd._lib import EINVAL

    c = _stretched(True)
    c.check(FEW, False)
    with pytest.raises(Exception, match="stretched geometry block") as e:
        c.g.field_reduce([("sum", c.f[0], None)], True)
    assert e.value.code == EINVAL
    c.g.close()


@pytest.fixture(scope="module")
def views(gpu):
    cs = [_refined(0, 2, rank) for rank in (0, 1)]
    yield cs
    for c in cs:
        c.g.close()


def test_regions_on_detached_views(views):
    assert not np.intersect1d(views[0].at[:views[0].g.n_local], views[1].at[:views[1].g.n_local]).size
    ext = []
    for c in views:
        g = c.g
        ni, nl = g.counts["inner"], g.n_local
        assert g.n_slots > nl and 0 < ni < nl
        for region in ("inner", "outer", "all"):
            for by_volume in (False, True):
                c.check(FEW, by_volume, region)
            c.check(MANY, True, region)
        ext.append(c.check([("min", 0, 1), ("max", 0, 1), ("max_abs", 0, 1)]))
    whole = RM.field_reduce([(op, views[0].F[0], views[0].F[1]) for op in ("min", "max", "max_abs")],
                            views[0].ids.size)
    assert _bits(min(ext[0][0], ext[1][0])) == _bits(whole[0].value)
    assert _bits(max(ext[0][1], ext[1][1])) == _bits(whole[1].value)
    assert _bits(max(ext[0][2], ext[1][2])) == _bits(whole[2].value)


def test_outer_of_one_process_is_empty(gpu):
    c = _uniform((4, 3, 2), nf=2)
    got = c.g.field_reduce([("sum", c.f[0], c.f[1]), ("min", c.f[0], None), ("max", c.f[0], None),
                            ("max_abs", c.f[0], None)], True, "outer")
    assert list(_bits(got)) == list(_bits([0.0, math.inf, -math.inf, 0.0]))
    c.g.close()


def test_determinism_and_the_two_forms(views):
    import torch

    c = views[1]
    g = c.g
    terms = [(op, None if a is None else c.f[a], None if b is None else c.f[b]) for op, a, b in FEW]
    for by_volume in (False, True):
        for region in ("all", "outer"):
            first = g.field_reduce(terms, by_volume, region)
            again = g.field_reduce(terms, by_volume, region)
            assert np.array_equal(_bits(first), _bits(again))
            t = torch.full((24,), -7.5, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()  # (the library writes on its own stream)
            ret = g.field_reduce(terms, by_volume, region, out=t[4:20])
            assert ret.data_ptr() == t[4:20].data_ptr()
            g.synchronize()
            h = t.cpu().numpy()
            assert np.array_equal(_bits(h[4:20]), _bits(first)) and np.all(h[:4] == -7.5) and np.all(h[20:] == -7.5)


def test_large_dynamic_range(gpu):
    c = _uniform((9, 7, 5), nf=2)
    ones = np.ones(c.ids.size)
    big = ones.copy()
    big[c.at[200]] = 1e16
    c.put(c.f[0], big)
    c.put(c.f[1], ones)
    F = [big, ones]
    got = c.check([("sum", 0, None), ("sum", 0, 1), ("min", 0, None), ("max", 0, None), ("max_abs", 0, 1),
                   ("sum", 1, None)], F=F)
    assert got[3] == 1e16 and got[2] == 1.0 and got[5] == 315.0
    c.g.close()


def test_refusals_leave_the_output_untouched(gpu):
    import torch

    from dccrg_amd._lib import EINVAL, lib

    c = _uniform((4, 3, 2), nf=2)
    g = c.g
    u32 = g.add_field("u32", np.uint32)
    var = g.add_variable_field("var", np.float64, False)
    bad, neg = types.SimpleNamespace(id=99), types.SimpleNamespace(id=-2)
    f0, f1 = c.f
    t = torch.full((16,), -7.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    calls = [
        (lambda: g.field_reduce([], out=t), "1 .. 16"),
        (lambda: g.field_reduce([("sum", f0, f1)] * 17, out=torch.full((17,), -7.5, dtype=torch.float64,
                                                                       device="cuda")), "1 .. 16"),
        (lambda: g.field_reduce([(4, f0, f1)], out=t), "unknown reduction"),
        (lambda: g.field_reduce([("sum", f0, None), (-1, f0, f1)], out=t), "unknown reduction"),
        (lambda: g.field_reduce([("sum", var, None)], out=t), "variable-size"),
        (lambda: g.field_reduce([("sum", f0, u32)], out=t), "8-byte"),
        (lambda: g.field_reduce([("max", bad, None)], out=t), "field"),
        (lambda: g.field_reduce([("max", f0, neg)], out=t), "field"),
    ]
    for call, match in calls:
        with pytest.raises(Exception, match=match) as e:
            call()
        assert e.value.code == EINVAL
    terms = (C.c_int * 3)(0, f0.id, f1.id)
    ptr = C.c_void_p(t.data_ptr())
    for region in (-1, 3):
        assert lib().dccrgx_field_reduce_device(g.h, terms, 1, 0, region, 0, ptr) == EINVAL
    assert lib().dccrgx_field_reduce_device(g.h, terms, 1, 0, 0, 0, None) == EINVAL
    assert lib().dccrgx_field_reduce_device(g.h, None, 1, 0, 0, 0, ptr) == EINVAL
    assert lib().dccrgx_field_reduce(g.h, terms, 1, 0, 0, 0, None) == EINVAL
    host = np.full(16, -7.5)
    hp = host.ctypes.data_as(C.POINTER(C.c_double))
    assert lib().dccrgx_field_reduce(g.h, terms, 0, 0, 0, 0, hp) == EINVAL
    assert lib().dccrgx_field_reduce(g.h, terms, 1, 0, 7, 0, hp) == EINVAL
    g.synchronize()
    assert np.all(t.cpu().numpy() == -7.5) and np.all(host == -7.5)
    # collective on a view of two processes that has no communicator; alone it works
    v, _ = make_pair((4, 3, 2), 0, (False, False, False), 1, nprocs=2, rank=0)
    fv = v.add_field("x", np.float64)
    fv.set(np.full(v.n_slots, 0.5))
    with pytest.raises(Exception, match="communicator") as e:
        v.field_reduce([("sum", fv, None)], collective=True, out=t)
    assert e.value.code == EINVAL
    v.synchronize()
    assert np.all(t.cpu().numpy() == -7.5)
    assert v.field_reduce([("sum", fv, None)])[0] == 0.5 * v.n_local
    assert g.field_reduce([("sum", f0, None)], collective=True)[0] == g.field_reduce([("sum", f0, None)])[0]
    v.close()
    g.close()
