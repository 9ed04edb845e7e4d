"""Fixed fp64 cell fields follow the mesh through stop_refining
(Dccrg.field_follow_mesh, dccrg_amd/csrc/field_adapt.hip) against the model
of tests/field_adapt_model.py, which test_field_adapt_model_cpu.py pins.

Everything is compared per cell id, bitwise.  The derivative D the model takes
is the product's own gradient(scale=1) output on the old mesh just before the
adapt; where no group of four finer cells took part in a refined parent's
derivative it is also bitwise gradient_model's, so those children are checked
against a model that shares nothing with the product.

The multi-process scenarios (sc_*) run in spawned processes through
test_gpu_transport._run_group."""
import numpy as np
import pytest

import field_adapt_model as FM
import gradient_model as GM
import reduce_model as RM
from helpers import make_pair, random_refines

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ODD_START, ODD_L0 = (0.1, -0.3, 0.2), (0.3, 0.7, 1.1)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _vals(ids, salt):
    """A double in [-1, 1) from the id alone (splitmix64)."""
    z = (np.asarray(ids, np.uint64) ^ np.uint64(0x5DEECE66D + 977 * salt)) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / 2.0 ** 52 - 1.0


class Pair:
    """The product grid, the oracle grid, the fields {name: (field, mode)} and
    the three gradient outputs; lengths(ids) gives the (n, 3) lengths of
    dccrgx_gradient's contract."""

    def __init__(self, g, o, base, R, periodic, lengths, modes, seed=7):
        self.g, self.o, self.base, self.R, self.periodic, self.lengths = g, o, base, R, periodic, lengths
        self.grad = [g.add_field(n, np.float64, False) for n in ("gx", "gy", "gz")]
        self.fields = {}
        rng = np.random.default_rng(seed)
        for name, mode in modes.items():
            f = g.add_field(name, np.float64)
            f.set(rng.random(g.n_slots) * 2 - 1)
            g.field_follow_mesh(f, mode)
            self.fields[name] = (f, mode)

    def by_id(self, f):
        """(sorted local ids, the field's values in that order)"""
        nl = self.g.n_local
        sl = self.g.slot_ids()[:nl]
        order = np.argsort(sl)
        return sl[order], f.get(0, nl)[order]

    def adapt(self, refine=(), unrefine=(), check_gm=True):
        """The same requests to the product and to the oracle, stop_refining
        on both, every field against the model.  Returns counts."""
        g, o = self.g, self.o
        old = np.sort(o.cells()[0])
        vals, D = {}, {}
        for name, (f, mode) in self.fields.items():
            ids, vals[name] = self.by_id(f)
            assert np.array_equal(ids, old)
            if mode == "linear":
                g.gradient(f, self.grad, 1.0)
                D[name] = np.stack([self.by_id(x)[1] for x in self.grad], axis=1)
        for c in refine:
            assert g.refine_completely(int(c))
            o.refine_completely(int(c))
        for c in unrefine:
            assert g.unrefine_completely(int(c)) == o.unrefine_completely(int(c))
        g.stop_refining()
        o.stop_refining()
        new = np.sort(o.cells()[0])
        L = self.lengths(old)
        st = dict(children=0, parents=0, limited=0, finer=0, pure=0)
        for name, (f, mode) in self.fields.items():
            ids, got = self.by_id(f)
            assert np.array_equal(ids, new)
            F = FM.follow(old, new, self.base, self.R, self.periodic, L, vals[name], D.get(name), mode)
            bad = np.flatnonzero(got.view(np.uint64) != F.values.view(np.uint64))
            assert bad.size == 0, (name, mode, new[bad][:5], F.kind[bad][:5], got[bad][:5], F.values[bad][:5])
            st["children"], st["parents"] = int((F.kind == 1).sum()), int((F.kind == 2).sum())
            if mode == "linear" and F.limiter:
                st["limited"] += sum(1 for x in F.limiter.values() if x[4] < 1.0)
                if check_gm:
                    G = GM.gradient(old, self.base, self.R, self.periodic, L, vals[name])
                    for p in F.limiter:
                        i = int(np.searchsorted(old, np.uint64(p)))
                        if G.finer[i].any():
                            st["finer"] += 1
                        else:
                            st["pure"] += 1
                            assert _same(D[name][i], G.grad[i]), (name, p)
        return st


def _cartesian(base, R, periodic, modes, rounds=0, frac=0.15, seed=0, hood=1):
    g, o = make_pair(base, R, periodic, hood, rounds, frac, seed=seed)
    g.set_geometry(ODD_START, ODD_L0)
    return Pair(g, o, base, R, periodic, lambda ids: GM.cartesian_lengths(ODD_L0, GM.levels(ids, base, R)), modes)


ALL_MODES = {"off": None, "mean": "mean", "sum": "sum", "lin": "linear"}


def test_small_open_grid_all_modes(gpu):
    """2 x 2 x 2, R = 2, no periodic dimension: every cell has an open side.
    Four level-0 cells refined at once, then one child (the cells beside it
    are refined with it), then everything merged back."""
    P = _cartesian((2, 2, 2), 2, (False, False, False), ALL_MODES)
    st = P.adapt(refine=(1, 4, 6, 8))
    assert st["children"] == 32 and st["pure"] == 4
    kids = P.o.mapping.batch(P.o.mapping.batch([1])["child"])["siblings"][0]
    st = P.adapt(refine=(int(kids[7]),))
    assert st["children"] > 8  # induced refines
    for _ in range(3):
        ids = np.sort(P.o.cells()[0])
        lv = P.o.mapping.batch(ids)["level"]
        if lv.max() == 0:
            break
        st = P.adapt(unrefine=[int(c) for c in ids[lv == lv.max()]])
        assert st["parents"] > 0
    assert np.sort(P.o.cells()[0]).size == 8
    P.g.close()


def test_refined_periodic_grid_mixed_fields(gpu):
    """4 x 4 x 4 periodic, R = 2, level jumps on both sides and finer faces:
    five following fields of mixed modes and one that does not follow, whose
    bits are what they always were (a child a copy, a merged parent zero)."""
    modes = {"control": None, "lin_a": "linear", "sum": "sum", "mean": "mean", "lin_b": "linear", "mean_b": "mean"}
    P = _cartesian((4, 4, 4), 2, (True, True, True), modes, rounds=2, seed=3)
    rng = np.random.default_rng(11)
    tot = dict(children=0, parents=0, limited=0, finer=0, pure=0)
    for rnd in range(2):
        ids = np.sort(P.o.cells()[0])
        lv = P.o.mapping.batch(ids)["level"]
        ref = random_refines(ids, lv, 2, rng, 0.1)
        cand = np.setdiff1d(ids[lv > 0], np.array(ref, np.uint64))
        unref = [int(c) for c in rng.choice(cand, min(120, cand.size), replace=False)]
        st = P.adapt(ref, unref)
        for k in tot:
            tot[k] += st[k]
    print(tot)
    assert tot["children"] > 50 and tot["parents"] > 5 and tot["limited"] > 5 and tot["finer"] > 0 and tot["pure"] > 0
    P.g.close()


def test_a_cell_that_is_its_own_neighbor(gpu):
    """1 x 1 x 4 periodic: D is 0 in x and y, so only t_2 is not zero."""
    P = _cartesian((1, 1, 4), 1, (True, True, True), {"lin": "linear", "sum": "sum"})
    f = P.fields["lin"][0]
    by_cell = np.array([0.0, 1.0, 2.5, 1.0])  # cell 2: neither a minimum nor a maximum
    f.set(by_cell[P.g.slot_ids().astype(np.int64) - 1])
    P.g.gradient(f, P.grad, 1.0)
    assert np.all(P.grad[0].get(0, 4) == 0) and np.all(P.grad[1].get(0, 4) == 0) and np.any(P.grad[2].get(0, 4) != 0)
    st = P.adapt(refine=(2,))
    assert st["children"] == 8 and st["pure"] == 1
    ids, v = P.by_id(f)
    kids = v[ids > 4]
    assert np.unique(kids).size == 2 and kids.min() < 1.0 < kids.max()
    st = P.adapt(unrefine=(int(ids[-1]),))
    assert st["parents"] == 1
    P.g.close()


def test_512_parents_and_the_sum_round_trip(gpu):
    """8 x 8 x 8 all refined, then all merged: more than one block and several
    waves of parents.  SUM after SUM restores integer-valued doubles exactly."""
    P = _cartesian((8, 8, 8), 1, (True, False, True), {"sum": "sum", "lin": "linear", "mean": "mean"})
    f = P.fields["sum"][0]
    ints = np.random.default_rng(5).integers(-1000, 1000, 512).astype(np.float64)
    f.set(ints)
    sl0 = P.g.slot_ids()[:512].copy()
    st = P.adapt(refine=range(1, 513), check_gm=False)
    assert st["children"] == 4096 and st["limited"] > 100
    st = P.adapt(unrefine=[int(c) for c in P.o.mapping.batch(np.arange(1, 513))["child"]], check_gm=False)
    assert st["parents"] == 512
    ids, v = P.by_id(f)
    assert _same(v, ints[np.argsort(sl0)])
    P.g.close()


def test_stretched_geometry(gpu):
    """The 'rounded' case of test_gpu_stretched (R = 3): the lengths come from
    the coordinates."""
    import stretched_model as SM
    from test_gpu_stretched import _pair as stretched_pair

    g, m, _, coords, R = stretched_pair("rounded")
    base, per = SM.LENGTH, SM.PERIODIC
    P = Pair(g, m.o, base, R, per, lambda ids: GM.stretched_lengths(coords, base, R, ids),
             {"lin": "linear", "mean": "mean", "sum": "sum"})
    rng = np.random.default_rng(44)
    ids = np.sort(m.o.cells()[0])
    lv = m.o.mapping.batch(ids)["level"]
    st = P.adapt(random_refines(ids, lv, R, rng, 0.15))
    assert st["children"] > 50 and st["limited"] > 0
    ids = np.sort(m.o.cells()[0])
    lv = m.o.mapping.batch(ids)["level"]
    fine = ids[lv > 0]
    st = P.adapt((), [int(c) for c in rng.choice(fine, min(200, fine.size), replace=False)])
    assert st["parents"] > 0
    g.close()


def test_a_non_negative_field_stays_non_negative_and_its_integral(gpu):
    """Isolated spikes on a background with zeros, LINEAR.  Every child is
    >= -8 * 2^-53 * max M (the header's bound on leaving [m, M]).  The
    integral: both reductions err by at most the model's gamma(k - 1) S; the
    products t * V add 2^-53 S on each side; a refined parent's children miss
    its value in the mean by at most 16 * 2^-53 (|v| + Delta), times its
    volume.  Nothing merges, so nothing else changes."""
    base, R, per = (4, 4, 4), 2, (True, True, True)
    P = _cartesian(base, R, per, {"rho": "linear"}, rounds=1, seed=2)
    g, f = P.g, P.fields["rho"][0]
    rng = np.random.default_rng(21)
    ids = np.sort(P.o.cells()[0])
    v = rng.random(ids.size) * 1e-3
    v[rng.random(ids.size) < 0.3] = 0.0
    v[rng.choice(ids.size, 12, replace=False)] = 5.0 + rng.random(12)
    f.set(v[np.searchsorted(ids, g.slot_ids())])
    before = float(g.field_reduce([("sum", f, None)], by_volume=True)[0])
    Lb = P.lengths(ids)
    Rb = RM.field_reduce([("sum", v, None)], ids.size, RM.volumes(Lb))[0]
    lv = P.o.mapping.batch(ids)["level"]
    ref = random_refines(ids, lv, R, rng, 0.3)
    g.gradient(f, P.grad, 1.0)
    D = np.stack([P.by_id(x)[1] for x in P.grad], axis=1)
    st = P.adapt(ref)
    assert st["limited"] > 10 and st["parents"] == 0
    new, w = P.by_id(f)
    assert w.min() >= -8 * U * v.max()
    after = float(g.field_reduce([("sum", f, None)], by_volume=True)[0])
    Ra = RM.field_reduce([("sum", w, None)], new.size, RM.volumes(P.lengths(new)))[0]
    F = FM.follow(ids, new, base, R, per, Lb, v, D, "linear")
    vol = dict(zip(ids.tolist(), RM.volumes(Lb).tolist()))
    slack = sum(16 * U * (abs(x[0]) + x[3]) * vol[p] for p, x in F.limiter.items())
    bound = Rb.bound + Ra.bound + U * (Rb.S + Ra.S) + slack
    print(f"integral {before!r} -> {after!r}, |diff| {abs(after - before):.3e}, bound {bound:.3e}")
    assert abs(after - before) <= bound
    g.close()


def test_advection_adapt_keeps_its_density_rule(gpu):
    """advection_adapt's density is bitwise what it is on a grid where nothing
    follows, whatever mode it is given; an eighth field that follows as MEAN
    and holds a copy of the density has the density's bits after the adapt,
    merged parents and new children included."""
    from test_gpu_advection import gpu_grid, prerefine

    base, R = (10, 10, 3), 2
    A, fa = gpu_grid(base, R)
    B, fb = gpu_grid(base, R)
    copy = A.add_field("copy", np.float64, False)
    prerefine(A, fa, R)
    prerefine(B, fb, R)
    A.field_follow_mesh(copy, "mean")
    A.field_follow_mesh(fa[0], "linear")
    A.field_follow_mesh(fa[1], "sum")  # a reset field: not touched either
    di = 0.025 / R
    created = removed = 0
    for step in range(10):
        dt = 0.5 * A.advection_max_time_step(fa)
        out = []
        for g, f in ((A, fa), (B, fb)):
            g.advection_step(f, dt)
            g.advection_check_adaptation(f[0], di)
            g.advection_commit(f[0])
            if g is A:
                copy.set(f[0].get())
            out.append(g.advection_adapt(f))
        assert out[0] == out[1], step
        created += out[0][0]
        removed += out[0][1]
        nl = A.n_local
        assert np.array_equal(A.slot_ids()[:nl], B.slot_ids()[:nl])
        for k in range(7):
            assert _same(fa[k].get(0, nl), fb[k].get(0, nl)), (step, k)
        assert _same(copy.get(0, nl), fa[0].get(0, nl)), step
    assert created > 0 and removed > 0
    assert A.field_follow_mode(fa[0]) == "linear"
    A.close()
    B.close()


def test_modes_errors_getter_and_off_again(gpu):
    import types

    from dccrg_amd._lib import EINVAL, lib

    P = _cartesian((2, 2, 2), 1, (False, False, False), {"a": None})
    g, f = P.g, P.fields["a"][0]
    u32 = g.add_field("u32", np.uint32)
    var = g.add_variable_field("var", np.float64, False)
    assert g.field_follow_mode(f) is None
    for call, match in ((lambda: g.field_follow_mesh(var, "mean"), "variable-size"),
                        (lambda: g.field_follow_mesh(u32, "mean"), "8-byte"),
                        (lambda: g.field_follow_mode(u32), "8-byte"),
                        (lambda: g.field_follow_mesh(types.SimpleNamespace(id=99), "sum"), "invalid field id")):
        with pytest.raises(Exception, match=match) as e:
            call()
        assert e.value.code == EINVAL
    for mode in (-1, 4):
        assert lib().dccrgx_field_follow_mesh(g.h, f.id, mode) == EINVAL
    with pytest.raises(ValueError):
        g.field_follow_mesh(f, "cubic")
    assert g.field_follow_mode(f) is None
    for mode in ("mean", "sum", "linear", None):
        g.field_follow_mesh(f, mode)
        assert g.field_follow_mode(f) == mode
    # on, a round trip, off again: the bits of a grid that never followed
    g.field_follow_mesh(f, "linear")
    P.fields["a"] = (f, "linear")
    P.adapt(refine=(3,))
    ids, _ = P.by_id(f)
    P.adapt(unrefine=(int(ids[-1]),))
    g.field_follow_mesh(f, None)
    P.fields["a"] = (f, None)
    st = P.adapt(refine=(5,))
    assert st["children"] == 8
    ids, v = P.by_id(f)
    assert np.all(v[ids > 8] == v[ids > 8][0])
    st = P.adapt(unrefine=(int(ids[-1]),))
    ids, v = P.by_id(f)
    assert st["parents"] == 1 and v[ids == 5][0] == 0.0
    g.close()


# ---- several processes -------------------------------------------------------------------
def sc_follow(rank, world):
    """A refined grid whose families span processes (a third of the cells
    moved on) adapts with every process requesting: after the adapt and a
    halo, every slot's value equals the one-process model's, bitwise."""
    from oracle import oracle as O
    from test_gpu_transport import _gather, _grid

    length, R, per, hood = (4, 4, 4), 2, (True, False, True), 1
    g = _grid(length, R, per, hood)
    g.set_geometry(ODD_START, ODD_L0)
    o = O.Grid(length, R, per, hood, world)
    modes = {"off": None, "mean": "mean", "sum": "sum", "linear": "linear"}
    fields = {}
    for name, mode in modes.items():
        fields[name] = g.add_field(name, np.float64, True)
        g.field_follow_mesh(fields[name], mode)
    grad = [g.add_field(n, np.float64, False) for n in ("gx", "gy", "gz")]
    res = {k: True for k in list(modes) + ["leaves", "copies"]}
    res.update(merged_remote=False, outer_parent=False, children=False, parents=False, limited=False)
    for it in range(5):
        if it == 2:  # split families across processes
            loc = g.local_cells()
            mv = loc[loc % np.uint64(3) == 0]
            g.balance_load_to(mv, np.full(mv.size, (rank + 1) % world, np.int32))
            part = _gather(g.local_cells())
            pid = np.concatenate(part)
            pown = np.concatenate([np.full(len(v), r, np.int32) for r, v in enumerate(part)])
            order = np.argsort(pid)
            o.set_cells(pid[order], pown[order])
            for name in modes:  # the mode survives balance_load
                res[name] &= g.field_follow_mode(fields[name]) == modes[name]
        sl, nl = g.slot_ids(), g.n_local
        ni = g.counts["inner"]
        for k, name in enumerate(modes):
            fields[name].set(_vals(sl[:nl], k), 0)
        g.update_copies_of_remote_neighbors()
        g.gradient(fields["linear"], grad, 1.0)
        parts = _gather((sl[:nl], np.stack([x.get(0, nl) for x in grad], axis=1)))
        old = np.concatenate([p[0] for p in parts])
        order = np.argsort(old)
        old, D = old[order], np.concatenate([p[1] for p in parts])[order]
        res["leaves"] &= bool(np.array_equal(old, np.sort(o.cells()[0])))
        loc = sl[:nl].tolist()
        p_ref, p_unref = (0.3, 0.0) if it < 2 else (0.05, 0.6)
        acts = []
        for c in loc:
            u = np.random.default_rng(c * 131 + it).random()
            lvl = g.get_refinement_level(c)
            if lvl > 0 and u < p_unref:
                acts.append((0, c))
            elif lvl < R and u < p_unref + p_ref:
                acts.append((1, c))
        for k, c in acts:
            (g.unrefine_completely, g.refine_completely)[k](c)
        for lst in _gather(acts):
            for k, c in lst:
                (o.unrefine_completely, o.refine_completely)[k](c)
        g.stop_refining()
        o.stop_refining()
        g.update_copies_of_remote_neighbors()
        new = np.sort(o.cells()[0])
        sl2, nl2 = g.slot_ids(), g.n_local
        nr2 = g.counts["recv"]
        res["leaves"] &= bool(np.array_equal(np.sort(np.concatenate(_gather(sl2[:nl2]))), new))
        at = np.searchsorted(new, sl2[: nl2 + nr2])
        L = GM.cartesian_lengths(ODD_L0, GM.levels(old, length, R))
        for k, (name, mode) in enumerate(modes.items()):
            F = FM.follow(old, new, length, R, per, L, _vals(old, k), D, mode)
            got = fields[name].get(0, nl2 + nr2)
            res[name] &= _same(got[:nl2], F.values[at[:nl2]])
            res["copies"] &= _same(got[nl2:], F.values[at[nl2:]])
            if mode == "linear":
                res["children"] |= bool((F.kind == 1).any())
                res["parents"] |= bool((F.kind == 2).any())
                res["limited"] |= any(x[4] < 1.0 for x in F.limiter.values())
                slot = {c: i for i, c in enumerate(loc)}
                res["outer_parent"] |= any(slot[p] >= ni for p in F.limiter if p in slot)
        before = set(loc)
        res["merged_remote"] |= any(int(c) not in before for c in g.get_removed_cells())
    for k in ("merged_remote", "outer_parent", "children", "parents", "limited"):
        res[k] = any(_gather(res[k]))
    g.close()
    return res


@pytest.fixture(scope="module")
def follow_results(gpu, tmp_path_factory):
    from test_gpu_transport import _run_group

    return {w: _run_group(w, tmp_path_factory.mktemp(f"follow{w}"), ["sc_follow"], module="test_gpu_field_follow_mesh")
            for w in (2, 3)}


@pytest.mark.parametrize("world", [2, 3])
def test_families_and_parents_across_processes(follow_results, world):
    out = follow_results[world]
    assert "sc_follow" in out and len(out["sc_follow"]) == world
    for rank, (kind, res) in sorted(out["sc_follow"].items()):
        assert kind == "ok", f"rank {rank}:\n{res}"
        for k, v in res.items():
            assert v, f"world {world} rank {rank}: {k} failed ({res})"
