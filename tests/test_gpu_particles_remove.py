"""Particles removed on the device (Dccrg.particles_remove,
dccrg_amd/csrc/particles.hip) against the model of
tests/particles_remove_model.py.

The verdicts, the kept records (order included), the rescaled weights, the
counts and the records moved into another pool are compared bitwise per cell
id: both sides do the comparisons and operations include/dccrgx.h names.  A
tally's sum has no specified order: with arbitrary weights the tally fields
start at 0.0 (so the one sum T + S is exact) and are held to reduce_model's
    |dev - exact| <= gamma(k - 1) * sum |m|,  k the cell's removed records;
with dyadic weights every partial sum is exact and the tallies are bitwise."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest

import dccrg_amd
import particles_create_model as PC
import particles_remove_model as RM
from deposit_model import DepositModel
from helpers import make_pair
from particles_model import seeded_particles
from reduce_model import gamma
from test_gpu_particles import REF_L0, REF_START, REFINED, _local_cells, _same
from test_gpu_particles import _pair as _pair3
from test_gpu_particles_deposit import ODD_L0, ODD_START, _cell_field, _check_deposit, _pair, _upload_all
from test_gpu_particles_deposit import _seed as _seed_model

pytestmark = pytest.mark.gpu

INF = np.inf
_names = itertools.count()


def _local_ids(g):
    return np.asarray(g.slot_ids()[: g.n_local], np.uint64)


def _field_of(g, values):
    """A float64 Field of {id: value} (every slot; a missing id: 0.0)."""
    return _cell_field(g, f"rm{next(_names)}", {int(c): values.get(int(c), 0.0) for c in g.slot_ids()})


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _both(g, fld, cells, K, exact_tally, tally=(), mask=None, prob_field=None, into=None, **kw):
    """The call on the device and on the model's `cells` ({id: records} of the
    local cells, changed in place); everything compared.  tally: ((u, v),
    {id: start value}); into: (Field, {id: records}).  Returns the counts."""
    ids = _local_ids(g)
    nl, nr = g.n_local, g.n_slots - g.n_local
    for _, d in tally:
        for c in ids:
            d.setdefault(int(c), 0.0)
    t_flds = [_field_of(g, d) for _, d in tally]
    remote_t = [f.get(nl, nr) for f in t_flds] if nr else []
    dev = g.particles_remove(fld, K, mask=None if mask is None else _field_of(g, mask),
                             prob_field=None if prob_field is None else _field_of(g, prob_field),
                             tally=[(uv, f) for (uv, _), f in zip(tally, t_flds)],
                             into=None if into is None else into[0], **kw)
    start = [dict(d) for _, d in tally]
    exp, mags = RM.remove(cells, K, mask=mask, prob_field=prob_field, tally=tally,
                          into=None if into is None else into[1], **kw)
    print("remove", dev, exp)
    assert dev == exp
    got = _local_cells(g, fld, K)
    bad = [c for c in got if not _same(got[c], cells[c])]
    assert sorted(got) == sorted(cells) and not bad, (bad[:5], got[bad[0]], cells[bad[0]])
    if into is not None:
        gi = _local_cells(g, into[0], K)
        bad = [c for c in gi if not _same(gi[c], into[1][c].reshape(-1, K))]
        assert not bad, (bad[:5], gi[bad[0]], into[1][bad[0]])
    worst = 0.0
    for t, ((_, d), f) in enumerate(zip(tally, t_flds)):
        vals = f.get(0, nl)
        for c, v in zip(ids, vals):
            c = int(c)
            if c not in mags[t]:  # no record removed: the bits stay
                assert _bits(v) == _bits(start[t].get(c, 0.0)), (t, c, v)
            elif exact_tally:
                assert _bits(v) == _bits(d[c]), (t, c, v, d[c])
            else:
                k, S, exact = mags[t][c]
                assert start[t].get(c, 0.0) == 0.0
                bound = gamma(k - 1) * S
                err = abs(float(v) - exact)
                worst = max(worst, err / bound if bound else (0.0 if err == 0.0 else INF))
                assert err <= bound, (t, c, v, exact, bound)
        if nr:
            assert np.array_equal(_bits(f.get(nl, nr)), _bits(remote_t[t]))
    if tally and not exact_tally:
        print(f"tallies: largest error {worst:.3f} of its bound")
    return dev


def _odd_refined(K, seed, per_cell=6, full=300):
    g, m, fld = _pair(start=ODD_START, l0=ODD_L0, K=K, **REFINED)
    rng = np.random.default_rng(seed)
    _seed_model(m, rng, per_cell)
    if full:
        c = int(m.leaves[m.leaves.size // 2])
        ctr, ln = m.o.geometry([c])
        r = rng.random((full, K)) * 2 - 1
        r[:, 0:3] = (ctr[0] - ln[0] / 2) + ln[0] * rng.random((full, 3))
        m.set(c, r)
    _upload_all(g, fld, m)
    cells = {int(c): m.cells[int(c)].copy() for c in _local_ids(g)}
    return g, m, fld, cells, rng


def _mask_of(cells, rng):
    """A tenth of the cells absorb; of the others that hold records one has a
    NaN (absorbs) and one -0.0 (does not)."""
    mask = {c: float(rng.random() < 0.1) for c in cells}
    open_ = [c for c, v in mask.items() if v == 0.0 and cells[c].shape[0] >= 2]
    mask[open_[3]] = np.nan
    mask[open_[7]] = -0.0
    return mask


def test_all_stages_against_the_model(gpu):
    K = 10
    g, m, fld, cells, rng = _odd_refined(K, 71)
    ids = _local_ids(g)
    assert sum(a.shape[0] for a in cells.values()) > 1000
    mask = _mask_of(cells, rng)
    pf = {int(c): float(rng.choice([0.0, 0.3, 0.7, 1.0, 1.5])) for c in ids}
    x_lo = ODD_START[0] + 0.1 * 8 * ODD_L0[0]
    x_hi = ODD_START[0] + 0.9 * 8 * ODD_L0[0]
    st = _both(g, fld, cells, K, False, tests=[(0, "keep", x_lo, x_hi), (4, "drop", 0.5, INF)], mask=mask, prob=0.8,
               prob_field=pf, seed=0xFEEDBEEF12, rescale=True, weight=6,
               tally=[((-1, -1), {}), ((3, -1), {}), ((3, 3), {})])
    assert min(st.values()) > 20
    g.close()


def test_three_doubles_and_a_counting_tally(gpu):
    g, m, fld, cells, rng = _odd_refined(3, 72)
    ids = _local_ids(g)
    start = {int(c): -0.0 if k % 2 else 5.0 for k, c in enumerate(ids)}
    st = _both(g, fld, cells, 3, True, tests=[(1, "drop", -INF, ODD_START[1] + 2.0)], prob=0.5, seed=3,
               tally=[((-1, -1), start)])
    assert st["by_test"] > 50 and st["by_chance"] > 50 and st["kept"] > 50
    g.close()


def _dyadic(cells, rng, cols):
    for a in cells.values():
        a[:, cols] = rng.integers(-32, 33, (a.shape[0], len(cols))) / 16.0


def test_dyadic_weights_give_bitwise_tallies(gpu):
    K = 6
    g, m, fld, cells, rng = _odd_refined(K, 73)
    _dyadic(m.cells, rng, [3, 4, 5])
    _upload_all(g, fld, m)
    cells = {int(c): m.cells[int(c)].copy() for c in _local_ids(g)}

    def start():
        return {int(c): float(rng.integers(-8, 9)) / 4 for c in _local_ids(g)}

    st = _both(g, fld, cells, K, True, prob=0.6, seed=9, weight=5,
               tally=[((-1, -1), start()), ((3, -1), start()), ((3, 4), start()), ((4, 4), start())])
    assert st["by_chance"] > 300
    g.close()


def _full_cell_grid(K=4):
    g, m, fld = _pair((12, 10, 10), K=K)
    rng = np.random.default_rng(74)
    last = int(m.leaves[-1])
    ctr, ln = m.o.geometry([1, last])
    for c, k, n in ((1, 0, 5), (last, 1, 300)):
        r = rng.random((n, K)) * 2 - 1
        r[:, 0:3] = (ctr[k] - ln[k] / 2) + ln[k] * rng.random((n, 3))
        m.set(c, r)
    _upload_all(g, fld, m)
    return g, m, fld, last


def test_one_full_cell_among_empty_cells(gpu):
    """300 records in the last cell, 5 in the first, 1 198 empty cells
    between: the cell spans blocks, and the block pass that holds both cells'
    records has a window of the offsets past the LDS cache."""
    g, m, fld, last = _full_cell_grid()
    other = g.add_variable_field("escaped", np.float64, False)
    cells = {int(c): m.cells[int(c)].copy() for c in _local_ids(g)}
    into = {c: np.zeros((0, 4)) for c in cells}
    st = _both(g, fld, cells, 4, False, tests=[(3, "keep", 0.0, INF)], weight=3,
               tally=[((-1, -1), {}), ((3, 3), {})], into=(other, into))
    assert 100 < cells[last].shape[0] < 200 and st["kept"] + st["by_test"] == 305 and 0 < cells[1].shape[0] < 5
    assert into[last].shape[0] + cells[last].shape[0] == 300
    g.close()


@pytest.mark.parametrize("total", [255, 256, 257])
def test_record_totals_at_the_block_edge(gpu, total):
    g, m, fld = _pair((5, 4, 3), K=4)
    rng = np.random.default_rng(total)
    ids = _local_ids(g)
    n = np.full(ids.size, total // ids.size)
    n[: total - int(n.sum())] += 1
    for c, k in zip(ids, n):
        m.set(int(c), rng.random((int(k), 4)))
    _upload_all(g, fld, m)
    cells = {int(c): m.cells[int(c)].copy() for c in ids}
    assert sum(a.shape[0] for a in cells.values()) == total
    st = _both(g, fld, cells, 4, False, tests=[(3, "drop", 0.25, 0.5)], prob=0.25, seed=total, weight=3,
               tally=[((-1, -1), {})])
    assert sum(st.values()) == total
    # the last record of all decides for itself
    last = [int(c) for c in ids if cells[int(c)].shape[0]][-1]
    x = cells[last][-1, 3]
    st = _both(g, fld, cells, 4, False, tests=[(3, "drop", x, np.nextafter(x, INF))])
    assert st["by_test"] >= 1
    g.close()


def test_everything_removed_then_create_and_step(gpu):
    g, m, fld, cells, rng = _odd_refined(3, 75, full=0)
    n0 = sum(a.shape[0] for a in cells.values())
    st = _both(g, fld, cells, 3, True, prob=1.0, seed=1)
    assert st == dict(kept=0, by_mask=0, by_test=0, by_chance=n0)
    assert int(fld.sizes(0, g.n_local).sum()) == 0
    assert g.particles_remove(fld, 3, prob=1.0) == dict(kept=0, by_mask=0, by_test=0, by_chance=0)
    made = g.particles_create(fld, 3, count=2.0, seed=5)
    assert made == 2 * g.n_local
    assert g.particles_step(fld, 3, (0.0, 0.0, 0.0), 0.0)["stayed"] == made
    g.close()


def test_nothing_removed_changes_nothing(gpu):
    g, m, fld, cells, rng = _odd_refined(4, 76)
    n0 = sum(a.shape[0] for a in cells.values())
    sizes, before = fld.sizes(), fld.get()
    tl = {int(c): -0.0 for c in _local_ids(g)}
    st = _both(g, fld, cells, 4, True, tests=[(3, "keep", -INF, INF), (0, "drop", 5.0, 5.0)],
               mask={int(c): -0.0 for c in _local_ids(g)}, prob=-1.0, rescale=True, weight=3, tally=[((-1, -1), tl)])
    assert st == dict(kept=n0, by_mask=0, by_test=0, by_chance=0)
    assert np.array_equal(fld.sizes(), sizes) and all(_same(a, b) for a, b in zip(before, fld.get()))
    g.close()


def test_a_field_that_was_never_set(gpu):
    g, m, fld = _pair((4, 3, 2), K=4)
    tl = g.add_field("t", np.float64)
    tl.set(np.full(g.n_slots, 2.5))
    other = g.add_variable_field("other", np.float64, False)
    zero = dict(kept=0, by_mask=0, by_test=0, by_chance=0)
    assert g.particles_remove(fld, 4, prob=1.0, tally=[((-1, -1), tl)], into=other) == zero
    assert np.all(tl.get() == 2.5)
    # a pool into a field that was never set
    assert g.particles_create(fld, 4, count=2.0, seed=2) == 2 * g.n_local
    before = _local_cells(g, fld, 4)
    assert g.particles_remove(fld, 4, prob=1.0, into=other)["by_chance"] == 2 * g.n_local
    got = _local_cells(g, other, 4)
    assert all(_same(got[c], before[c]) for c in before)
    g.close()


def test_repeatable_and_seeded(gpu):
    res = []
    for seed in (11, 11, 12):
        g, m, fld, cells, rng = _odd_refined(5, 77)
        tl = g.add_field("t", np.float64)
        tl.set(np.zeros(g.n_slots))
        st = g.particles_remove(fld, 5, prob=0.5, seed=seed, rescale=True, weight=4, tally=[((3, 4), tl)])
        res.append((st, fld.sizes(), np.concatenate(fld.get()), tl.get()))
        g.close()
    a, b, c = res
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and _same(a[2], b[2]) and _same(a[3], b[3])
    assert not np.array_equal(a[1], c[1])


def test_two_views(gpu):
    """The views of process 0 and 1 of 2: remote copies keep bytes and sizes
    (of the pool, of the tally, of `into`), every local cell's result is what
    the one-process grid gives for that id."""
    K = 6

    def records(ids, ctr, ln):
        return seeded_particles(ids, ctr, ln, np.random.default_rng(78), 5, K)

    def call(g, fld, tl, other):
        mask = _field_of(g, {int(c): float(int(c) % 5 == 0) for c in g.slot_ids()})
        pf = _field_of(g, {int(c): (int(c) % 4) / 4 for c in g.slot_ids()})
        return g.particles_remove(fld, K, tests=[(3, "drop", 0.5, INF)], mask=mask, prob=1.0, prob_field=pf, seed=8,
                                  rescale=True, weight=5, tally=[((5, 4), tl)], into=other)

    g1, m1, f1 = _pair(start=ODD_START, l0=ODD_L0, K=K, **REFINED)
    ctr, ln = m1.o.geometry(m1.leaves)
    recs = records(m1.leaves, ctr, ln)  # per id: the same on every process
    for c, r in recs.items():
        m1.set(c, r)
    _upload_all(g1, f1, m1)
    t1 = _field_of(g1, {})
    o1 = g1.add_variable_field("other", np.float64, False)
    st1 = call(g1, f1, t1, o1)
    one, one_o = _local_cells(g1, f1, K), _local_cells(g1, o1, K)
    one_t = dict(zip((int(c) for c in _local_ids(g1)), t1.get(0, g1.n_local)))
    tot = {k: 0 for k in st1}
    for rank in (0, 1):
        g, o = make_pair(REFINED["length"], REFINED["R"], REFINED["periodic"], REFINED["hood"], REFINED["rounds"],
                         REFINED["frac"], nprocs=2, rank=rank)
        g.set_geometry(ODD_START, ODD_L0)
        fld = g.add_variable_field("particles", np.float64, True)
        other = g.add_variable_field("other", np.float64, False)
        fld.set([recs[int(c)].reshape(-1) for c in g.slot_ids()])
        other.set([recs[int(c)][:1].reshape(-1) for c in g.slot_ids()])
        tl = _field_of(g, {int(c): 7.0 for c in g.slot_ids()[g.n_local:]})
        nl, nr = g.n_local, g.n_slots - g.n_local
        assert nr > 0
        remote = [fld.get(nl, nr), other.get(nl, nr), tl.get(nl, nr)]
        assert sum(a.size for a in remote[0]) > 0
        st = call(g, fld, tl, other)
        got, got_o = _local_cells(g, fld, K), _local_cells(g, other, K)
        for c in got:
            assert _same(got[c], one[c]), c
            assert _same(got_o[c], np.concatenate([recs[c][:1], one_o[c]])), c
        assert all(_bits(v) == _bits(one_t[int(c)]) for c, v in zip(_local_ids(g), tl.get(0, nl)))
        for before, f in zip(remote[:2], (fld, other)):
            after = f.get(nl, nr)
            assert len(after) == len(before) and all(_same(x, y) for x, y in zip(before, after))
        assert np.all(tl.get(nl, nr) == 7.0)
        for k in tot:
            tot[k] += st[k]
        g.close()
    assert tot == st1 and min(st1.values()) > 0
    g1.close()


def _function_remove(g, fld, tl):
    """A remove whose arguments are functions of the cell id."""
    sl = g.slot_ids()
    mask = _field_of(g, {int(c): float(int(c) % 7 == 0) for c in sl})
    pf = _field_of(g, {int(c): (int(c) % 4) / 4 for c in sl})
    return g.particles_remove(fld, 6, tests=[(4, "keep", 1.0, 2.5)], mask=mask, prob=1.0, prob_field=pf, seed=33,
                              rescale=True, weight=3, tally=[((-1, -1), tl)])


def sc_remove(rank, world):
    """The refined case across real processes: created records (functions of
    the id) are removed; every process's local cells hold, bit for bit, what a
    one-process grid holds for the same ids."""
    import dccrg_amd
    from oracle import oracle as O
    from helpers import random_refines
    from test_gpu_particles_create import _function_create
    from test_gpu_transport import _gather, _grid

    c = REFINED
    o = O.Grid(c["length"], c["R"], c["periodic"], c["hood"], world)
    rng = np.random.default_rng(0)
    for _ in range(c["rounds"]):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        for cell in random_refines(ids, lv, c["R"], rng, c["frac"]):
            o.refine_completely(cell)
        o.stop_refining()
    g = _grid(c["length"], c["R"], c["periodic"], c["hood"])
    g.set_cells(*o.cells())
    g.set_geometry(ODD_START, ODD_L0)
    fld = g.add_variable_field("particles", np.float64, True)
    _function_create(g, fld)
    tl = _field_of(g, {})
    st = _function_remove(g, fld, tl)
    mine = _local_cells(g, fld, 6)
    mine_t = dict(zip((int(x) for x in _local_ids(g)), tl.get(0, g.n_local)))
    ids, _ = o.cells()
    g1 = dccrg_amd.Dccrg(0, 1, 0)
    g1.set_initial_length(c["length"]).set_maximum_refinement_level(c["R"]).set_periodic(*c["periodic"])
    g1.set_neighborhood_length(c["hood"]).initialize()
    g1.set_cells(ids, np.zeros(len(ids), np.int32))
    g1.set_geometry(ODD_START, ODD_L0)
    f1 = g1.add_variable_field("particles", np.float64, True)
    _function_create(g1, f1)
    t1 = _field_of(g1, {})
    st1 = _function_remove(g1, f1, t1)
    one = _local_cells(g1, f1, 6)
    one_t = dict(zip((int(x) for x in _local_ids(g1)), t1.get(0, g1.n_local)))
    res = dict(some_local=len(mine) > 0, counted=st["kept"] == sum(a.shape[0] for a in mine.values()),
               equal=all(_same(a, one[cid]) for cid, a in mine.items()),
               tally=all(_bits(v) == _bits(one_t[cid]) for cid, v in mine_t.items()))
    parts = _gather((st, sorted(mine)))
    res["every_cell_once"] = sorted(x for p in parts for x in p[1]) == sorted(one)
    res["totals"] = all(sum(p[0][k] for p in parts) == st1[k] and st1[k] > 10 for k in st1)
    g.close()
    g1.close()
    return res


def test_remove_across_processes(gpu, tmp_path_factory):
    from test_gpu_transport import _run_group

    results = _run_group(2, tmp_path_factory.mktemp("rm2"), names=["sc_remove"], module="test_gpu_particles_remove")
    assert "sc_remove" in results and len(results["sc_remove"]) == 2
    for rank, (kind, out) in sorted(results["sc_remove"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"


def test_into_appends_adds_up_and_returns(gpu):
    K = 4
    g, m, fld, cells, rng = _odd_refined(K, 79)
    other = g.add_variable_field("other", np.float64, False)
    ids = _local_ids(g)
    own = {int(c): rng.random((int(rng.integers(0, 3)), K)) for c in g.slot_ids()}
    other.set([own[int(c)].reshape(-1) for c in g.slot_ids()])
    into = {int(c): own[int(c)].copy() for c in ids}
    n0 = sum(a.shape[0] for a in cells.values())
    n_own = sum(a.shape[0] for a in into.values())
    st = _both(g, fld, cells, K, True, tests=[(3, "drop", 0.0, INF)], prob=0.3, seed=4, into=(other, into))
    gone = st["by_test"] + st["by_chance"]
    assert gone > 100 and st["kept"] + gone == n0
    assert sum(a.shape[0] for a in _local_cells(g, other, K).values()) == n_own + gone
    g.close()
    # everything into an empty pool and back: the original lists
    g, m, fld, cells, rng = _odd_refined(K, 80)
    other = g.add_variable_field("other", np.float64, False)
    orig = _local_cells(g, fld, K)
    n0 = sum(a.shape[0] for a in orig.values())
    assert g.particles_remove(fld, K, prob=1.0, into=other)["by_chance"] == n0
    assert int(fld.sizes(0, g.n_local).sum()) == 0
    assert g.particles_remove(other, K, tests=[(0, "drop", -INF, INF)], into=fld)["by_test"] == n0
    back = _local_cells(g, fld, K)
    assert all(_same(back[c], orig[c]) for c in orig) and int(other.sizes(0, g.n_local).sum()) == 0
    g.close()


def test_write_tracking_deposit_and_reduce_see_the_shortened_lists(gpu):
    g, m, fld = _pair(start=REF_START, l0=REF_L0, K=4, **REFINED)
    _seed_model(m, np.random.default_rng(81), 4)
    _upload_all(g, fld, m)
    out = g.add_field("rho", np.float64)
    _check_deposit(g, fld, DepositModel(m), out, "cic", 3)
    first = out.get(0, g.n_local)
    n0, = g.particles_reduce(fld, [("sum", None, None)], 4)
    cells = {int(c): m.cells[int(c)].copy() for c in _local_ids(g)}
    st = _both(g, fld, cells, 4, True, prob=0.5, seed=6)
    for c, a in cells.items():
        m.set(c, a)
    _check_deposit(g, fld, DepositModel(m), out, "cic", 3)
    assert not np.array_equal(first, out.get(0, g.n_local))
    n1, = g.particles_reduce(fld, [("sum", None, None)], 4)
    assert n1 == st["kept"] and n0 == st["kept"] + st["by_chance"] and st["by_chance"] > 100
    g.close()


def test_write_tracking_a_tally_into_a_cached_velocity(gpu):
    """The tally writes an advection velocity after advection_max_time_step
    has cached its result: the next time step is a cold twin's and differs
    from the one before the write."""
    from test_gpu_field_write_tracking import check_after_write, particles

    def w_remove(g, f, sp, st):
        p = particles(g, 7)
        st["counts"] = g.particles_remove(p, 4, prob=2.0, weight=3, tally=[((-1, -1), f[1])])

    r = check_after_write(w_remove, False)
    assert r["dt_changed"] and r["dt"] != r["dt_before"]


def test_follow_mesh_carries_a_pool_after_a_remove(gpu):
    from test_gpu_particles_adapt import _adapt, _check

    g, m, fld = _pair3(start=ODD_START, l0=ODD_L0, **REFINED)
    g.particles_follow_mesh(fld, 3)
    ids = _local_ids(g)
    lv = m.o.mapping.batch(ids)["level"]
    full = int(ids[lv < REFINED["R"]][5])
    cnt = {int(c): 2.0 for c in g.slot_ids()}
    cnt[full] = 600.0
    F = _cell_field(g, "cnt", cnt)
    n = np.array([int(cnt[int(c)]) for c in ids])
    assert g.particles_create(fld, 3, count=1.0, count_field=F, seed=41) == int(n.sum())
    ctr, ln = g.geometry(ids)
    cells = PC.records(ids, n, ctr, ln, 3, None, 41)
    st = _both(g, fld, cells, 3, True, prob=0.5, seed=42)
    assert cells[full].shape[0] > 200 and st["by_chance"] > 500
    for c, r in cells.items():
        m.set(c, r)
    ad = _adapt(g, m, refine=(full,))
    assert ad["lost"] == 0 and ad["to_children"] >= 200
    _check(g, fld, m, ad)
    g.close()


def test_refusals(gpu):
    """Every refusal of include/dccrgx.h's list but one, each leaving both
    pools and the tallies bitwise unchanged.  Not run: more than 2^31 - 1
    records in into_field afterwards, which needs a pool of over 51 GB."""
    K = 4
    g, m, fld = _pair((4, 3, 2), K=K)
    rho = g.add_field("rho", np.float64)
    rho2 = g.add_field("rho2", np.float64)
    u32 = g.add_field("u32", np.uint32)
    other = g.add_variable_field("other", np.float64, False)
    odd = g.add_variable_field("odd", np.float64, False)
    ghost = types.SimpleNamespace(id=99)
    assert g.particles_create(fld, K, count=2.0, recipe={3: ("uniform", 0.0, 1.0)}, seed=1) == 2 * g.n_local
    assert g.particles_create(other, K, count=1.0, seed=2) == g.n_local
    assert g.particles_create(odd, 3, count=1.0, seed=3) == g.n_local
    for f in (rho, rho2):
        f.set(np.arange(g.n_slots, dtype=np.float64))
    watched = (fld, other, odd)
    state = [(f.sizes(), f.get()) for f in watched]
    fixed = [rho.get(), rho2.get()]

    def unchanged():
        for (sizes, before), f in zip(state, watched):
            if not (np.array_equal(f.sizes(), sizes) and all(_same(a, b) for a, b in zip(before, f.get()))):
                return False
        return _same(rho.get(), fixed[0]) and _same(rho2.get(), fixed[1])

    everything = dict(prob=1.0, weight=3, tally=[((-1, -1), rho)], into=other)

    def refused(match, field=fld, k=K, **kw):
        args = dict(everything)
        args.update(kw)
        with pytest.raises(Exception, match=match):
            g.particles_remove(field, k, **args)
        assert unchanged(), match

    refused("fixed-size", field=rho2)
    refused("fixed-size", into=rho2)
    refused("at least 3 doubles", k=2, weight=-1)
    refused("not a multiple of 8", k=3, weight=-1, into=None)
    refused("not a multiple of 8", into=odd)
    refused("number of tests", tests=[(3, "keep", 0.0, 1.0)] * 9)
    refused("names a double outside", tests=[(K, "keep", 0.0, 1.0)])
    refused("names a double outside", tests=[(-1, "keep", 0.0, 1.0)])
    refused("mode must be", tests=[(3, 2, 0.0, 1.0)])
    refused("mode must be", tests=[(3, -1, 0.0, 1.0)])
    refused("bound is NaN", tests=[(3, "keep", np.nan, 1.0)])
    refused("bound is NaN", tests=[(3, "drop", 0.0, np.nan)])
    for bad, what in ((u32, "8-byte"), (other, "no fixed element layout"), (ghost, "invalid field id")):
        refused(what, mask=bad)
        refused(what, prob_field=bad)
        refused(what, tally=[((-1, -1), bad)])
    for p in (np.nan, np.inf, -np.inf):
        refused("finite", prob=p)
    refused("rescale needs", rescale=True, weight=-1)
    for w in (0, 2, K, -2):
        refused("weight_double must be", weight=w)
    for uv in ((2, -1), (-1, K), (-2, 3)):
        refused("tally factor", tally=[(uv, rho)])
    refused("number of tallies", tally=[((-1, -1), rho)] * 5)
    refused("two tallies share", tally=[((-1, -1), rho), ((3, -1), rho)])
    refused("also the mask_field", tally=[((-1, -1), rho)], mask=rho)
    refused("also the mask_field", tally=[((-1, -1), rho)], prob_field=rho)
    refused("into_field is the var_field", into=fld)
    # the raw call leaves the counts untouched
    st = (C.c_uint64 * 4)(7, 7, 7, 7)
    one_i, one_d = (C.c_int * 2)(3, 5), (C.c_double * 2)(0.0, 1.0)
    rc = dccrg_amd.lib().dccrgx_particles_remove(g.h, fld.id, K, one_i, one_d, 1, -1, -1, 1.0, 0, 0, -1, one_i, one_i, 0,
                                                 -1, st)
    assert rc == dccrg_amd._lib.EINVAL and b"mode" in dccrg_amd.lib().dccrgx_last_error() and list(st) == [7] * 4
    assert unchanged()
    # and the call they all refused goes through
    n = 2 * g.n_local
    assert g.particles_remove(fld, K, **everything) == dict(kept=0, by_mask=0, by_test=0, by_chance=n)
    g.close()
