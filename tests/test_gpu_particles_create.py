"""Particles created on the device (Dccrg.particles_create,
dccrg_amd/csrc/particles.hip) against the model of
tests/particles_create_model.py.

Every double that is not a normal is compared bitwise, per cell id, order
included: both sides do the operations include/dccrgx.h names, in its order,
on the same Philox words.  A normal's log and cos are library functions on
both sides; it is held to
    |dev - model| <= |spread| 2^-48 (1 + |z|) + 2^-52 |value|
(<= 1 ulp for log, <= 2 for cos, <= 1 for sqrt on the device, <= 1 ulp each
in the host libm, r <= sqrt(2 * 53 ln 2) ~ 8.6).

Largest deviation seen on an MI355X: 1.776e-15, 0.115 of its bound (the
append test's 5 864 normals with spreads up to 6; 0.106 of the bound over the
2 068 of test_bitwise_against_the_model).  The tests print the figure."""
import ctypes as C
import types

import numpy as np
import pytest

import dccrg_amd
import particles_create_model as PC
import stretched_model as SM
from deposit_model import DepositModel
from helpers import make_pair
from particles_model import ParticleModel
from test_gpu_particles import REF_L0, REF_START, REFINED, _local_cells, _same
from test_gpu_particles import _pair as _pair3
from test_gpu_particles_deposit import ODD_L0, ODD_START, _cell_field, _check_deposit, _pair, _upload_all
from test_gpu_particles_deposit import _seed as _seed_model
from test_particles_create_model_cpu import ROUND_SEED, STATS_CELLS, STATS_PER_CELL, STATS_SEED

pytestmark = pytest.mark.gpu

K10 = 10


def _local_ids(g):
    return np.asarray(g.slot_ids()[: g.n_local], np.uint64)


def _by_id(rng, ids, draw):
    return {int(c): float(draw(rng)) for c in ids}


def _case_fields(g, ids, rng):
    """The count field (0 in some cells, 1 in some, 300 in one) and three
    scaling fields, as {id: value} and as Fields."""
    cnt = {int(c): float(rng.integers(0, 2)) for c in ids}
    full = int(ids[ids.size // 2])
    cnt[full] = 300.0
    vals = dict(cnt=cnt, A=_by_id(rng, ids, lambda r: r.random() * 2 - 1), B=_by_id(rng, ids, lambda r: r.random() + 0.5),
                T=_by_id(rng, ids, lambda r: r.random() * 3))
    flds = {k: _cell_field(g, f"create_{k}", v) for k, v in vals.items()}
    return vals, flds, full


def _recipes(vals, flds, ids):
    """The case's recipe for the device and for the model."""
    arr = {k: np.array([v[int(c)] for c in ids]) for k, v in vals.items()}

    def both(F):
        return (dict((k, flds[v]) for k, v in F.items()), dict((k, arr[v]) for k, v in F.items()))

    spec = {3: (("const", 1.5), {}), 4: (("uniform", -2.0, 4.0), {}), 5: (("const", 0.25), dict(base_field="A")),
            6: (("uniform", 2.0, 0.5), dict(base_field="A", spread_field="B")),
            7: (("normal", 1.0, 2.0), dict(spread_field="T")), 9: (("normal", 0.0, 1.0), {})}
    dev, mod = {}, {}
    for j, (s, F) in spec.items():
        d, m = both(F)
        dev[j] = s + ((d,) if d else ())
        mod[j] = s + ((m,) if m else ())
    return dev, mod


def _model(g, ids, n, K, recipe, seed):
    ctr, ln = g.geometry(ids)
    return PC.records(ids, n, ctr, ln, K, recipe, seed, with_z=True)


def _assert_created(got, exp, zz, K, old=None):
    """got[c]: the cell's records; exp[c]: the model's new ones behind old[c]."""
    worst = worst_abs = 0.0
    exact = [j for j in range(K) if j not in zz[next(iter(zz))]] if zz else list(range(K))
    n_normals = 0
    for c, e in exp.items():
        a = got[c]
        k0 = 0 if old is None else old[c].shape[0]
        assert a.shape[0] == k0 + e.shape[0], (c, a.shape, k0, e.shape)
        if old is not None:
            assert _same(np.ascontiguousarray(a[:k0]), old[c]), c
        new = a[k0:]
        assert _same(np.ascontiguousarray(new[:, exact]), np.ascontiguousarray(e[:, exact])), (c, new, e)
        for j, (z, spread) in (zz[c] if zz else {}).items():
            dev = np.abs(new[:, j] - e[:, j])
            bound = np.abs(spread) * 2.0 ** -48 * (1 + np.abs(z)) + 2.0 ** -52 * np.abs(e[:, j])
            if dev.size:
                n_normals += dev.size
                worst = max(worst, float(np.max(dev / bound)))
                worst_abs = max(worst_abs, float(np.max(dev)))
            assert np.all(dev <= bound), (c, j, new[:, j], e[:, j], bound)
    print(f"normals: {n_normals} compared, largest |dev - model| {worst_abs:.3e}, {worst:.4f} of its bound")


@pytest.fixture(scope="module")
def refined_case(gpu):
    """The refined grid with the odd geometry after one create of K = 10."""
    g, m, fld = _pair(start=ODD_START, l0=ODD_L0, K=K10, **REFINED)
    ids = _local_ids(g)
    vals, flds, full = _case_fields(g, ids, np.random.default_rng(61))
    dev, mod = _recipes(vals, flds, ids)
    n = np.array([int(vals["cnt"][int(c)]) for c in ids])
    made = g.particles_create(fld, K10, count=1.0, count_field=flds["cnt"], recipe=dev, seed=0xC0FFEE12345)
    yield dict(g=g, m=m, fld=fld, ids=ids, vals=vals, flds=flds, full=full, dev=dev, mod=mod, n=n, made=made)
    g.close()


def test_bitwise_against_the_model(refined_case):
    c = refined_case
    g, ids, n = c["g"], c["ids"], c["n"]
    assert c["made"] == int(n.sum()) and np.count_nonzero(n == 0) > 10 and np.count_nonzero(n == 1) > 10
    exp, zz = _model(g, ids, n, K10, c["mod"], 0xC0FFEE12345)
    got = _local_cells(g, c["fld"], K10)
    _assert_created(got, exp, zz, K10)
    ctr, ln = g.geometry(ids)
    for k, cid in enumerate(ids):
        r = got[int(cid)]
        assert np.all((r[:, 0:3] >= ctr[k] - ln[k] / 2) & (r[:, 0:3] < ctr[k] + ln[k] / 2))
        assert np.all(r[:, 8] == 0.0)


def test_two_full_cells_at_the_ends_of_a_row_of_empty_ones(gpu):
    """The record search's direct branch: the one block pass of the generate
    kernel holds the records of the first and of the last local slot, so its
    window of the new records' offsets is 1 201 entries, more than the 1 024
    a block keeps in LDS, and every double finds its cell in global memory."""
    g, m, fld = _pair((1200, 1, 1), periodic=(False, False, False), K=4)
    ids = _local_ids(g)
    assert ids.size == 1200 == g.n_slots
    n = np.zeros(ids.size, np.int64)
    n[0] = n[-1] = 1  # in slot order: 1 198 empty slots between the two records of the pass
    cnt = _cell_field(g, "cnt", {int(c): float(k) for c, k in zip(ids, n)})
    rec = {3: ("uniform", -2.0, 4.0)}
    assert g.particles_create(fld, 4, count=1.0, count_field=cnt, recipe=rec, seed=0xFACADE) == 2
    exp, zz = _model(g, ids, n, 4, rec, 0xFACADE)
    _assert_created(_local_cells(g, fld, 4), exp, zz, 4)
    g.close()


def test_append_keeps_the_lists_and_repeats_with_the_seed(refined_case):
    c = refined_case
    g, fld, ids = c["g"], c["fld"], c["ids"]
    before = _local_cells(g, fld, K10)
    n2 = np.full(ids.size, 2)
    assert g.particles_create(fld, K10, count=2.9, recipe=c["dev"], seed=7) == 2 * ids.size
    exp, zz = _model(g, ids, n2, K10, c["mod"], 7)
    after = _local_cells(g, fld, K10)
    _assert_created(after, exp, zz, K10, old=before)
    assert g.particles_create(fld, K10, count=2.0, recipe=c["dev"], seed=7) == 2 * ids.size
    again = _local_cells(g, fld, K10)
    assert g.particles_create(fld, K10, count=2.0, recipe=c["dev"], seed=8) == 2 * ids.size
    other = _local_cells(g, fld, K10)
    for cid in after:
        k = after[cid].shape[0]
        assert _same(np.ascontiguousarray(again[cid][:k]), after[cid])
        assert _same(np.ascontiguousarray(again[cid][k:]), np.ascontiguousarray(after[cid][k - 2:]))  # the same seed
        assert _same(np.ascontiguousarray(other[cid][:k + 2]), again[cid])
        assert not np.any(other[cid][k + 2:, [0, 1, 2, 4]] == again[cid][k:, [0, 1, 2, 4]])  # another seed


def test_statistics_on_the_device(gpu):
    g, m, fld = _pair((8, 8, 8), K=4)
    assert g.n_local == STATS_CELLS and np.array_equal(np.sort(_local_ids(g)), np.arange(1, STATS_CELLS + 1))
    N = g.particles_create(fld, 4, count=STATS_PER_CELL, recipe={3: ("normal", 0.0, 1.0)}, seed=STATS_SEED)
    assert N == 2 ** 18
    s1, s2, cnt = g.particles_reduce(fld, [("sum", 3, None), ("sum", 3, 3), ("sum", None, None)], 4)
    mean = s1 / N
    var = s2 / N - mean * mean
    print("device normals: mean", mean, "variance", var)
    assert cnt == N
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1.0) <= 5 * np.sqrt(2.0 / N)
    g.close()


def test_random_rounding(gpu):
    g, m, fld = _pair((8, 8, 8), K=3)
    ids = _local_ids(g)
    half = _cell_field(g, "half", {int(c): 0.5 for c in g.slot_ids()})
    made = g.particles_create(fld, 3, count=1.0, count_field=half, round="random", seed=ROUND_SEED)
    n = (fld.sizes(0, g.n_local) // np.uint64(24)).astype(np.int64)
    assert np.array_equal(n, PC.counts(ids, 1.0, np.full(ids.size, 0.5), random=True, seed=ROUND_SEED))
    assert made == int(n.sum()) and abs(made - 256) <= 5 * np.sqrt(512 * 0.25)
    # the rounding's uniform depends on the cell and the seed only: the positions are the model's
    ctr, ln = g.geometry(ids)
    exp = PC.records(ids, n, ctr, ln, 3, None, ROUND_SEED)
    got = _local_cells(g, fld, 3)
    assert all(_same(got[int(c)], exp[int(c)]) for c in ids)
    g.close()


def test_created_records_are_located_in_their_own_cell(gpu):
    g, m, fld = _pair3(start=REF_START, l0=REF_L0, **REFINED)
    made = g.particles_create(fld, 3, count=3.0, seed=11)
    assert made == 3 * g.n_local
    st = g.particles_step(fld, 3, (0.0, 0.0, 0.0), 0.0)
    assert st == dict(stayed=made, moved=0, arrived=0, handed_over=0, lost=0)
    g.close()


@pytest.mark.parametrize("name", SM.CASES)
def test_stretched_geometry(gpu, name):
    from test_gpu_stretched import _pair as stretched_pair

    g, m, fld, coords, R = stretched_pair(name)
    ids = _local_ids(g)
    made = g.particles_create(fld, 3, count=2.0, seed=12)
    assert made == 2 * ids.size
    ctr, ln = g.geometry(ids)
    exp = PC.records(ids, np.full(ids.size, 2), ctr, ln, 3, None, 12)
    got = _local_cells(g, fld, 3)
    assert all(_same(got[int(c)], exp[int(c)]) for c in ids)
    assert len({round(float(x), 9) for x in ln[:, 0]}) > 3  # cells of several lengths
    g.close()


def _function_fields(g):
    """Cell fields that are functions of the id, the same on every process."""
    sl = g.slot_ids()
    cnt = {int(c): float(int(c) % 3) for c in sl}
    A = {int(c): 0.5 + (int(c) % 7) / 8 for c in sl}
    return _cell_field(g, "cnt", cnt), _cell_field(g, "A", A)


def _function_create(g, fld, seed=21):
    cnt, A = _function_fields(g)
    rec = {3: ("const", 0.5, dict(base_field=A)), 4: ("uniform", 1.0, 2.0, dict(spread_field=A)), 5: ("normal", 0.0, 1.0)}
    return g.particles_create(fld, 6, count=1.0, count_field=cnt, recipe=rec, seed=seed)


def test_two_views(gpu):
    """The views of process 0 and 1 of 2: remote copies keep their records,
    local cells hold what the one-process grid holds for the same ids."""
    g1, m1, f1 = _pair(start=ODD_START, l0=ODD_L0, K=6, **REFINED)
    _function_create(g1, f1)
    one = _local_cells(g1, f1, 6)
    seen = 0
    for rank in (0, 1):
        g, o = make_pair(REFINED["length"], REFINED["R"], REFINED["periodic"], REFINED["hood"], REFINED["rounds"],
                         REFINED["frac"], nprocs=2, rank=rank)
        g.set_geometry(ODD_START, ODD_L0)
        m = ParticleModel(o, ODD_START, ODD_L0, 6)
        fld = g.add_variable_field("particles", np.float64, True)
        _seed_model(m, np.random.default_rng(62 + rank), 4)
        _upload_all(g, fld, m)
        nl, nr = g.n_local, g.n_slots - g.n_local
        assert nr > 0
        remote = fld.get(nl, nr)
        assert sum(a.size for a in remote) > 0
        made = _function_create(g, fld)
        got = _local_cells(g, fld, 6)
        assert made == sum(int(c) % 3 for c in got)
        for c, a in got.items():
            k = m.cells[c].shape[0]
            assert _same(np.ascontiguousarray(a[:k]), m.cells[c]) and _same(np.ascontiguousarray(a[k:]), one[c]), c
        after = fld.get(nl, nr)
        assert len(after) == len(remote) and all(_same(x, y) for x, y in zip(remote, after))
        seen += len(got)
        g.close()
    assert seen == len(one)
    g1.close()


def sc_create(rank, world):
    """The refined case across real processes: every process's local cells
    hold, bit for bit, what a one-process grid creates for the same ids."""
    import dccrg_amd
    from oracle import oracle as O
    from helpers import random_refines
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
    made = _function_create(g, fld)
    mine = _local_cells(g, fld, 6)
    ids, _ = o.cells()
    g1 = dccrg_amd.Dccrg(0, 1, 0)
    g1.set_initial_length(c["length"]).set_maximum_refinement_level(c["R"]).set_periodic(*c["periodic"])
    g1.set_neighborhood_length(c["hood"]).initialize()
    g1.set_cells(ids, np.zeros(len(ids), np.int32))
    g1.set_geometry(ODD_START, ODD_L0)
    f1 = g1.add_variable_field("particles", np.float64, True)
    total = _function_create(g1, f1)
    one = _local_cells(g1, f1, 6)
    res = dict(some_local=len(mine) > 0, counted=made == sum(a.shape[0] for a in mine.values()),
               equal=all(_same(a, one[cid]) for cid, a in mine.items()))
    parts = _gather((made, sorted(mine)))
    res["every_cell_once"] = sorted(x for p in parts for x in p[1]) == sorted(one)
    res["total"] = sum(p[0] for p in parts) == total and total > 100
    res["split"] = all(p[0] > 0 for p in parts)
    g.close()
    g1.close()
    return res


def test_create_across_processes(gpu, tmp_path_factory):
    from test_gpu_transport import _run_group

    results = _run_group(2, tmp_path_factory.mktemp("cw2"), names=["sc_create"], module="test_gpu_particles_create")
    assert "sc_create" in results and len(results["sc_create"]) == 2
    for rank, (kind, out) in sorted(results["sc_create"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"


def test_write_tracking_deposit_sees_the_new_records(gpu):
    g, m, fld = _pair(start=REF_START, l0=REF_L0, K=4, **REFINED)
    _seed_model(m, np.random.default_rng(63), 4)
    _upload_all(g, fld, m)
    out = g.add_field("rho", np.float64)
    _check_deposit(g, fld, DepositModel(m), out, "cic", 3)
    first = out.get(0, g.n_local)
    ids = _local_ids(g)
    rec = {3: ("uniform", 0.5, 1.0)}
    assert g.particles_create(fld, 4, count=2.0, recipe=rec, seed=31) == 2 * ids.size
    ctr, ln = g.geometry(ids)
    new = PC.records(ids, np.full(ids.size, 2), ctr, ln, 4, rec, 31)
    for c in ids:
        m.set(int(c), np.concatenate([m.cells[int(c)], new[int(c)]]))
    _check_deposit(g, fld, DepositModel(m), out, "cic", 3)
    assert not np.array_equal(first, out.get(0, g.n_local))
    g.close()


def test_follow_mesh_carries_created_records(gpu):
    from test_gpu_particles_adapt import _adapt, _check

    g, m, fld = _pair3(start=ODD_START, l0=ODD_L0, **REFINED)
    g.particles_follow_mesh(fld, 3)
    ids = _local_ids(g)
    lv = m.o.mapping.batch(ids)["level"]
    full = int(ids[lv < REFINED["R"]][5])
    cnt = {int(c): 1.0 for c in g.slot_ids()}
    cnt[full] = 300.0
    F = _cell_field(g, "cnt", cnt)
    n = np.array([int(cnt[int(c)]) for c in ids])
    assert g.particles_create(fld, 3, count=1.0, count_field=F, seed=41) == int(n.sum())
    ctr, ln = g.geometry(ids)
    for c, r in PC.records(ids, n, ctr, ln, 3, None, 41).items():
        m.set(c, r)
    st = _adapt(g, m, refine=(full,))
    assert st["lost"] == 0 and st["to_children"] >= 300
    _check(g, fld, m, st)
    g.close()


def test_refusals(gpu):
    from oracle import oracle as O

    g, m, fld = _pair((4, 3, 2), K=4)
    ids = _local_ids(g)
    out = g.add_field("rho", np.float64)
    u32 = g.add_field("u32", np.uint32)
    other = g.add_variable_field("other", np.float64, False)
    ghost = types.SimpleNamespace(id=99)
    assert g.particles_create(fld, 4, count=1.0, recipe={3: ("const", 2.0)}, seed=1) == ids.size
    sizes, before = fld.sizes(), fld.get()

    def unchanged():
        return np.array_equal(fld.sizes(), sizes) and all(_same(a, b) for a, b in zip(before, fld.get()))

    with pytest.raises(Exception, match="fixed-size"):
        g.particles_create(out, 4)
    with pytest.raises(Exception, match="at least 3 doubles"):
        g.particles_create(fld, 2)
    with pytest.raises(Exception, match="not a multiple of 8"):
        g.particles_create(fld, 3)
    with pytest.raises(Exception, match="recipe kind"):
        g.particles_create(fld, 4, recipe={3: (3, 1.0, 1.0)})
    with pytest.raises(Exception, match="recipe kind"):
        g.particles_create(fld, 4, recipe={3: (-1, 1.0, 1.0)})
    for bad, what in ((u32, "8-byte"), (other, "no fixed element layout"), (ghost, "invalid field id")):
        with pytest.raises(Exception, match=what):
            g.particles_create(fld, 4, count_field=bad)
        with pytest.raises(Exception, match=what):
            g.particles_create(fld, 4, recipe={3: ("const", 1.0, dict(base_field=bad))})
        with pytest.raises(Exception, match=what):
            g.particles_create(fld, 4, recipe={3: ("uniform", 1.0, 1.0, dict(spread_field=bad))})
    with pytest.raises(ValueError):
        g.particles_create(fld, 4, round="nearest")
    made = C.c_uint64(5)
    ri, rd = (C.c_int * 12)(*([0, -1, -1] * 4)), (C.c_double * 8)()
    rc = dccrg_amd.lib().dccrgx_particles_create(g.h, fld.id, 4, -1, 1.0, 2, ri, rd, 0, C.byref(made))
    assert rc == dccrg_amd._lib.EINVAL and b"round_random" in dccrg_amd.lib().dccrgx_last_error()
    for count in (np.nan, np.inf, -np.inf):
        with pytest.raises(Exception, match="finite"):
            g.particles_create(fld, 4, count=count)
    assert unchanged()
    # counts found on the device: the cell is named, nothing changes
    for bad in (np.nan, -1.0, 2.0 ** 31):
        vals = {int(c): 1.0 for c in g.slot_ids()}
        vals[int(ids[7])] = bad
        F = _cell_field(g, f"bad{bad}", vals)
        with pytest.raises(Exception, match=f"cell {int(ids[7])} "):
            g.particles_create(fld, 4, count=1.0, count_field=F)
        assert unchanged()
    with pytest.raises(Exception, match="cell "):
        g.particles_create(fld, 4, count=-0.5)
    with pytest.raises(Exception, match="cell "):
        g.particles_create(fld, 4, count=2.0 ** 31)
    assert unchanged()
    zero = _cell_field(g, "zero", {int(c): 0.0 for c in g.slot_ids()})
    assert g.particles_create(fld, 4, count=5.0, count_field=zero) == 0
    assert g.particles_create(fld, 4, count=0.999) == 0
    assert unchanged()
    # a stretched file block without coordinates: no geometry on the device
    g.set_geometry_block(O.stretched_geometry_block([[0.0, 0.5, 1.5, 3.0, 5.0], [0.0, 1.0, 2.0, 4.0], [0.0, 1.0, 2.0]]))
    with pytest.raises(Exception, match="stretched geometry block"):
        g.particles_create(fld, 4)
    assert unchanged()
    g.close()
