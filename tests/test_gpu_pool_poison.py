"""The device pool's poison mode (DCCRGX_POOL_POISON, csrc/pool.hip) as a
detector of uninitialised and stale device reads.

Every buffer of the library comes from one caching pool.  A block handed out
without being cleared is either fresh device memory, which usually reads as
zero, or a recycled block of the same size class, which in a test that builds
the same small mesh twice usually holds the right answer of the last identical
call.  Either way a kernel that skips an element passes.  With the knob set,
every byte of a block holds the fill byte when it is handed out, when it is
released, and when DBuf::alloc keeps a block of the same size, so the
comparisons the suite already makes see what such a kernel leaves behind.

Two bytes, for what they decode to here: 255 makes every double a NaN and
every int32 -1 (this code's "none" slot: an integer read of it can pass); 165
makes an int32 negative but not -1, unsigned words huge, flags non-zero and a
double tiny and finite (it can vanish in a sum).

(a) the contract of what the library promises about new memory, directly;
(b) existing tests of every subsystem, called as they are under both bytes:
their own assertions against oracle, model or byte model are the judge."""
import contextlib
import importlib
import inspect

import numpy as np
import pytest

import dccrg_amd
from test_gpu_multirank import CASES as RANK_VIEWS

pytestmark = pytest.mark.gpu

BYTES = (255, 165)
KNOB = "DCCRGX_POOL_POISON"


@pytest.fixture(params=BYTES, ids=lambda b: f"byte{b}")
def poison(request, gpu, monkeypatch):
    monkeypatch.setenv(KNOB, str(request.param))
    return request.param


def _grid(length, R, periodic=(False, False, False), hood=1, init=True):
    g = dccrg_amd.Dccrg(0, 1, 0)
    g.set_initial_length(length).set_maximum_refinement_level(R).set_periodic(*periodic).set_neighborhood_length(hood)
    return g.initialize() if init else g


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# element sizes 1, 2, 4 and 8 bytes, and one subarray type (64 bytes)
DTYPES = [np.uint8, np.int16, np.uint32, np.float64, np.dtype((np.uint64, 8))]


# ---- (a) what new memory holds ---------------------------------------------------------
def test_field_added_after_initialize_is_zero(poison):
    g = _grid((5, 4, 3), 1, (True, False, True))
    for k, dt in enumerate(DTYPES):
        f = g.add_field(f"late{k}", dt)
        got = f.get()
        assert got.shape[0] == g.n_slots
        assert not _bits(got).any(), (np.dtype(dt), int(np.count_nonzero(_bits(got))))
    g.close()


def test_field_added_before_initialize_is_zero(poison):
    g = _grid((5, 4, 3), 1, (True, False, True), init=False)
    fields = [g.add_field(f"early{k}", dt) for k, dt in enumerate(DTYPES)]
    g.initialize()
    for f in fields:
        got = f.get()
        assert got.shape[0] == g.n_slots
        assert not _bits(got).any(), (f.dtype, int(np.count_nonzero(_bits(got))))
    g.close()


def test_variable_field_starts_empty(poison):
    g = _grid((5, 4, 3), 1, (True, False, True))
    v = g.add_variable_field("late", np.int32)
    assert v.sizes().shape[0] == g.n_slots and not v.sizes().any()
    g.close()
    g = _grid((5, 4, 3), 1, (True, False, True), init=False)
    v = g.add_variable_field("early", np.int32)
    g.initialize()
    assert v.sizes().shape[0] == g.n_slots and not v.sizes().any()
    assert all(a.size == 0 for a in v.get())
    g.close()


def _pattern(ids, dt):
    """Distinct bytes per cell, none of them all zero, all 0xFF or all 0xA5."""
    dt = np.dtype(dt)
    n = dt.itemsize
    h = np.asarray(ids, np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15) + np.arange(1, n + 1, dtype=np.uint64) * \
        np.uint64(0xBF58476D1CE4E5B9)
    b = ((h >> np.uint64(37)) & np.uint64(0x7F)).astype(np.uint8) | np.uint8(1)  # 1..127, odd
    return np.ascontiguousarray(b)


def test_refinement_keeps_survivors_and_fills_new_cells(poison):
    """8 x 8 x 8, R = 2: a rebuild allocates every field anew.  Cells that
    stay keep their bytes, a new child has its parent's (tests/payload_model.py,
    test_gpu_payload_bytes.py), a variable-size field's child is empty
    (test_gpu_variable.py), a merged parent is zero and the removed children's
    payloads are kept aside (test_gpu_unrefine.py)."""
    g = _grid((8, 8, 8), 2)
    fields = [g.add_field(f"f{k}", dt) for k, dt in enumerate(DTYPES)]
    var = g.add_variable_field("var", np.int32)

    def fill():
        ids = g.slot_ids()[: g.n_local]
        for f in fields:
            f.set(_pattern(ids, f.dtype).view(f.dtype.base).reshape((ids.size,) + f.dtype.shape))
        var.set([np.full(int(c) % 3 + 1, int(c), np.int32) for c in ids])
        return ids

    def parents(ids):
        return g.mapping_batch(np.asarray(ids, np.uint64))["parent"]

    # two rounds of refinement: level 1, then level 2 inside it
    old = fill()
    for c in (1, 37, 512, 200):
        assert g.refine_completely(c)
    new = np.sort(np.asarray(g.stop_refining(), np.uint64))
    assert new.size == 32
    for rnd in range(2):
        now = g.slot_ids()[: g.n_local]
        is_new = np.isin(now, new)
        src = np.where(is_new, parents(now), now)
        assert np.isin(src, old).all()
        for f in fields:
            got = _bits(f.get(0, g.n_local)).reshape(now.size, -1)
            assert np.array_equal(got, _pattern(src, f.dtype)), (rnd, f.dtype)
        for c, fresh, a in zip(now.tolist(), is_new.tolist(), var.get(0, g.n_local)):
            assert np.array_equal(a, np.zeros(0, np.int32) if fresh else np.full(c % 3 + 1, c, np.int32)), (rnd, c)
        if rnd == 0:
            old = fill()
            # a child of cell 1 (which induces the refinement of its level-0 neighbors) and one more level-0 cell
            for c in (int(new[0]), 300):
                assert g.refine_completely(c)
            new = np.sort(np.asarray(g.stop_refining(), np.uint64))
            assert new.size > 16 and set(g.mapping_batch(new)["level"].tolist()) == {1, 2}

    # and back: one family of level-2 cells merges into its parent
    old = fill()
    kids = new[g.mapping_batch(new)["level"] == 2][:8]
    par = int(parents(kids[:1])[0])
    assert np.all(parents(kids) == par)
    assert g.unrefine_completely(int(kids[0]))
    g.stop_refining()
    removed = np.asarray(g.get_removed_cells(sorted=False), np.uint64)
    assert np.array_equal(np.sort(removed), np.sort(kids))
    now = g.slot_ids()[: g.n_local]
    assert par in now.tolist() and not np.isin(kids, now).any()
    for f in fields:
        got = _bits(f.get(0, g.n_local)).reshape(now.size, -1)
        want = _pattern(now, f.dtype)
        want[now == par] = 0
        assert np.array_equal(got, want), f.dtype
        assert np.array_equal(_bits(f.get_removed()).reshape(removed.size, -1), _pattern(removed, f.dtype)), f.dtype
    for c, a in zip(now.tolist(), var.get(0, g.n_local)):
        assert np.array_equal(a, np.zeros(0, np.int32) if c == par else np.full(c % 3 + 1, c, np.int32)), c
    for c, a in zip(removed.tolist(), var.get_removed()):
        assert np.array_equal(a, np.full(c % 3 + 1, c, np.int32)), c
    g.close()


def test_second_identical_call_has_the_bits_of_the_first(poison):
    """The "last call's answer" case: the same operation twice, its buffers of
    the same sizes both times, the outputs overwritten with a third pattern in
    between.  The gradient on a refined grid (test_gpu_gradient.py holds it
    bitwise to its model where no finer neighbor is involved)."""
    G = importlib.import_module("test_gpu_gradient")
    c, model = G._refined(0)
    want = model(0.37)
    c.fill()
    c.g.gradient(c.f, c.out, 0.37)
    first = c.check(want, 0.37)
    c.fill(3.25)
    c.g.gradient(c.f, c.out, 0.37)
    second = c.check(want, 0.37)
    for a, b in zip(first, second):
        assert G._same(a, b)
    c.g.close()


# ---- (b) replays -------------------------------------------------------------------------
# (module, test, its arguments; fixtures are passed through by name)
T, F = True, False
REPLAYS = [
    # mesh build, closure
    ("test_gpu_neighbors", "test_refined", dict(length=(4, 4, 4), R=2, periodic=(T, T, T), hood=1, rounds=2, frac=0.15,
                                                seed=4)),
    ("test_gpu_neighbors", "test_refinement_closure_matches", dict(seed=11)),
    # unrefine, user neighborhoods, the append's second launch
    ("test_gpu_unrefine", "test_unrefine_matches_oracle",
     dict(case=dict(length=(6, 5, 4), R=2, per=(T, T, F), hood=0, seed=2))),
    ("test_gpu_user_hood", "test_user_hood_lists_match_oracle",
     dict(length=(6, 6, 6), R=2, periodic=(T, T, F), L=1, rounds=2, k=7)),
    ("test_gpu_user_hood", "test_user_hood_update_lists",
     dict(length=(6, 6, 6), R=2, periodic=(T, T, F), L=1, P=4, rounds=2)),
    ("test_gpu_append_retry", "test_induced_refines_second_launch_same_mesh", {}),
    ("test_gpu_append_retry", "test_ghost_ring_second_launch_same_knowledge", {}),
    # rank views, halo lists, slab plans
    ("test_gpu_multirank", "test_rank_views_match_oracle",
     dict(zip(("length", "R", "periodic", "hood", "P", "rounds"), RANK_VIEWS[4]))),
    ("test_gpu_multirank", "test_slab_gol_structured_equals_single_rank",
     dict(length=(256, 6, 9), periodic=(T, F, T), P=3)),
    # game of life
    ("test_gpu_gol", "test_structured_matches_oracle", dict(length=(256, 6, 9), periodic=(T, T, T))),
    ("test_gpu_gol", "test_csr_refined_matches_oracle", {}),
    ("test_gpu_gol_amr", "test_refined_game_matches_oracle",
     dict(length=(9, 8, 7), periodic=(T, T, T), frac=0.4, seed=2, density=0.05, steps=1)),
    ("test_gpu_gol_amr", "test_turn_equals_split_phases_and_clears_lists", {}),
    # advection
    ("test_gpu_advection", "test_steps_match_oracle", dict(base=(16, 16, 2), R=2, steps=30)),
    ("test_gpu_advection", "test_parity_grid_exercises_both_tile_kernels", {}),
    ("test_gpu_advection", "test_inner_outer_split_equals_all", {}),
    ("test_gpu_advection", "test_neighbor_records_bitwise_equal_fields", dict(base=(12, 12, 3), R=2)),
    ("test_gpu_advection_3d", "test_sweeps_match_the_model", dict(name="nested", periodic=(T, T, T), path="table")),
    ("test_gpu_advection_adapt", "test_adaptive_advection_matches_oracle", dict(base=(10, 10, 3), R=2, steps=15)),
    ("test_gpu_advection_lds", "test_three_levels_in_one_general_tile", {}),
    # Poisson
    ("test_gpu_poisson", "test_cache_factors_bitwise", {}),
    ("test_gpu_poisson", "test_fixed_iterations_match_oracle", dict(iters=5, tol=1e-11)),
    ("test_gpu_poisson", "test_failsafe_matches_oracle", {}),
    ("test_gpu_poisson_stretched", "test_fixed_iterations_match_model", dict(iters=5)),
    # fields
    ("test_gpu_gradient", "test_views_of_several_processes", dict(nprocs=3, rank=1)),
    ("test_gpu_curl_divergence", "test_views_of_several_processes", dict(nprocs=3, rank=1)),
    ("test_gpu_field_reduce", "test_regions_on_detached_views", {}),
    ("test_gpu_field_follow_mesh", "test_refined_periodic_grid_mixed_fields", {}),
    # payloads, files
    ("test_gpu_payload_bytes", "test_rebuild_carry_and_removed_store", {}),
    ("test_gpu_payload_bytes", "test_variable_pool", {}),
    ("test_gpu_variable", "test_payloads_survive_refinement", {}),
    ("test_gpu_grid_file", "test_file_bytes_and_round_trip",
     dict(length=(4, 3, 2), R=2, periodic=(T, F, T), hood=1, rounds=2)),
    ("test_gpu_grid_file", "test_variable_payload_file_and_round_trip", {}),
    # particles
    ("test_gpu_particles", "test_refined_grid", {}),
    ("test_gpu_particles_deposit", "test_refined_grid", dict(K=4)),
    ("test_gpu_particles_moments", "test_refined_grid", dict(shape="cic", weight=6)),
    ("test_gpu_particles_boris", "test_bitwise_on_a_refined_grid", {}),
    ("test_gpu_particles_adapt", "test_refined_grid_three_rounds_with_steps", {}),
    ("test_gpu_particles_create", "test_bitwise_against_the_model", {}),
    ("test_gpu_particles_remove", "test_all_stages_against_the_model", {}),
    ("test_gpu_particles_reduce", "test_refined_grid", {}),
    ("test_gpu_pic_cycle", "test_three_cycles", {}),
]


def _replay_id(row):
    mod, name, kw = row
    return f"{mod[len('test_gpu_'):]}.{name[len('test_'):]}"


@pytest.mark.parametrize("row", REPLAYS, ids=_replay_id)
def test_replay(poison, gpu, monkeypatch, tmp_path, golden_dir, row):
    mod, name, kw = row
    m = importlib.import_module(mod)
    fn = getattr(m, name)
    passed = dict(gpu=gpu, monkeypatch=monkeypatch, tmp_path=tmp_path, golden_dir=golden_dir)
    args = dict(kw)
    with contextlib.ExitStack() as stack:
        for p in inspect.signature(fn).parameters:
            if p in args:
                continue
            if p in passed:
                args[p] = passed[p]
            elif p == "nbrec_on":  # test_gpu_advection's fixture: the switch it sets
                monkeypatch.setenv("DCCRGX_NBREC", "1")
                args[p] = None
            else:
                # a fixture of that module that builds its case from `gpu`: built
                # here, under the knob, and torn down after the call
                fixture = getattr(m, p)
                make = contextlib.contextmanager(getattr(fixture, "__wrapped__", fixture))
                assert list(inspect.signature(make).parameters) == ["gpu"], (mod, p)
                args[p] = stack.enter_context(make(gpu))
        fn(**args)
