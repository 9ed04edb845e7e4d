"""The cell payload movers against a byte model (tests/payload_model.py),
bitwise: the halo pack and place, the carry of payloads through a rebuild,
the removed-cell store, the variable-size pool and the migration, at every
element size and window the dispatchers tell apart:

  k_pack / k_place   uint32_t / uint64_t only for a whole 4- / 8-byte element,
                     pack_bytes_kernel / place_bytes_kernel for everything else
  k_gather_rows      4, 8 and 16 (uint4) bytes typed, gather_bytes_kernel else
  wave_copy          4-byte words when both addresses and the length are
                     multiples of 4, one byte per lane else

and past the first pass of their grid-stride loops.  Send and receive lists
come from the oracle, never from the library under test; slots are the
library's (slot_ids), which is all a caller knows of them."""
import numpy as np
import pytest

import payload_model as PM
from helpers import make_pair

pytestmark = pytest.mark.gpu

U8 = np.uint8

# name, element bytes, transferred, window (offset, length; None = the element)
FIELD_SET = [
    ("a", 1, True, None),  # bytes path, the smallest element
    ("b", 4, True, None),  # uint32_t fast path
    ("c", 2, False, None),  # must never move in a halo
    ("d", 8, True, None),  # uint64_t fast path
    ("e", 8, True, (0, 4)),  # bytes path: len < elem at offset 0
    ("f", 8, True, (4, 4)),  # bytes path: off > 0
    ("g", 3, True, (1, 1)),  # odd element, its middle byte
    ("h", 12, True, (4, 8)),
    ("i", 16, True, None),  # uint4 gather in rebuilds
    ("j", 24, True, (23, 1)),  # the last byte only
]
SIZES = [0, 1, 2, 3, 5, 7, 8, 255, 256, 257, 1000]  # variable payloads: misaligned offsets, several wave strides


def bytes_dtype(elem):
    return np.dtype((U8, (elem,)))


def add_fields(g, spec=FIELD_SET):
    out = []
    for name, elem, transfer, win in spec:
        f = g.add_field(name, bytes_dtype(elem), transfer)
        if win is not None:
            f.set_window(*win)
        out.append(f)
    return out


def model_fields(spec=FIELD_SET):
    return [PM.field(elem, transfer, win) for _, elem, transfer, win in spec]


def fill(g, fs, rng):
    """Random bytes into every slot of every field, remote copies included
    (they start stale, so an untouched byte is told from a delivered one)."""
    n = g.n_slots
    data = [rng.integers(0, 256, (n, f.dtype.itemsize), dtype=U8) for f in fs]
    for f, d in zip(fs, data):
        f.set(d)
    return data


def read(g, fs):
    return [f.get().reshape(g.n_slots, f.dtype.itemsize) for f in fs]


def slot_map(g):
    ids = g.slot_ids()
    assert ids.size == g.n_slots
    return {int(c): s for s, c in enumerate(ids)}


def exchange_and_check(gs, fss, mf, send_list, rng, hood=None):
    """One halo update between detached views, by halo_message_size /
    halo_pack / halo_place, checked at every step.  `send_list(r, p)`: the
    oracle's ids r sends to p.  Returns {(r, p): message bytes}."""
    from dccrg_amd.grid import DEFAULT_HOOD

    hood = DEFAULT_HOOD if hood is None else hood
    P = len(gs)
    slot = [slot_map(g) for g in gs]
    before = [fill(g, fs, rng) for g, fs in zip(gs, fss)]
    bpc = PM.bytes_per_cell(mf)
    pairs = [(r, p) for r in range(P) for p in range(P) if p != r]
    msgs = {}
    for r, p in pairs:
        ids = send_list(r, p)
        sb, rb = gs[r].halo_message_size(p, hood)
        assert (sb, rb) == tuple(reversed(gs[p].halo_message_size(r, hood))), (r, p)  # both ends agree
        assert sb == len(ids) * bpc, (r, p)
        m = gs[r].halo_pack(p, hood).copy()
        exp = PM.halo_message(mf, before[r], ids, slot[r])
        assert m.size == exp.size and np.array_equal(m, exp), (r, p)
        msgs[(r, p)] = m
    expect = [[b.copy() for b in v] for v in before]
    for (r, p), m in msgs.items():
        gs[p].halo_place(r, m, hood)
        expect[p] = PM.halo_place(mf, expect[p], send_list(r, p), slot[p], m)
    after = [read(g, fs) for g, fs in zip(gs, fss)]
    touched = [[np.zeros(b.shape, bool) for b in v] for v in before]
    for r, p in pairs:
        ids = [int(c) for c in send_list(r, p)]
        sr = np.array([slot[r][c] for c in ids], np.int64)
        sp = np.array([slot[p][c] for c in ids], np.int64)
        assert np.all(sr < gs[r].n_local) and np.all(sp >= gs[p].n_local)
        for k, f in enumerate(mf):
            if not f.transfer:
                continue
            w = slice(f.win_off, f.win_off + f.win_len)
            # each remote copy's window bytes are its owner's
            assert np.array_equal(after[p][k][sp, w], before[r][k][sr, w]), (r, p, k)
            touched[p][k][sp, w] = True
    for p in range(P):
        for k, f in enumerate(mf):
            # every other byte of every slot of every field is what it was
            assert np.array_equal(after[p][k][~touched[p][k]], before[p][k][~touched[p][k]]), (p, k)
            assert np.array_equal(after[p][k], expect[p][k]), (p, k)
            if not f.transfer:
                assert np.array_equal(after[p][k], before[p][k]), (p, k)
    return msgs


def refined_views():
    from test_gpu_multirank import views

    return views((6, 6, 6), 2, (True, False, True), 1, 3, rounds=2, frac=0.15, seed=7)


def test_halo_every_branch_and_window_changes(gpu):
    """k_pack / k_place on detached views: the uint32_t and uint64_t fast
    paths (b, d) next to pack_bytes_kernel / place_bytes_kernel with len <
    elem at offset 0 (e), off > 0 (f, h), an odd element's middle byte (g),
    the last byte of 24 (j) and a 1-byte element (a), in one plan, so a wrong
    offset, elem used for len, or a misplaced field segment of plan_layout
    shows in the message or in a byte outside a window.  The windows then
    change between exchanges as the facade's sync_window changes them (a
    2-byte whole element joins, a window one byte short of its element at
    offset 1 and at offset 0).  A refined (6, 6, 6) grid on 3 processes is
    the issue's shape: every ordered pair exchanges 150 to 210 cells of three
    levels, a few blocks of the byte kernels, at about 2000 cells in all."""
    import dccrg_amd

    gs, o = refined_views()
    rng = np.random.default_rng(101)
    spec = list(FIELD_SET)
    fss = [add_fields(g, spec) for g in gs]
    names = [s[0] for s in spec]

    def send_list(r, p):
        return o.cells_to_send(r, p)

    for r in range(3):
        for p in range(3):
            if p != r:
                assert np.array_equal(o.cells_to_send(r, p), o.cells_to_receive(p, r))
    m1 = exchange_and_check(gs, fss, model_fields(spec), send_list, rng)
    assert PM.bytes_per_cell(model_fields(spec)) == 47
    assert all(m.size == 47 * send_list(r, p).size for (r, p), m in m1.items())
    assert min(m.size for m in m1.values()) > 47 * 50

    # refusals: a message one byte short, a window past the element
    state = [read(g, fs) for g, fs in zip(gs, fss)]
    with pytest.raises(dccrg_amd.DccrgError):
        gs[1].halo_place(0, m1[(0, 1)][:-1])
    with pytest.raises(dccrg_amd.DccrgError):
        fss[0][names.index("j")].set_window(20, 5)
    for g, fs, st in zip(gs, fss, state):
        assert all(np.array_equal(a, b) for a, b in zip(read(g, fs), st))

    def change(name, transfer=None, window=None):
        k = names.index(name)
        n, elem, t, w = spec[k]
        spec[k] = (n, elem, t if transfer is None else transfer, w if window is None else window)
        for fs in fss:
            if transfer is not None:
                fs[k].set_transfer(transfer)
            if window is not None:
                fs[k].set_window(*window)

    change("e", window=(2, 5))
    change("d", transfer=False)
    change("c", transfer=True)
    m2 = exchange_and_check(gs, fss, model_fields(spec), send_list, rng)
    assert PM.bytes_per_cell(model_fields(spec)) == 47 + 1 - 8 + 2
    assert all(m.size == 42 * send_list(r, p).size for (r, p), m in m2.items())

    # windows one byte short of the element: i / len and i / elem part ways late
    change("h", window=(1, 11))
    change("j", window=(0, 23))
    m3 = exchange_and_check(gs, fss, model_fields(spec), send_list, rng)
    assert all(m.size == (42 - 8 + 11 - 1 + 23) * send_list(r, p).size for (r, p), m in m3.items())
    for g in gs:
        g.close()


def test_halo_empty_pairs_on_a_line(gpu):
    """(10, 1, 1) on 4 processes, not periodic: a message is one cell (n = 1,
    the smallest launch of every pack / place branch) and ranks 0 and 2 share
    nothing, so their message is empty on both ends (k_pack / k_place with n
    = 0 launch nothing, the size check still holds)."""
    from test_gpu_multirank import views

    gs, o = views((10, 1, 1), 0, (False, False, False), 1, 4)
    fss = [add_fields(g) for g in gs]
    assert o.cells_to_send(0, 2).size == 0 and o.cells_to_send(2, 0).size == 0
    msgs = exchange_and_check(gs, fss, model_fields(), lambda r, p: o.cells_to_send(r, p), np.random.default_rng(5))
    assert msgs[(0, 2)].size == 0 and msgs[(2, 0)].size == 0 and msgs[(0, 3)].size == 0
    assert msgs[(0, 1)].size == 47 and msgs[(1, 2)].size == 47
    for g in gs:
        g.close()


def test_halo_user_neighborhood(gpu):
    """The same fields through a user neighborhood of 3 random offsets: the
    non-direct plan (its own send / receive slot lists, a strict subset of
    the default ones), so pack and place index through a plan whose receive
    slots are no contiguous run.  Lists: the oracle's neighbors_of_hood.  The
    grid is the first test's, the smallest here with mixed levels on three
    ranks, so both plans are held to the model on one mesh."""
    from test_gpu_user_hood import random_hood

    gs, o = refined_views()
    P = len(gs)
    hood = random_hood(np.random.default_rng(4), 1, 3)
    for g in gs:
        assert g.add_neighborhood(3, hood)
    fss = [add_fields(g) for g in gs]
    ids, owners = o.cells()
    owner = dict(zip(ids.tolist(), owners.tolist()))
    recv = {}
    for c in ids.tolist():
        nid, _ = o.neighbors_of_hood(c, hood)
        for n in nid.tolist():
            if owner[n] != owner[c]:
                recv.setdefault((owner[c], owner[n]), set()).add(n)

    def send_list(r, p):  # what p receives from r
        return np.array(sorted(recv.get((p, r), ())), np.uint64)

    strict = 0
    for r in range(P):
        for p in range(P):
            if p != r:
                d = set(o.cells_to_send(r, p).tolist())
                assert set(send_list(r, p).tolist()) <= d
                strict += set(send_list(r, p).tolist()) < d
    assert strict > 0
    msgs = exchange_and_check(gs, fss, model_fields(), send_list, np.random.default_rng(6), hood=3)
    assert sum(m.size for m in msgs.values()) > 0
    # and the default plan still moves its own, larger lists
    exchange_and_check(gs, fss, model_fields(), lambda r, p: o.cells_to_send(r, p), np.random.default_rng(8))
    for g in gs:
        g.close()


def test_halo_second_pass_of_the_grid_stride_loop(gpu):
    """pack_bytes_kernel / place_bytes_kernel past their first pass: grid_for
    caps a launch at 8192 blocks of 256 threads = 2 097 152, one per message
    byte.  (64, 64, 4) on 2 processes, periodic in z only, sends both planes
    of each rank (8192 cells); one whole 264-byte field makes 2 162 688 bytes,
    65 536 more than the cap.  At neighborhood length 1 no smaller grid gives
    a rank 8192 cells to send with fewer slots (about 4 MB per view)."""
    from test_gpu_multirank import views

    gs, o = views((64, 64, 4), 0, (False, False, True), 1, 2)
    spec = [("w", 264, True, None)]
    fss = [add_fields(g, spec) for g in gs]
    msgs = exchange_and_check(gs, fss, model_fields(spec), lambda r, p: o.cells_to_send(r, p),
                              np.random.default_rng(9))
    assert o.cells_to_send(0, 1).size == 8192
    assert msgs[(0, 1)].size == 2162688 > 8192 * 256 and msgs[(1, 0)].size == 2162688
    for g in gs:
        g.close()


def _refine_some(g, o, ids):
    req = [int(c) for c in sorted(ids.tolist()) if int(c) % 3 == 0]
    for c in req:
        assert g.refine_completely(c)
        o.refine_completely(c)
    new = g.stop_refining()
    o.stop_refining()
    assert new.size == 8 * len(req) and len(req) >= 8
    return req


def _unrefine_all(g, o, ids):
    lv = o.mapping.batch(ids)["level"]
    for c in ids[lv == 1].tolist():
        g.unrefine_completely(c)
        o.unrefine_completely(c)
    g.stop_refining()
    o.stop_refining()


def _parents(o, ids):
    return dict(zip(ids.tolist(), o.mapping.batch(ids)["parent"].tolist()))


def test_rebuild_carry_and_removed_store(gpu):
    """k_gather_rows through stop_refining and set_cells on one rank, every
    element size of FIELD_SET: the typed rows of 4, 8 and 16 (uint4) bytes
    and gather_bytes_kernel for 1, 2, 3, 12 and 24; then the removed-cell
    store (k_pack of whole elements, bytes path for all but 4 and 8).  A
    (4, 4, 2) grid with a third of its cells refined has stayers, children
    and, after the unrefinement, merged parents side by side; the kernels
    index by slot and by byte only, so 32 cells reach all they can do."""
    g, o = make_pair((4, 4, 2), 1)
    fs = add_fields(g)
    rng = np.random.default_rng(21)
    assert g.n_slots == g.n_local == 32
    # 1. refine a third: children hold their parent's bytes, stayers theirs
    ids0 = g.slot_ids()
    old = fill(g, fs, rng)
    req = _refine_some(g, o, ids0)
    ids1 = g.slot_ids()
    assert np.array_equal(np.sort(ids1), o.cells()[0])
    got = read(g, fs)
    par = _parents(o, ids1)
    pos0 = {int(c): s for s, c in enumerate(ids0)}
    for k, f in enumerate(fs):
        exp, _ = PM.rebuild(ids0, old[k], ids1, par)
        assert np.array_equal(got[k], exp), f.name
        for s, c in enumerate(ids1.tolist()):
            src = pos0[c] if c in pos0 else pos0[par[c]]
            assert np.array_equal(got[k][s], old[k][src]), (f.name, c)
    # 2. unrefine every family: removed payloads, merged parents zero
    old = fill(g, fs, rng)
    _unrefine_all(g, o, ids1)
    removed = g.get_removed_cells()
    assert np.array_equal(np.sort(removed), o.removed()[0]) and removed.size == 8 * len(req)
    ids2 = g.slot_ids()
    assert np.array_equal(np.sort(ids2), np.sort(ids0))
    got = read(g, fs)
    par = _parents(o, ids2)
    pos1 = {int(c): s for s, c in enumerate(ids1)}
    pos2 = {int(c): s for s, c in enumerate(ids2)}
    for k, f in enumerate(fs):
        exp, rem = PM.rebuild(ids1, old[k], ids2, par, removed)
        assert np.array_equal(got[k], exp), f.name
        assert np.array_equal(f.get_removed().reshape(removed.size, -1), rem), f.name
        assert np.array_equal(rem, old[k][[pos1[int(c)] for c in removed]])
        assert not got[k][[pos2[c] for c in req]].any(), f.name
    # 3. set_cells with the same leaves and owners keeps every byte
    old = fill(g, fs, rng)
    g.set_cells(np.sort(ids2), np.zeros(ids2.size, np.int32))
    ids3 = g.slot_ids()
    assert np.array_equal(np.sort(ids3), np.sort(ids2))
    got = read(g, fs)
    for k, f in enumerate(fs):
        exp, _ = PM.rebuild(ids2, old[k], ids3, par)
        assert np.array_equal(got[k], exp), f.name
    g.close()


def _payload(rng, n):
    return rng.integers(0, 256, int(n), dtype=U8)


def _check_pool(v, model):
    n = len(model)
    assert np.array_equal(v.sizes(0, n), PM.pool_sizes(model))
    got = v.get(0, n)
    assert len(got) == n
    for s, (a, b) in enumerate(zip(got, model)):
        assert a.dtype == U8 and np.array_equal(a, b), s


def test_variable_pool(gpu):
    """wave_copy's byte branch and its stride loop: uint8 payloads whose
    sizes cycle through 0, 1, 2, 3, 5, 7, 8, 255, 256, 257 and 1000 put the
    pool offsets off every 4-byte boundary (the word branch needs both
    addresses and the length aligned) and make a wave take up to 16 strides of
    64 lanes.  set / get of the whole range and of a middle range, sizes,
    resize (shrink, grow and to zero in one call), var_remap through
    stop_refining (children empty) and the removed store, all against the
    model.  32 cells hold every size three times, at different offsets."""
    g, o = make_pair((4, 4, 2), 1)
    v = g.add_variable_field("v", U8)
    rng = np.random.default_rng(31)
    n = g.n_slots
    empty = [np.zeros(0, U8)] * n
    _check_pool(v, empty)
    vals = [_payload(rng, SIZES[s % 11]) for s in range(n)]
    v.set(vals)
    model = PM.pool_set(empty, vals)
    _check_pool(v, model)
    assert any(int(x) % 4 for x in PM.pool_offsets(model))
    # a middle slot range: download, then upload with other sizes
    got = v.get(5, 13)
    assert all(np.array_equal(a, b) for a, b in zip(got, model[5:18])) and len(got) == 13
    assert np.array_equal(np.concatenate(got), PM.pool_download(model, 5, 13))
    assert np.array_equal(v.sizes(5, 13), PM.pool_sizes(model, 5, 13))
    mid = [_payload(rng, SIZES[(7 * s + 3) % 11]) for s in range(9)]
    v.set(mid, slot0=6)
    model = PM.pool_set(model, mid, 6)
    _check_pool(v, model)
    # resize: shrinking, growing and to zero in one call
    cur = PM.pool_sizes(model).tolist()
    new = [(c // 2, c + SIZES[(s + 4) % 11], 0)[s % 3] for s, c in enumerate(cur)]
    assert any(0 < a < b and b > 256 for a, b in zip(new, cur)) and any(a > b > 0 for a, b in zip(new, cur))
    v.resize(new)
    model = PM.pool_resize(model, new)
    _check_pool(v, model)
    # a resize of a middle range leaves the others alone
    v.resize([3, 0, 600], slot0=10)
    model = PM.pool_resize(model, [3, 0, 600], 10)
    _check_pool(v, model)
    # through a rebuild: stayers keep, children empty
    vals = [_payload(rng, SIZES[(s + 2) % 11]) for s in range(n)]
    v.set(vals)
    model = PM.pool_set(model, vals)
    ids0 = g.slot_ids()
    req = _refine_some(g, o, ids0)
    ids1 = g.slot_ids()
    model, _ = PM.rebuild(ids0, model, ids1, _parents(o, ids1))
    assert sum(a.size == 0 for a in model) >= 8 * len(req)
    _check_pool(v, model)
    # unrefine: the removed children's payloads, merged parents empty
    vals = [_payload(rng, SIZES[(s + 5) % 11]) for s in range(ids1.size)]
    v.set(vals)
    model = PM.pool_set(model, vals)
    _unrefine_all(g, o, ids1)
    removed = g.get_removed_cells()
    assert removed.size == 8 * len(req)
    ids2 = g.slot_ids()
    model, rem = PM.rebuild(ids1, model, ids2, _parents(o, ids2), removed)
    got = v.get_removed()
    assert len(got) == len(rem) and all(np.array_equal(a, b) for a, b in zip(got, rem))
    assert sum(r.size for r in rem) > 1000
    _check_pool(v, model)
    g.close()


def test_variable_pool_second_pass_of_the_wave_loop(gpu):
    """WAVE_LOOP past its first pass in var_resize_copy_kernel: wave_grid
    caps a launch at 8192 blocks of 4 waves = 32 768 waves, one per slot.
    (32, 32, 33) unrefined is 33 792 slots, the smallest box of that base
    above the cap; sizes id % 3 keep the pool at 33 KB."""
    import dccrg_amd

    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((32, 32, 33)).set_maximum_refinement_level(0)
    g.set_neighborhood_length(1).initialize()
    n = g.n_slots
    assert n == 33792 > 8192 * 4
    ids = g.slot_ids()
    v = g.add_variable_field("v", U8)
    rng = np.random.default_rng(41)
    raw = rng.integers(1, 256, 3 * n, dtype=U8)  # no zero byte: a byte not copied shows
    vals = [raw[3 * s:3 * s + int(c) % 3] for s, c in enumerate(ids.tolist())]
    v.set(vals)
    model = PM.pool_set([np.zeros(0, U8)] * n, vals)

    def check():
        assert np.array_equal(v.sizes(0, n), PM.pool_sizes(model))
        assert np.array_equal(np.concatenate(v.get(0, n)), PM.pool_download(model))

    check()
    for new in ([(int(c) + 1) % 3 for c in ids.tolist()], [2] * n, [1 + int(c) % 2 for c in ids.tolist()]):
        v.resize(new)
        model = PM.pool_resize(model, new)
        check()
    assert any(a.any() for a in model[32768:])  # copied bytes live in the second pass
    g.close()


# ---------------------------------------------------------------------------- two real processes
def sc_payload_bytes(rank, world):
    """Run in each of two processes over the host transport (see
    test_two_processes)."""
    from oracle import oracle as O
    from test_gpu_transport import _gather, _grid

    length, R, per, hood = (6, 5, 4), 1, (True, False, False), 1
    g = _grid(length, R, per, hood)
    o = O.Grid(length, R, per, hood, world)
    for c in g.local_cells().tolist():
        if c % 4 == 1:
            g.refine_completely(c)
    for c in o.cells()[0].tolist():
        if c % 4 == 1:
            o.refine_completely(c)
    g.stop_refining()
    o.stop_refining()
    res = {}
    part = _gather(g.local_cells())
    pid = np.concatenate(part)
    pown = np.concatenate([np.full(len(x), r, np.int32) for r, x in enumerate(part)])
    order = np.argsort(pid)
    oids, oown = o.cells()
    res["leaves"] = bool(np.array_equal(pid[order], oids) and np.array_equal(pown[order], oown))
    fs = add_fields(g)
    v = g.add_variable_field("v", U8, True)
    mf = model_fields()
    rng = np.random.default_rng(1000 + rank)

    def fill_all():
        """Every slot of every field; returns (fixed arrays, variable list,
        {id: (rows, variable bytes)} of the local cells of every rank)."""
        data = fill(g, fs, rng)
        sl = g.slot_ids()
        nl = g.n_local
        # remote copies start with stale sizes too
        var = [_payload(rng, SIZES[(int(c) + (0 if s < nl else 5)) % 11]) for s, c in enumerate(sl.tolist())]
        v.set(var)
        mine = {int(c): ([d[s].copy() for d in data], var[s]) for s, c in enumerate(sl[:nl].tolist())}
        owner = {}
        for d in _gather(mine):
            owner.update(d)
        return data, var, owner

    def halo_ok():
        data, var, owner = fill_all()
        slot = slot_map(g)
        nl = g.n_local
        g.update_copies_of_remote_neighbors()
        expect = [d.copy() for d in data]
        evar = list(var)
        n_recv = 0
        copies = True
        got = read(g, fs)
        gvar = v.get()
        for p in range(world):
            if p == rank:
                continue
            ids = o.cells_to_receive(rank, p)
            n_recv += ids.size
            pslot = {int(c): i for i, c in enumerate(ids)}
            pview = [np.array([owner[int(c)][0][k] for c in ids], U8).reshape(ids.size, f.elem)
                     for k, f in enumerate(mf)]
            expect = PM.halo_place(mf, expect, ids, slot, PM.halo_message(mf, pview, ids, pslot))
            for c in ids.tolist():
                s = slot[c]
                copies &= s >= nl
                evar[s] = owner[c][1]
                copies &= bool(np.array_equal(gvar[s], owner[c][1]))
                for k, f in enumerate(mf):
                    if f.transfer:
                        w = slice(f.win_off, f.win_off + f.win_len)
                        copies &= bool(np.array_equal(got[k][s, w], owner[c][0][k][w]))
        whole = all(np.array_equal(a, b) for a, b in zip(got, expect))
        whole &= len(gvar) == len(evar) and all(np.array_equal(a, b) for a, b in zip(gvar, evar))
        whole &= bool(np.array_equal(v.sizes(), np.array([a.size for a in evar], np.uint64)))
        return bool(copies and n_recv > 0), bool(whole)

    # 1. the library's own halo: full-window fields received in place next to
    # windowed ones placed from the buffer, whole messages and cell by cell
    g.set_send_single_cells(False)
    res["halo_copies"], res["halo_rest_untouched"] = halo_ok()
    g.set_send_single_cells(True)
    res["single_copies"], res["single_rest_untouched"] = halo_ok()
    g.set_send_single_cells(False)

    # 2. migration: whole elements of every field, c and the bytes outside windows too
    _, _, owner = fill_all()
    loc = g.local_cells()
    mv = loc[loc % np.uint64(3) == 0]
    g.balance_load_to(mv, np.full(mv.size, (rank + 1) % world, np.int32))
    sl = g.slot_ids()[: g.n_local].tolist()
    got = read(g, fs)
    gvar = v.get(0, g.n_local)
    ok = True
    for s, c in enumerate(sl):
        ok &= all(np.array_equal(got[k][s], owner[c][0][k]) for k in range(len(fs)))
        ok &= bool(np.array_equal(gvar[s], owner[c][1]))
    res["migrated"] = bool(ok)
    res["moved_in"] = any(_gather(bool(set(sl) - set(loc.tolist()))))

    # 3. unrefine families split across the processes: the removed payloads
    # of every element size reach the parent's process
    _, _, owner = fill_all()
    before = set(g.local_cells().tolist())
    for c in sorted(before):
        if g.get_refinement_level(c) == 1:
            g.unrefine_completely(c)
    g.stop_refining()
    removed = g.get_removed_cells().tolist()
    ok = True
    for k, f in enumerate(fs):
        exp = np.array([owner[c][0][k] for c in removed], U8).reshape(len(removed), mf[k].elem)
        ok &= bool(np.array_equal(f.get_removed().reshape(len(removed), -1), exp))
    res["removed_fixed"] = bool(ok)
    rem = v.get_removed()
    res["removed_variable"] = bool(len(rem) == len(removed) and
                                   all(np.array_equal(a, owner[c][1]) for a, c in zip(rem, removed)))
    res["merged"] = any(_gather(len(removed) > 0))
    res["remote_payload"] = any(_gather(any(c not in before for c in removed)))
    slot = slot_map(g)
    parents = set(g.mapping_batch(np.array(removed, np.uint64))["parent"].tolist()) if removed else set()
    got = read(g, fs)
    gvar = v.get()
    res["parents_zero"] = bool(all(not got[k][slot[p]].any() for p in parents for k in range(len(fs))) and
                               all(gvar[slot[p]].size == 0 for p in parents))
    g.close()
    return res


def test_two_processes(gpu, tmp_path):
    """The same fields and the uint8 variable field between two real
    processes over the host transport, on a refined (6, 5, 4) grid: the
    library's own halo with send_single_cells off and on (whole-element
    fields of the direct plan are received in place, windowed ones through
    the buffer and place_bytes_kernel; variable payloads by var_gather /
    var_scatter with misaligned offsets), balance_load_to of a third of the
    cells (k_pack / k_place of whole elements, every size) and the removed
    payloads of families split across the processes.  Two processes are the
    fewest with a peer; the grid is sc_variable's."""
    from test_gpu_transport import _run_group

    results = _run_group(2, tmp_path, names=["sc_payload_bytes"], module="test_gpu_payload_bytes")
    assert len(results.get("sc_payload_bytes", {})) == 2
    for rank, (kind, out) in sorted(results["sc_payload_bytes"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, val in out.items():
            assert val, f"rank {rank}: {k} failed ({out})"
