"""The byte model of the payload movers (tests/payload_model.py) against
hand-written bytes and against its own invariants on the oracle's per-rank
views: what tests/test_gpu_payload_bytes.py holds the library to must itself
be right.  No GPU."""
import numpy as np
import pytest

import payload_model as PM
from helpers import random_refines

U8 = np.uint8


def test_hand_written_two_cells_two_fields():
    """Two cells, two fields, every byte written out: field 0 is 3 bytes with
    the window (1, 2), field 1 is 2 bytes, whole.  Cell 5 sits in slot 1 and
    cell 9 in slot 0, so ascending id is not ascending slot."""
    fields = [PM.field(3, True, (1, 2)), PM.field(2)]
    view = [np.array([[10, 11, 12], [20, 21, 22]], U8), np.array([[30, 31], [40, 41]], U8)]
    slot = {5: 1, 9: 0}
    msg = PM.halo_message(fields, view, [5, 9], slot)
    assert msg.tolist() == [21, 22, 11, 12, 40, 41, 30, 31]
    assert PM.halo_message(fields, view, [9], slot).tolist() == [11, 12, 30, 31]
    assert PM.migration_message(fields, view, [5, 9], slot).tolist() == [20, 21, 22, 10, 11, 12, 40, 41, 30, 31]
    # the receiver: three slots, cells 5 and 9 are its remote copies at slots 2 and 1
    recv = [np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], U8), np.array([[50, 51], [60, 61], [70, 71]], U8)]
    keep = [b.copy() for b in recv]
    out = PM.halo_place(fields, recv, [5, 9], {5: 2, 9: 1, 77: 0}, msg)
    assert out[0].tolist() == [[1, 2, 3], [4, 11, 12], [7, 21, 22]]
    assert out[1].tolist() == [[50, 51], [30, 31], [40, 41]]
    assert all(np.array_equal(a, b) for a, b in zip(recv, keep))  # the input is not written
    # a field left out of the transfer leaves the message and stays put
    off = [fields[0], fields[1]._replace(transfer=False)]
    m2 = PM.halo_message(off, view, [5, 9], slot)
    assert m2.tolist() == [21, 22, 11, 12]
    out = PM.halo_place(off, recv, [5, 9], {5: 2, 9: 1}, m2)
    assert np.array_equal(out[1], recv[1])
    with pytest.raises(ValueError):
        PM.halo_place(fields, recv, [5, 9], {5: 2, 9: 1}, msg[:-1])
    with pytest.raises(ValueError):
        PM.halo_message(fields, view, [9, 5], slot)  # not ascending
    with pytest.raises(ValueError):
        PM.field(24, True, (20, 5))
    mig = PM.migration_place(fields, recv, [5, 9], {5: 2, 9: 1}, PM.migration_message(fields, view, [5, 9], slot))
    assert mig[0].tolist() == [[1, 2, 3], [10, 11, 12], [20, 21, 22]]
    assert mig[1].tolist() == [[50, 51], [30, 31], [40, 41]]


def test_hand_written_rebuild():
    """Cells 1, 2, 3 and the children 10..17 of a cell 4: 2 is refined into
    20..27, the family of 4 merges.  Stayers keep, children copy the parent
    (empty for a variable field), the merged parent is zero / empty, removed
    payloads come back in the order asked for."""
    old_ids = [1, 2, 3] + list(range(10, 18))
    old = np.arange(11 * 2, dtype=U8).reshape(11, 2) + 1
    new_ids = [3, 1, 4] + list(range(20, 28))
    parent = {1: 1, 3: 3, 4: 4, **{c: 2 for c in range(20, 28)}}
    removed = [17, 10, 12]
    new, rem = PM.rebuild(old_ids, old, new_ids, parent, removed)
    assert new[0].tolist() == [5, 6] and new[1].tolist() == [1, 2]
    assert new[2].tolist() == [0, 0]
    assert all(row.tolist() == [3, 4] for row in new[3:])
    assert rem.tolist() == [[21, 22], [7, 8], [11, 12]]
    var = [np.full(i % 4, i, U8) for i in range(11)]
    new, rem = PM.rebuild(old_ids, var, new_ids, parent, removed)
    assert new[0].tolist() == [2, 2] and new[1].tolist() == []
    assert all(a.size == 0 for a in new[2:])
    assert [r.tolist() for r in rem] == [[10, 10], [3, 3, 3], [5]]


def test_hand_written_pool():
    cells = [np.array([1, 2, 3], U8), np.zeros(0, U8), np.array([4], U8), np.array([5, 6], U8)]
    assert PM.pool_sizes(cells).tolist() == [3, 0, 1, 2]
    assert PM.pool_offsets(cells).tolist() == [0, 3, 3, 4, 6]
    assert PM.pool_download(cells).tolist() == [1, 2, 3, 4, 5, 6]
    assert PM.pool_download(cells, 1, 2).tolist() == [4]
    r = PM.pool_resize(cells, [2, 0, 3], slot0=1)  # grow, to zero, grow
    assert [c.tolist() for c in r] == [[1, 2, 3], [0, 0], [], [5, 6, 0]]
    r = PM.pool_resize(cells, [1])  # shrink
    assert [c.tolist() for c in r] == [[1], [], [4], [5, 6]]
    u = PM.pool_upload(cells, [9, 8, 7], 2, 2)
    assert [c.tolist() for c in u] == [[1, 2, 3], [], [9], [8, 7]]
    with pytest.raises(ValueError):
        PM.pool_upload(cells, [9, 8], 2, 2)
    s = PM.pool_set(cells, [[7, 7], [6]], slot0=1)
    assert [c.tolist() for c in s] == [[1, 2, 3], [7, 7], [6], [5, 6]]
    assert [c.tolist() for c in cells] == [[1, 2, 3], [], [4], [5, 6]]


FIELDS = [PM.field(1), PM.field(4), PM.field(2, False), PM.field(8, True, (4, 4)), PM.field(3, True, (1, 1)),
          PM.field(24, True, (23, 1))]


@pytest.fixture(scope="module")
def rank_views():
    """The oracle's per-rank views of a refined (6, 6, 6) grid, R = 2, on 3
    processes, every slot of every field filled with its own random bytes."""
    from oracle import oracle as O

    P = 3
    o = O.Grid((6, 6, 6), 2, (True, False, True), 1, P)
    rng = np.random.default_rng(7)
    for _ in range(2):
        ids, _ = o.cells()
        for c in random_refines(ids, o.mapping.batch(ids)["level"], 2, rng, 0.15):
            o.refine_completely(c)
        o.stop_refining()
    views = []
    for r in range(P):
        loc, rem = o.rank_cells(r, "local"), o.rank_cells(r, "remote_bdy")
        ids = np.concatenate([loc, rem])
        slot = {int(c): i for i, c in enumerate(ids)}
        data = [rng.integers(0, 256, (ids.size, f.elem), dtype=U8) for f in FIELDS]
        views.append((loc.size, slot, data))
    return o, P, views


def test_round_trip_on_oracle_views(rank_views):
    """Pack on every sender, place on every receiver: each remote copy's
    window bytes are its owner's, every byte outside a window and every local
    slot is what it was; a message is n_send x sum(win_len) bytes."""
    o, P, views = rank_views
    bpc = 1 + 4 + 4 + 1 + 1
    assert PM.bytes_per_cell(FIELDS) == bpc
    after = [[b.copy() for b in v[2]] for v in views]
    touched = [[np.zeros(b.shape, bool) for b in v[2]] for v in views]
    n_placed = 0
    for r in range(P):
        for p in range(P):
            if p == r:
                continue
            send = o.cells_to_send(r, p)
            assert np.array_equal(send, o.cells_to_receive(p, r))
            msg = PM.halo_message(FIELDS, views[r][2], send, views[r][1])
            assert msg.size == send.size * bpc
            after[p] = PM.halo_place(FIELDS, after[p], send, views[p][1], msg)
            for c in send.tolist():
                assert views[r][1][c] < views[r][0]  # sent cells are local to the sender
                s = views[p][1][c]
                assert s >= views[p][0]  # and remote copies on the receiver
                for k, f in enumerate(FIELDS):
                    if f.transfer:
                        touched[p][k][s, f.win_off:f.win_off + f.win_len] = True
                        own = views[r][2][k][views[r][1][c]]
                        assert np.array_equal(after[p][k][s, f.win_off:f.win_off + f.win_len],
                                              own[f.win_off:f.win_off + f.win_len])
            n_placed += send.size
    assert n_placed > 100
    for p in range(P):
        nl = views[p][0]
        for k, f in enumerate(FIELDS):
            before, got = views[p][2][k], after[p][k]
            assert np.array_equal(got[~touched[p][k]], before[~touched[p][k]])
            assert np.array_equal(got[:nl], before[:nl])
            assert not touched[p][k][:nl].any()
            if not f.transfer:
                assert np.array_equal(got, before)
        # every remote copy is in some peer's list: its windows were all written
        assert all(touched[p][k][nl:, f.win_off:f.win_off + f.win_len].all() for k, f in enumerate(FIELDS) if f.transfer)


def test_pair_without_shared_cells_is_empty():
    """(10, 1, 1) on 4 processes, not periodic: ranks 0 and 2 are not
    neighbors, their message is empty and placing it changes nothing."""
    from oracle import oracle as O

    o = O.Grid((10, 1, 1), 0, (False, False, False), 1, 4)
    assert o.cells_to_send(0, 2).size == 0 and o.cells_to_receive(2, 0).size == 0
    assert o.cells_to_send(0, 1).size > 0
    loc = o.rank_cells(0, "local")
    slot = {int(c): i for i, c in enumerate(loc)}
    data = [np.full((loc.size, f.elem), 7, U8) for f in FIELDS]
    msg = PM.halo_message(FIELDS, data, o.cells_to_send(0, 2), slot)
    assert msg.size == 0 and msg.dtype == U8
    out = PM.halo_place(FIELDS, data, o.cells_to_receive(0, 2), slot, msg)
    assert all(np.array_equal(a, b) for a, b in zip(out, data))
