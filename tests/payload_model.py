"""A byte model of the cell payload movers, in plain NumPy uint8 arrays.

Nothing here comes from the library under test: the rules are the ones
include/dccrgx.h documents.

* halo: the wire message of a neighborhood to one peer is, for each
  transferred fixed-size field in field order, bytes [win_off, win_off +
  win_len) of each listed cell in ascending id; the receiver writes exactly
  those bytes of its remote copies and nothing else.
* migration: every field in field order, whole elements, the moving cells in
  ascending id.
* rebuild (stop_refining / set_cells): a cell that stays keeps its bytes, a
  new child takes its parent's (a variable-size field: empty), a merged
  parent is all zero (variable-size: empty), and the removed children's
  payloads are kept aside in the order of get_removed_cells.
* the variable-size pool: per slot a byte string; resize keeps the leading
  min(old, new) bytes and zeroes the rest; a slot range is uploaded and
  downloaded as the concatenation of its cells.

A field is a FieldSpec; a rank's view of the fields is a list with one
(n_slots, elem) uint8 array per field (slots: the local cells, then the
remote copies), and `slot_of_id` maps a cell id to its slot in that view.
"""
from collections import namedtuple

import numpy as np

FieldSpec = namedtuple("FieldSpec", "elem transfer win_off win_len")


def field(elem, transfer=True, window=None):
    """A FieldSpec; `window` = (offset, length), None = the whole element."""
    off, ln = (0, elem) if window is None else window
    if not (ln > 0 and off >= 0 and off + ln <= elem):
        raise ValueError("window outside the element")
    return FieldSpec(int(elem), bool(transfer), int(off), int(ln))


def bytes_per_cell(fields):
    """Halo bytes of one cell: the windows of the transferred fields."""
    return sum(f.win_len for f in fields if f.transfer)


def _slots(ids, slot_of_id):
    ids = [int(c) for c in ids]
    if any(a >= b for a, b in zip(ids, ids[1:])):
        raise ValueError("cell lists are strictly ascending in id")
    return np.array([slot_of_id[c] for c in ids], np.int64)


def halo_message(fields, bytes_of_rank, send_ids, slot_of_id):
    """The sender's wire message for the cells `send_ids` (ascending)."""
    sl = _slots(send_ids, slot_of_id)
    parts = []
    for f, b in zip(fields, bytes_of_rank):
        assert b.dtype == np.uint8 and b.ndim == 2 and b.shape[1] == f.elem
        if f.transfer:
            parts.append(b[sl, f.win_off:f.win_off + f.win_len].reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def halo_place(fields, bytes_of_rank, recv_ids, slot_of_id, message):
    """The receiver's view after placing `message` (the sender's
    halo_message for the same cells): a new list of arrays in which only the
    window bytes of the listed cells' slots differ from `bytes_of_rank`."""
    sl = _slots(recv_ids, slot_of_id)
    message = np.asarray(message, np.uint8).reshape(-1)
    if message.size != sl.size * bytes_per_cell(fields):
        raise ValueError("halo message has the wrong size")
    out, o = [], 0
    for f, b in zip(fields, bytes_of_rank):
        b = b.copy()
        if f.transfer:
            n = sl.size * f.win_len
            b[sl, f.win_off:f.win_off + f.win_len] = message[o:o + n].reshape(sl.size, f.win_len)
            o += n
        out.append(b)
    return out


def migration_message(fields, bytes_of_rank, moving_ids, slot_of_id):
    """Every field in field order, whole elements, cells in ascending id
    (transfer flags and windows play no part)."""
    sl = _slots(moving_ids, slot_of_id)
    parts = [b[sl].reshape(-1) for f, b in zip(fields, bytes_of_rank)]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def migration_place(fields, bytes_of_rank, arriving_ids, slot_of_id, message):
    """Inverse of migration_message on the new owner."""
    sl = _slots(arriving_ids, slot_of_id)
    message = np.asarray(message, np.uint8).reshape(-1)
    if message.size != sl.size * sum(f.elem for f in fields):
        raise ValueError("migration message has the wrong size")
    out, o = [], 0
    for f, b in zip(fields, bytes_of_rank):
        b = b.copy()
        n = sl.size * f.elem
        b[sl] = message[o:o + n].reshape(sl.size, f.elem)
        o += n
        out.append(b)
    return out


def rebuild(old_ids, old_bytes, new_ids, parent_of, removed_ids=()):
    """The carry of one field through a rebuild of the local cells.

    `old_bytes`: an (n_old, elem) array (fixed-size field) or a list of 1-D
    arrays (variable-size field), one entry per cell of `old_ids`;
    `parent_of`: id -> parent id (the id itself at level 0).  Returns
    (new_bytes, removed): the payload per cell of `new_ids`, and the old
    payloads of `removed_ids` in that order."""
    old_pos = {int(c): i for i, c in enumerate(old_ids)}
    variable = isinstance(old_bytes, (list, tuple))
    if variable:
        new = []
    else:
        new = np.zeros((len(new_ids), old_bytes.shape[1]), np.uint8)
    for i, c in enumerate(int(c) for c in new_ids):
        p = int(parent_of[c])
        if c in old_pos:  # stays
            src = old_pos[c]
        elif p != c and p in old_pos:  # a new child
            src = None if variable else old_pos[p]
        else:  # a merged parent
            src = None
        if variable:
            new.append(old_bytes[src].copy() if src is not None else np.zeros(0, np.uint8))
        elif src is not None:
            new[i] = old_bytes[src]
    rem = [old_bytes[old_pos[int(c)]] for c in removed_ids]
    if variable:
        return new, [r.copy() for r in rem]
    return new, (np.array(rem, np.uint8).reshape(len(rem), old_bytes.shape[1]))


# ---- the variable-size pool: a list of 1-D uint8 arrays, one per slot
def pool_sizes(cells, slot0=0, n=None):
    n = len(cells) - slot0 if n is None else n
    return np.array([cells[slot0 + i].size for i in range(n)], np.uint64)


def pool_offsets(cells):
    """Byte offset of every slot in the pool (n + 1 entries)."""
    return np.concatenate([[0], np.cumsum([c.size for c in cells])]).astype(np.uint64)


def pool_resize(cells, new_sizes, slot0=0):
    """The cells from slot0 on take `new_sizes`: the first min(old, new)
    bytes kept, the rest zero; every other slot as it was."""
    out = [c.copy() for c in cells]
    for i, s in enumerate(int(s) for s in new_sizes):
        c = np.zeros(s, np.uint8)
        k = min(s, cells[slot0 + i].size)
        c[:k] = cells[slot0 + i][:k]
        out[slot0 + i] = c
    return out


def pool_download(cells, slot0=0, n=None):
    """The concatenated bytes of slots [slot0, slot0 + n)."""
    n = len(cells) - slot0 if n is None else n
    parts = [cells[slot0 + i] for i in range(n)]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def pool_upload(cells, raw, slot0, n):
    """Slots [slot0, slot0 + n) take the concatenated bytes `raw`, split by
    their current sizes."""
    raw = np.asarray(raw, np.uint8).reshape(-1)
    if raw.size != int(pool_sizes(cells, slot0, n).sum()):
        raise ValueError("byte count differs from the cells' sizes")
    out = [c.copy() for c in cells]
    o = 0
    for i in range(n):
        k = cells[slot0 + i].size
        out[slot0 + i] = raw[o:o + k].copy()
        o += k
    return out


resize, download, upload = pool_resize, pool_download, pool_upload


def pool_set(cells, values, slot0=0):
    """VariableField.set: resize to the values' sizes, then upload them."""
    values = [np.asarray(v, np.uint8).reshape(-1) for v in values]
    out = pool_resize(cells, [v.size for v in values], slot0)
    raw = np.concatenate(values) if values else np.zeros(0, np.uint8)
    return pool_upload(out, raw, slot0, len(values))
