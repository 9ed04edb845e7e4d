"""The grow-and-relaunch collector of the mesh build (collect_sorted_unique,
dccrgx_prims.hpp): a kernel appends ids to a list of a first capacity, and
when the count read back exceeds it the kernel runs once more with room for
that count.  k_induced_refines (first capacity 16 n + 1024) and k_ghost_level0
(2^22) share it, and neither fills its first capacity on a test-sized mesh, so
DCCRGX_APPEND_CAP=1 forces the second launch here.

* One rank, 8 x 8 x 8, two levels, periodic in x: a level-0 cell is refined,
  then the child in its (+x, +y, +z) corner, which touches level-0 cells, so
  the closure induces their refinement (more than one id: the second launch
  runs).  Cells, created cells and the neighbors_of rows equal the default
  run's exactly.
* A detached two-rank view cannot run stop_refining (it needs a
  communicator, test_gpu_balance.py), but its known-leaf query writes out the
  initial mesh's ghost ring through k_ghost_level0: ids and owners equal the
  default run's exactly, for both ranks."""
import numpy as np
import pytest

import dccrg_amd

pytestmark = pytest.mark.gpu

BASE = (8, 8, 8)


def _grid(rank=0, size=1):
    g = dccrg_amd.Dccrg(rank, size, 0).set_initial_length(BASE).set_neighborhood_length(1)
    g.set_maximum_refinement_level(2).set_periodic(True, False, False).initialize()
    return g


def _refine_twice():
    g = _grid()
    cell = 1 + 3 + 3 * BASE[0] + 3 * BASE[0] * BASE[1]  # level-0 cell (3, 3, 3)
    assert g.refine_completely(cell)
    first = g.stop_refining()
    assert first.size == 8
    assert g.refine_completely(int(np.max(first)))  # the (+x, +y, +z) child
    second = g.stop_refining()
    out = dict(first=first, second=second, cells=g.get_cells(), of=g.csr("of"))
    g.close()
    return out


def test_induced_refines_second_launch_same_mesh(gpu, monkeypatch):
    monkeypatch.delenv("DCCRGX_APPEND_CAP", raising=False)
    a = _refine_twice()
    monkeypatch.setenv("DCCRGX_APPEND_CAP", "1")
    b = _refine_twice()
    monkeypatch.delenv("DCCRGX_APPEND_CAP", raising=False)
    # the child's own 8 children and those of the induced level-0 cells: the
    # closure emitted more ids than the forced capacity of 1
    assert a["second"].size > 8 and a["second"].size % 8 == 0
    # every refined cell is replaced by its 8 children
    assert a["cells"].size == int(np.prod(BASE)) + 7 * (1 + a["second"].size // 8)
    for k in ("first", "second", "cells"):
        assert np.array_equal(a[k], b[k]), k
    for x, y in zip(a["of"], b["of"]):
        assert np.array_equal(x, y)


def test_ghost_ring_second_launch_same_knowledge(gpu, monkeypatch):
    for rank in range(2):
        out = []
        for cap in (None, "1"):
            if cap is None:
                monkeypatch.delenv("DCCRGX_APPEND_CAP", raising=False)
            else:
                monkeypatch.setenv("DCCRGX_APPEND_CAP", cap)
            g = _grid(rank, 2)
            out.append(g.get_cell_process())
            g.close()
        monkeypatch.delenv("DCCRGX_APPEND_CAP", raising=False)
        (ids, own), (ids1, own1) = out
        # the ring holds the other rank's cells: more than the forced capacity
        assert np.count_nonzero(own != rank) > 1
        assert np.array_equal(ids, ids1) and np.array_equal(own, own1)
