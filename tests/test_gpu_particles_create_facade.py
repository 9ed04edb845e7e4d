"""examples/particles_create.cpp: a plasma loaded and an inflow kept up with
grid.particles_create on a grid open in x, at 1 and 2 processes.  The program
prints the record count and the charge of every cycle from particles_reduce;
the loaded count is the requested total, the count stays inside the band the
example states, and the loaded charge is the weight sum of the model of
tests/particles_create_model.py (the weights are dyadic, 0.25 * (1 + 0.25 k):
every partial sum is exact, so the sums are equal whatever their order)."""
import functools
import re

import numpy as np
import pytest

import particles_create_model as PC
from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu

HEX = r"(-?0x[0-9a-f.]+p[-+]\d+)"
CYCLE = rf"^cycle (\d+) records (\d+) charge {HEX} created (\d+) lost (\d+)$"


@functools.lru_cache(maxsize=None)
def _run(P):
    return mpirun("particles_create", P)  # asserts exit status 0


def _model_charge():
    ids = np.arange(1, 16 * 4 * 4 + 1, dtype=np.uint64)
    ix = (ids - np.uint64(1)) % np.uint64(16)
    dens = 1 + 0.25 * (ix % np.uint64(4)).astype(np.float64)
    ctr = np.stack([ix + 0.5, ((ids - np.uint64(1)) // np.uint64(16)) % np.uint64(4) + 0.5,
                    (ids - np.uint64(1)) // np.uint64(64) + 0.5], axis=1).astype(np.float64)
    recs = PC.records(ids, np.full(ids.size, 4), ctr, np.ones_like(ctr), 7,
                      {6: ("const", 0.25, dict(base_field=dens))}, seed=1)
    return float(sum(r[:, 6].sum() for r in recs.values()))


@pytest.mark.parametrize("P", [1, 2])
def test_particles_create_example(gpu, P):
    out = _run(P)
    assert re.search(r"^PASSED$", out, re.M), out
    m = re.search(rf"^loaded records (\d+) charge {HEX}$", out, re.M)
    assert m and int(m.group(1)) == 4 * 16 * 4 * 4, out
    assert float.fromhex(m.group(2)) == _model_charge(), out
    band = re.search(r"^band (\d+) (\d+) records min (\d+) max (\d+)$", out, re.M)
    assert band, out
    lo, hi, seen_lo, seen_hi = (int(x) for x in band.groups())
    assert (lo, hi) == (1024 - 128, 1024 + 128) and lo <= seen_lo <= seen_hi <= hi
    cycles = re.findall(CYCLE, out, re.M)
    assert [int(c[0]) for c in cycles] == list(range(1, 21)), out
    held = 1024
    for _, n, q, created, lost in cycles:
        held += int(created) - int(lost)
        assert int(n) == held and lo <= held <= hi, out
        assert float.fromhex(q) > 0
    assert sum(int(c[3]) for c in cycles) > 50 and sum(int(c[4]) for c in cycles) > 50, out


def test_the_lines_do_not_depend_on_the_processes(gpu):
    one, two = (re.findall(CYCLE, _run(P), re.M) for P in (1, 2))
    # (the charge is a sum in an order that depends on the partition: the counts are compared)
    assert len(one) == 20 and [(c[0], c[1], c[3], c[4]) for c in one] == [(c[0], c[1], c[3], c[4]) for c in two]
