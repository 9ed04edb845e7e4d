"""examples/particles_deposit.cpp: particles_deposit and particles_gather
through the facade's device members on a 4 x 4 x 4 periodic grid at 1 and 3
processes.  The data are dyadic (positions on eighths of a cell, q on 2^-10,
the cell field on sixteenths), so every sum is exact: both process counts
print the same line, and the deposited total is the particles' total charge,
recomputed here from the example's seeded stream."""
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu

MASK = (1 << 64) - 1


def _stream(seed):
    """The example's splitmix64 stream of doubles in [0, 1)."""
    s = seed
    while True:
        s = (s + 0x9E3779B97F4A7C15) & MASK
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
        yield (z >> 11) / 9007199254740992.0


def _expected():
    records, charge = 0, 0.0
    for cell in range(1, 65):
        rnd = _stream(cell)
        count = 1 + int(5 * next(rnd))
        for _ in range(count):
            for _ in range(3):
                next(rnd)
            charge += int(1024 * next(rnd)) / 1024  # exact: multiples of 2^-10
        records += count
    return records, charge


def test_particles_deposit_members(gpu):
    records, charge = _expected()
    lines = {}
    for P in (1, 3):
        out = mpirun("particles_deposit", P)  # asserts exit status 0
        m = re.search(r"^deposit (\d+) (\S+) (\S+)$", out, re.M)
        assert m, out
        assert int(m.group(1)) == records, out
        assert float(m.group(2)) == charge, (out, charge)
        assert float(m.group(3)) != 0.0
        lines[P] = m.group(0)
    assert lines[1] == lines[3]
