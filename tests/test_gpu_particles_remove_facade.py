"""examples/particles_absorb.cpp: a drifting plasma on a periodic grid with an
absorbing body (a mask field) and a speed cut, removed with
grid.particles_remove at 1 and 2 processes.  The program prints, from
particles_reduce and field_reduce alone, the record count, the pool's charge,
the collected charge and the four counts of every cycle; the weights are
dyadic (0.25 * (1 + 0.25 k)), so pool + collected is the loaded charge exactly
whatever the order of the sums."""
import functools
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu

HEX = r"(-?0x[0-9a-f.]+p[-+]\d+)"
CYCLE = rf"^cycle (\d+) records (\d+) charge {HEX} collected {HEX} kept (\d+) mask (\d+) test (\d+) chance (\d+)$"


@functools.lru_cache(maxsize=None)
def _run(P):
    return mpirun("particles_absorb", P)  # asserts exit status 0


@pytest.mark.parametrize("P", [1, 2])
def test_particles_absorb_example(gpu, P):
    out = _run(P)
    assert re.search(r"^PASSED$", out, re.M), out
    m = re.search(rf"^loaded records (\d+) charge {HEX}$", out, re.M)
    assert m and int(m.group(1)) == 4 * 16 * 4 * 4, out
    loaded = float.fromhex(m.group(2))
    # 4 records of weight 0.25 * (1 + 0.25 (ix mod 4)) in each of 16 x 4 x 4 cells
    assert loaded == 16 * 4 * sum(1 + 0.25 * k for k in range(4))
    cycles = re.findall(CYCLE, out, re.M)
    assert [int(c[0]) for c in cycles] == list(range(1, 21)), out
    held, last_collected = 1024, 0.0
    for _, n, q, s, kept, by_mask, by_test, by_chance in cycles:
        assert int(kept) + int(by_mask) + int(by_test) + int(by_chance) == held, out
        held = int(kept)
        assert int(n) == held and int(by_chance) == 0
        assert float.fromhex(q) + float.fromhex(s) == loaded, out
        assert float.fromhex(s) >= last_collected
        last_collected = float.fromhex(s)
    assert int(cycles[0][5]) > 32  # the records loaded inside the body, but for the first step's traffic
    assert sum(int(c[5]) for c in cycles) > 100 and 0 < held < 1024, out


def test_the_lines_do_not_depend_on_the_processes(gpu):
    one, two = (re.findall(CYCLE, _run(P), re.M) for P in (1, 2))
    # (the charges are exact sums of dyadic weights: every field is compared)
    assert len(one) == 20 and one == two
