"""examples/pic_diagnostics.cpp: the electromagnetic particle-in-cell cycle of
pic_electromagnetic.cpp on the periodic 8 x 8 x 8 grid with every scalar of a
cycle (field energy, max |div B|, total charge, momenta, kinetic energy,
max |v_d| dt) from one collective field_reduce_device and one collective
particles_reduce_device call, at 1 and 2 processes.  The program checks them
against the host way (download and loop): extrema bitwise, sums within
gamma(k - 1) sum |t_i|, the records' charge against the deposited one, the
record count; it prints hex floats and PASSED.  The extrema and the record
count do not depend on the number of processes."""
import functools
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu

HEX = r"(-?0x[0-9a-f.]+p[-+]\d+)"
SECOND = rf"^cycle (\d) max \|div B\| {HEX} max \|v\| {HEX} {HEX} {HEX} records (\d+) max \|v\| dt {HEX}$"


@functools.lru_cache(maxsize=None)
def _run(P):
    return mpirun("pic_diagnostics", P)  # asserts exit status 0


@pytest.mark.parametrize("P", [1, 2])
def test_pic_diagnostics(gpu, P):
    out = _run(P)
    assert re.search(r"^PASSED$", out, re.M), out
    m = re.search(r"^pic_diagnostics cycles 4 records (\d+) (\d+) lost 0$", out, re.M)
    assert m and m.group(1) == m.group(2) == str(2 * 512), out
    # a cycle: 7 sums of the fields' call, 8 of the records', 4 extrema
    assert re.search(r"^sums checked 60, 0 off; extrema checked 16, 0 off$", out, re.M), out
    a = re.findall(rf"^cycle (\d) field energy {HEX} kinetic energy {HEX} charge {HEX} momentum {HEX} {HEX} {HEX}$", out,
                   re.M)
    b = re.findall(SECOND, out, re.M)
    assert [int(l[0]) for l in a] == [int(l[0]) for l in b] == [0, 1, 2, 3], out
    for l in a:
        energy, kinetic, charge = (float.fromhex(x) for x in l[1:4])
        assert energy > 0 and kinetic > 0 and abs(charge - 1024) < 1024 * 0.1, out
    for l in b:
        assert int(l[5]) == 1024 and 0 < float.fromhex(l[6]) < 1.0, out
        assert float.fromhex(l[1]) < 1e-13, out  # div B is rounding


def test_extrema_and_count_do_not_depend_on_the_processes(gpu):
    one, two = (re.findall(SECOND, _run(P), re.M) for P in (1, 2))
    assert len(one) == 4 and [l[:6] for l in one] == [l[:6] for l in two], (one, two)
