"""examples/pic_electromagnetic.cpp: four cycles of a full electromagnetic
particle-in-cell code (charge and current in one particles_deposit_moments
call, Faraday's and Ampere's law as one accumulating curl each, the current
through field_axpy, one gather of E and B, particles_boris, step) through the
facade's device members on a periodic 8 x 8 x 8 grid, at 1 and 2 processes.
The program checks its own invariants each cycle (no record lost, the record
count kept, max |div B| under its counted rounding bound) and prints PASSED;
max |div E|, which has the current as its source, is far above that bound."""
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [1, 2])
def test_pic_electromagnetic(gpu, P):
    out = mpirun("pic_electromagnetic", P)  # asserts exit status 0
    assert re.search(r"^PASSED$", out, re.M), out
    m = re.search(r"^pic_electromagnetic cycles 4 records (\d+) (\d+) lost 0$", out, re.M)
    assert m and m.group(1) == m.group(2) == str(2 * 512), out
    assert re.search(r"^div B within its bound in 4 of 4 cycles$", out, re.M), out
    lines = re.findall(r"^cycle (\d) max \|div B\| (\S+) bound (\S+) max \|div E\| (\S+)$", out, re.M)
    assert [int(l[0]) for l in lines] == [0, 1, 2, 3], out
    for _, div_b, bound, div_e in lines:
        assert float(div_b) <= float(bound) < 1e-13 and float(div_e) > 1e3 * float(bound), out
