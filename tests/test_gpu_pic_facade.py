"""examples/pic_electrostatic.cpp: three electrostatic particle-in-cell cycles
(deposit, Poisson solve, gradient, gather, accelerate, step) through the
facade's device members on a refined periodic 8 x 8 x 8 grid, at 1 and 2
processes.  The program checks its own invariants (E of phi = x^2 is -2 x
where both x-neighbors lie inside the grid; no record lost, the record count
conserved) and prints PASSED."""
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [1, 2])
def test_pic_electrostatic(gpu, P):
    out = mpirun("pic_electrostatic", P)  # asserts exit status 0
    assert re.search(r"^PASSED$", out, re.M), out
    m = re.search(r"^pic cycles 3 records (\d+) (\d+) lost 0$", out, re.M)
    assert m and m.group(1) == m.group(2) == str(2 * (512 - 8 + 64)), out
    m = re.search(r"^field of x\^2 checked on (\d+) cells, 0 off$", out, re.M)
    assert m and int(m.group(1)) > 400, out
