"""examples/pic_magnetized.cpp: three cycles of the particle half of a magnetised
particle-in-cell code (charge and current in one particles_deposit_moments
call, Poisson solve, gradient, one gather of E and B, particles_boris, step)
through the facade's device members on a refined periodic 8 x 8 x 8 grid, at 1
and 2 processes.  The program checks its own invariants each cycle (no record
lost, the record count kept, the cells' charge and current equal to the
records' within the deposit's rounding bound and the share tolerance) and
prints PASSED."""
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [1, 2])
def test_pic_magnetized(gpu, P):
    out = mpirun("pic_magnetized", P)  # asserts exit status 0
    assert re.search(r"^PASSED$", out, re.M), out
    m = re.search(r"^pic_magnetized cycles 3 records (\d+) (\d+) lost 0$", out, re.M)
    assert m and m.group(1) == m.group(2) == str(2 * (512 - 8 + 64)), out
    assert re.search(r"^moment sums checked 12, 0 off$", out, re.M), out
