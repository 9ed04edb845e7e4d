"""examples/pic_adaptive.cpp: the electrostatic particle-in-cell cycle on a mesh
that adapts every second cycle, through the facade's device members, at 1 and
2 processes.  The particles follow the mesh, the charge density follows as
MEAN, the charge per cell as SUM and the potential as LINEAR
(field_follow_mesh).  The program checks its own invariants - the integral of
the density and the sum of the charges across every stop_refining within the
reduction's bound, the record count, no record lost - and prints PASSED; both
adaptations must have happened."""
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [1, 2])
def test_pic_adaptive(gpu, P):
    out = mpirun("pic_adaptive", P)  # asserts exit status 0
    assert re.search(r"^PASSED$", out, re.M), out
    m = re.search(r"^pic adaptive cycles 8 records (\d+) (\d+) lost 0 created (\d+) removed (\d+) off 0$", out, re.M)
    assert m, out
    before, after, created, removed = (int(v) for v in m.groups())
    assert before == after == 512 + 8 * 8 and created > 0 and removed > 0, out
    assert len(re.findall(r"^cycle \d iterations followed \d+ zero \d+$", out, re.M)) == 8, out
    assert len(re.findall(r"^adapt \d cells ", out, re.M)) == 4, out
