"""examples/particles_adapt.cpp: particles that follow the mesh through the
facade's device members (particles_follow_mesh, particles_adapt_stats beside
particles_step) on a 4 x 4 x 4 periodic grid - refine, step, merge again,
step - at 1 and 3 processes: the particle count is conserved, nothing is lost,
no particle lies outside its cell, and both process counts print the same
line."""
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu


def test_particles_follow_mesh_members(gpu):
    lines = {}
    for P in (1, 3):
        out = mpirun("particles_adapt", P)
        m = re.search(r"^particles (\d+) (\d+) outside (\d+) lost (\d+)$", out, re.M)
        assert m, out
        before, after, outside, lost = (int(v) for v in m.groups())
        assert before >= 64 and after == before and outside == 0 and lost == 0, out
        lines[P] = m.group(0)
    assert lines[1] == lines[3]
