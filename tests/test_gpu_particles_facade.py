"""examples/particles_device.cpp: the scenario of tests/particles/simple.cpp
(3 x 1 x 1 periodic cells, neighborhood length 1, vx = 0.1, 50 steps, halo
then step) through the facade's device members (add_variable_field<double>,
particles_step, Cartesian_Geometry::get_min / get_max, get_existing_cell) at
1 and 3 processes: the particle count is conserved, no particle lies outside
its cell, and both process counts print the same line."""
import re

import pytest

from test_gpu_facade import mpirun

pytestmark = pytest.mark.gpu


def test_particles_device_members(gpu):
    lines = {}
    for P in (1, 3):
        out = mpirun("particles_device", P)
        m = re.search(r"^particles (\d+) (\d+) outside (\d+)$", out, re.M)
        assert m, out
        before, after, outside = (int(v) for v in m.groups())
        assert before >= 3 and after == before and outside == 0, out
        lines[P] = m.group(0)
    assert lines[1] == lines[3]
