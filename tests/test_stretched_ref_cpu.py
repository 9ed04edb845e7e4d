"""Stretched_Cartesian_Geometry pinned to the reference, on the CPU.

tests/golden/stretched_ref.json holds what the reference's own
dccrg_stretched_cartesian_geometry.hpp answers for the two cases of
tests/stretched_model.py: get_length, get_center, get_min and get_max of every
possible cell, get_real_coordinate and get_indices of the point set, and the
bytes its write() puts into a grid file.  Where the reference checkout and MPI
are present, the probe below (this repository's text; the reference's headers
come in by include path) is compiled and its output must equal the file;
everywhere, the plain-Python model must equal the file.

get_indices of the reference reads below its coordinate list for a coordinate
exactly at a dimension's first boundary, so those points are left out of its
part of the file: test_excluded_points states how many.

    PYTHONPATH=. python tests/test_stretched_ref_cpu.py     regenerates the file (needs the reference)
"""
import json
import os
import subprocess

import numpy as np
import pytest

import stretched_model as SM
from oracle import oracle as O
from oracle import ref_programs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stretched_ref.json")

PROBE = r"""
// Prints what Stretched_Cartesian_Geometry answers, as raw bytes on stdout.
// stdin (text; doubles as the hexadecimal of their bits):
//   lx ly lz R px py pz
//   n c...            (three lines: a dimension's coordinates)
//   npts, then npts * 3 doubles
//   path of a scratch file for write()
// stdout: per cell 1..last length, center, min, max (3 doubles each); per
// point get_real_coordinate (3 doubles) and get_indices (3 uint64); then
// data_size() as uint64 and the bytes write() put at offset 0 of the file.
#include <mpi.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "dccrg_length.hpp"
#include "dccrg_mapping.hpp"
#include "dccrg_topology.hpp"
#include "dccrg_stretched_cartesian_geometry.hpp"

static double read_double() {
	std::string s;
	std::cin >> s;
	const uint64_t u = std::stoull(s, nullptr, 16);
	double d;
	std::memcpy(&d, &u, 8);
	return d;
}
static void put(const void* p, size_t n) { std::fwrite(p, 1, n, stdout); }
static void put3(const std::array<double, 3>& a) { put(a.data(), 24); }

int main(int argc, char** argv) {
	MPI_Init(&argc, &argv);
	unsigned long long lx, ly, lz;
	int R, per[3];
	if (!(std::cin >> lx >> ly >> lz >> R >> per[0] >> per[1] >> per[2])) return 2;
	dccrg::Mapping mapping;
	if (!mapping.set_length({{lx, ly, lz}})) return 3;
	if (!mapping.set_maximum_refinement_level(R)) return 4;
	dccrg::Grid_Topology topology;
	for (size_t d = 0; d < 3; d++) topology.set_periodicity(d, per[d] != 0);
	dccrg::Stretched_Cartesian_Geometry geometry(mapping.length, mapping, topology);
	dccrg::Stretched_Cartesian_Geometry::Parameters params;
	for (size_t d = 0; d < 3; d++) {
		size_t n;
		std::cin >> n;
		for (size_t i = 0; i < n; i++) params.coordinates[d].push_back(read_double());
	}
	if (!geometry.set(params)) return 5;
	for (uint64_t cell = 1; cell <= mapping.get_last_cell(); cell++) {
		put3(geometry.get_length(cell));
		put3(geometry.get_center(cell));
		put3(geometry.get_min(cell));
		put3(geometry.get_max(cell));
	}
	size_t npts;
	std::cin >> npts;
	for (size_t i = 0; i < npts; i++) {
		std::array<double, 3> x;
		for (size_t d = 0; d < 3; d++) x[d] = read_double();
		put3(geometry.get_real_coordinate(x));
		const dccrg::Types<3>::indices_t ind = geometry.get_indices(x);
		put(ind.data(), 24);
	}
	std::string path;
	std::cin >> path;
	MPI_File f;
	if (MPI_File_open(MPI_COMM_SELF, const_cast<char*>(path.c_str()), MPI_MODE_CREATE | MPI_MODE_RDWR, MPI_INFO_NULL,
	                  &f) != MPI_SUCCESS)
		return 6;
	if (!geometry.write(f, 0)) return 7;
	const uint64_t size = geometry.data_size();
	std::vector<char> bytes(size);
	MPI_File_read_at(f, 0, bytes.data(), int(size), MPI_BYTE, MPI_STATUS_IGNORE);
	MPI_File_close(&f);
	put(&size, 8);
	put(bytes.data(), size);
	std::fflush(stdout);
	MPI_Finalize();
	return 0;
}
"""


def _hex(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def _case_input(name):
    R, coords = SM.case_coords(name)
    pts = SM.point_set(coords, R)
    return R, coords, pts, pts[~SM.at_first_coordinate(coords, pts)]


def run_probe(binary, name, scratch):
    """The reference's answers for one case, in the golden file's layout."""
    R, coords, _, pts = _case_input(name)
    lines = ["%d %d %d %d %d %d %d" % (*SM.LENGTH, R, *[int(p) for p in SM.PERIODIC])]
    for c in coords:
        lines.append(" ".join([str(len(c))] + [_hex(v) for v in c]))
    lines.append(str(pts.shape[0]))
    lines += [" ".join(_hex(v) for v in p) for p in pts]
    lines.append(os.path.join(scratch, name + ".block"))
    r = subprocess.run([binary], input="\n".join(lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    out = r.stdout
    n_cells = O.Mapping(SM.LENGTH, R).last_cell
    cells = np.frombuffer(out[: n_cells * 96], np.float64).reshape(n_cells, 4, 3)
    at = n_cells * 96
    rec = np.frombuffer(out[at : at + pts.shape[0] * 48], np.uint64).reshape(-1, 6)
    at += pts.shape[0] * 48
    size = int(np.frombuffer(out[at : at + 8], np.uint64)[0])
    block = out[at + 8 :]
    assert len(block) == size
    return dict(length=cells[:, 0], center=cells[:, 1], min=cells[:, 2], max=cells[:, 3],
                real=rec[:, 0:3].copy().view(np.float64), indices=rec[:, 3:6].copy(),
                block=np.frombuffer(block, np.uint8))


def compile_probe(directory):
    src = os.path.join(directory, "stretched_probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    out = os.path.join(directory, "stretched_probe")
    subprocess.run(["g++", "-std=c++11", "-O2", "-I", ref_programs.REF, "-I", ref_programs.MPI_INC, "-o", out, src,
                    os.path.join(ref_programs.MPI_LIB, "libmpi.so"),
                    "-Wl,-rpath,/usr/lib/x86_64-linux-gnu:" + ref_programs.MPI_LIB], check=True)
    return out


def _reference_available():
    return (ref_programs.present() and os.path.exists(os.path.join(ref_programs.MPI_INC, "mpi.h"))
            and os.path.exists(os.path.join(ref_programs.MPI_LIB, "libmpi.so")))


KEYS = ("length", "center", "min", "max", "real", "indices", "block")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        raw = json.load(f)
    return {name: SM.unpack(_case_input(name)[0], _case_input(name)[3], raw[name]) for name in SM.CASES}


def test_reference_gives_the_golden_file(golden, tmp_path):
    if not _reference_available():
        pytest.skip("the reference checkout or MPI is not present")
    binary = compile_probe(str(tmp_path))
    for name in SM.CASES:
        got = run_probe(binary, name, str(tmp_path))
        for k in KEYS:
            assert SM.same_bits(got[k], golden[name][k]), (name, k)


@pytest.mark.parametrize("name", SM.CASES)
def test_excluded_points(name):
    """Only points with a coordinate exactly at its dimension's first boundary
    are left out of the reference's part: three distinct values, one a
    dimension."""
    R, coords, pts, kept = _case_input(name)
    first = np.array([c[0] for c in coords])
    out = pts[SM.at_first_coordinate(coords, pts)]
    assert 0 < out.shape[0] == pts.shape[0] - kept.shape[0] <= 60
    assert np.all(np.any(out == first, axis=1)) and not np.any(kept == first)
    # the reference's own loop cannot answer them, the facade's rule gives cell 0's first index
    with pytest.raises(IndexError):
        SM.indices_of(coords, R, out[:1], facade_rule=False)
    assert np.all(SM.indices_of(coords, R, out)[out == first] == 0)


@pytest.mark.parametrize("name", SM.CASES)
def test_model_gives_the_golden_file(golden, name):
    R, coords, _, pts = _case_input(name)
    G = golden[name]
    ids = np.arange(1, O.Mapping(SM.LENGTH, R).last_cell + 1, dtype=np.uint64)
    b = O.Mapping(SM.LENGTH, R).batch(ids)
    geo = SM.cell_geometry(coords, R, b["level"], b["indices"])
    for k in ("length", "center", "min", "max"):
        assert SM.same_bits(geo[k], G[k]), k
    assert SM.same_bits(SM.real_coordinates(coords, SM.PERIODIC, pts), G["real"])
    assert np.array_equal(SM.indices_of(coords, R, pts, facade_rule=False), G["indices"])
    assert np.array_equal(SM.indices_of(coords, R, pts), G["indices"])
    assert SM.geometry_block(coords) == G["block"].tobytes() == O.stretched_geometry_block(coords)
    # the cases do what they are for
    assert np.count_nonzero(G["indices"] == SM.ERROR_INDEX) > 100
    assert np.count_nonzero(np.isnan(G["real"])) > 10
    if name == "rounded":
        # c0 + 2^R li < c1 in x's second and z's last cell: x's third boundary gets the third cell's
        # first index, z's end one past the grid
        pt = np.array([[coords[0][2], 0.5, 0.0], [0.0, 0.5, coords[2][2]]])
        ind = SM.indices_of(coords, R, pt, facade_rule=False)
        assert ind[0, 0] == 2 << R and ind[1, 2] == 2 << R == SM.LENGTH[2] << R


def test_particle_model_uses_the_same_functions(golden):
    """StretchedParticleModel.real_coordinate / locate on the golden points."""
    R, coords, allpts, pts = _case_input("exact")
    o = O.Grid(SM.LENGTH, R, SM.PERIODIC, 1, 1)
    m = SM.StretchedParticleModel(o, coords)
    assert SM.same_bits(m.real_coordinate(pts), golden["exact"]["real"])
    # unrefined grid: the cell is the level-0 cell of the golden indices
    ind = golden["exact"]["indices"]
    inside = np.all(ind != SM.ERROR_INDEX, axis=1) & np.all(ind < m.glen, axis=1)
    exp = np.zeros(pts.shape[0], np.uint64)
    exp[inside] = o.mapping.from_indices(ind[inside], np.zeros(int(inside.sum()), np.int32))
    # (locate wraps first: compare where the point is inside the grid already)
    got = m.locate(pts)
    assert np.array_equal(got[inside], exp[inside]) and np.count_nonzero(exp) > 500


def _write_golden():
    import tempfile

    assert _reference_available(), "the reference checkout and MPI are needed"
    with tempfile.TemporaryDirectory() as td:
        binary = compile_probe(td)
        raw = {name: SM.pack(_case_input(name)[0], _case_input(name)[3], run_probe(binary, name, td))
               for name in SM.CASES}
    with open(GOLDEN, "w") as f:
        json.dump(raw, f, indent=0, sort_keys=True)
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    _write_golden()
