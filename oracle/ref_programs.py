"""ORACLE build recipe - test infrastructure only: the reference's own test
programs compiled against the drop-in facade (include/dccrg.hpp) into
oracle/_ref/.

Where the reference checkout is present (BASELINE.json "reference_path", or
$DCCRG_REFERENCE), build() compiles
  ref_game_of_life            examples/game_of_life.cpp (BASELINE config 1)
  ref_kat_<name>              the known-answer programs of REF_KATS
  ref_variable_*              tests/variable_data_size/*.cpp
each with only its dccrg include lines pointed at include/ (the rewritten
source lives in a temporary directory), and
  ref_advection               examples/ref_advection.cpp, the repo's main over
                              the reference's tests/advection/*.hpp
  ref_game_of_life_amr        examples/ref_game_of_life_amr.cpp over the
                              reference's tests/game_of_life/*.hpp
with those headers included in place.  Only the binaries land in the tree,
under oracle/_ref/, which git ignores: they travel with the tree to a machine
without the reference, are never committed, and link the in-tree
libdccrgx.so through a relative rpath.  Where the reference is absent
build() does nothing and leaves oracle/_ref/ as it found it.

The GPU tests that run them: tests/test_gpu_ref_kats.py,
tests/test_gpu_ref_advection.py, tests/test_gpu_ref_gol_amr.py,
tests/test_gpu_facade.py."""
import json
import os
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_ref")
MPI_INC = "/opt/conda/include"
MPI_LIB = "/opt/conda/lib"


def reference_dir():
    ref = os.environ.get("DCCRG_REFERENCE")
    if not ref:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            ref = json.load(f)["reference_path"]
    return ref


REF = reference_dir()
REF_ADVECTION = os.path.join(REF, "tests", "advection")  # cell/initialize/solve/adapter.hpp, included in place
REF_GOL = os.path.join(REF, "tests", "game_of_life")  # cell/initialize/refine/solve.hpp, included in place
# the reference's known-answer test programs for the hot path (a8-a11, f4):
# each aborts or returns non-zero on a wrong answer; only the include line is
# rewritten (tests/test_gpu_ref_kats.py runs them under mpiexec)
REF_KATS = {
    "get_cells": "tests/get_cells/test1.cpp",
    "proc_bdy_cells": "tests/proc_bdy_cells/test1.cpp",
    "iterators1": "tests/iterators/test1.cpp",
    "iterators2": "tests/iterators/test2.cpp",
    "iterators3": "tests/iterators/test3.cpp",
    "iterators4": "tests/iterators/test4.cpp",
    "iterators5": "tests/iterators/test5.cpp",
    "get_face_neighbors": "tests/get_face_neighbors/test1.cpp",
    "get_neighbors_": "tests/get_neighbors_/test1.cpp",
    "neighbor_list_length": "tests/user_neighborhood/neighbor_list_length.cpp",
    # round 5: Stretched_Cartesian_Geometry, dccrg_mpi_support.hpp,
    # Additional_*_Items, get_cell_mpi_datatype, the blinker
    "scalability": "tests/game_of_life/scalability.cpp",
    "scalability1d": "tests/game_of_life/scalability1d.cpp",
    "dont_refine": "tests/refine/dont_refine.cpp",
    "acd_test1": "tests/additional_cell_data/test1.cpp",
    "acd_test2": "tests/additional_cell_data/test2.cpp",
    "acd_neighbor_data1": "tests/additional_cell_data/neighbor_data1.cpp",
    "acd_neighbor_data2": "tests/additional_cell_data/neighbor_data2.cpp",
    "get_cell_mpi_datatype": "tests/get_cell_datatype/get_cell_mpi_datatype.cpp",
    "datatype_run_time": "tests/get_cell_datatype/run_time.cpp",
    "simple_game_of_life": "examples/simple_game_of_life.cpp",
}
# the reference's variable-size payload tests (f4)
REF_VARIABLE = {"ref_variable_data_size": "tests/variable_data_size/variable_data_size.cpp",
                "ref_variable_neighbour_data": "tests/variable_data_size/variable_neighbour_data.cpp"}
_REF_INCLUDE = re.compile(r'#include "(?:\.\./)+(dccrg[A-Za-z0-9_]*\.hpp)"')


def rewrite_includes(txt, rel):
    """A reference program's dccrg includes ("../../dccrg.hpp",
    "../../dccrg_mpi_support.hpp", ...) pointed at the facade's headers of the
    same names in include/; nothing else in the program changes."""
    txt = _REF_INCLUDE.sub(r'#include "\1"', txt)
    assert re.search(r'#include "dccrg[A-Za-z0-9_]*\.hpp"', txt), rel
    return txt


def cxx(src, out, extra_inc=(), wait=True):
    """A facade program: plain C++ (g++) against include/ + the image's MPICH,
    linked to the in-tree libdccrgx.so (system libstdc++ first in the rpath).
    `out` lies two directories below the repository's root (examples/bin,
    oracle/_ref), which the relative rpath relies on.  `extra_inc` come after
    include/, so a reference header's "dccrg.hpp" resolves to the facade."""
    inc = os.path.join(ROOT, "include")
    xs = [a for d in extra_inc for a in ("-I", d)]
    cmd = ["g++", "-std=c++17", "-O2", "-I", inc, "-I", os.path.join(inc, "compat"), "-I", MPI_INC] + xs + [src,
           "-L", os.path.join(ROOT, "dccrg_amd"), "-ldccrgx", os.path.join(MPI_LIB, "libmpi.so"),
           "-Wl,-rpath,$ORIGIN/../../dccrg_amd:/usr/lib/x86_64-linux-gnu:" + MPI_LIB, "-o", out]
    if not wait:
        return subprocess.Popen(cmd)
    subprocess.run(cmd, check=True)


def present():
    return os.path.exists(os.path.join(REF, "dccrg_mapping.hpp"))


def build() -> None:
    """Every reference program above into oracle/_ref/ (needs libdccrgx.so)."""
    if not present():
        return
    os.makedirs(OUT, exist_ok=True)
    procs = []
    with tempfile.TemporaryDirectory() as td:
        jobs = [("ref_game_of_life", "examples/game_of_life.cpp")]
        jobs += [("ref_kat_" + name, rel) for name, rel in REF_KATS.items()]
        jobs += list(REF_VARIABLE.items())
        for name, rel in jobs:
            path = os.path.join(REF, rel)
            if not os.path.exists(path):
                continue
            src = os.path.join(td, name + ".cpp")
            with open(path) as f:
                txt = rewrite_includes(f.read(), rel)
            with open(src, "w") as f:
                f.write(txt)
            procs.append(cxx(src, os.path.join(OUT, name), wait=False))
        # the reference's advection solver (tests/advection/*.hpp, unmodified,
        # read in place) under the repo's 2d.cpp-style main, and its refined
        # game of life (tests/game_of_life/*.hpp) under the repo's
        # unrefined2d.cpp-style main
        for name, hdrs in (("ref_advection", REF_ADVECTION), ("ref_game_of_life_amr", REF_GOL)):
            if os.path.exists(os.path.join(hdrs, "solve.hpp")):
                assert not os.path.exists(os.path.join(hdrs, "dccrg.hpp"))
                procs.append(cxx(os.path.join(ROOT, "examples", name + ".cpp"), os.path.join(OUT, name), [hdrs],
                                 wait=False))
        bad = [p.args[-1] for p in procs if p.wait() != 0]
    if bad:
        raise RuntimeError(f"reference programs failed to compile against the facade: {bad}")


if __name__ == "__main__":
    build()
