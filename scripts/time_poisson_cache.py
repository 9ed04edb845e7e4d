"""Time Poisson_Solve's cache pass (dccrgx_poisson_cache: classification, type
halo, the factor kernel, factor halo, the transposed factors) on one 128^3
grid with a maximum refinement level of 1 and the center refined, once under
the Cartesian geometry and once under a stretched geometry with seeded uneven
coordinates, the same tree, alternating.  The host clock around the call,
which ends in a stream synchronise; the median of the repeats after a warm-up
of each.  Prints one JSON line and, with a path argument, writes it there."""
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
import dccrg_amd  # noqa: E402


def main(out=None, n=128, repeats=7):
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(0)
    g.set_maximum_refinement_level(1).set_periodic(True, True, True).initialize()
    lo, hi = n // 2 - n // 16, n // 2 + n // 16
    k = np.arange(lo, hi, dtype=np.uint64)
    center = (1 + k[None, None, :] + n * k[None, :, None] + n * n * k[:, None, None]).ravel()
    for c in center:
        g.refine_completely(int(c))
    g.stop_refining()
    rng = np.random.default_rng(128)
    coords = [np.concatenate([[0.0], np.cumsum(0.25 + 0.75 * rng.random(n))]) for _ in range(3)]
    ids = g.local_cells()
    rhs = g.add_field("rhs", np.float64, False)
    sol = g.add_field("solution", np.float64, False)
    rhs.set(np.zeros(g.n_local))
    sol.set(np.zeros(g.n_local))
    s = dccrg_amd.Poisson_Solve()

    def geometry(stretched):
        if stretched:
            g.set_stretched_geometry(coords)
        else:
            g.set_geometry((0, 0, 0), (1.0, 1.0, 1.0))

    def timed():
        g.synchronize()
        t0 = time.perf_counter()
        s.cache_system_info(ids, g)
        g.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ms = {False: [], True: []}
    for stretched in (False, True):  # warm-up: code objects, buffers, the coordinates' upload
        geometry(stretched)
        timed()
    for _ in range(repeats):
        for stretched in (False, True):
            geometry(stretched)
            ms[stretched].append(timed())
    cart, st = statistics.median(ms[False]), statistics.median(ms[True])
    res = {"what": "dccrgx_poisson_cache, 128^3 level-0 cells, R = 1, center refined, one MI355X",
           "cells": int(g.n_local), "repeats": repeats, "cartesian_ms": cart, "stretched_ms": st,
           "stretched_over_cartesian": st / cart,
           "cartesian_ms_all": ms[False], "stretched_ms_all": ms[True]}
    g.close()
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
