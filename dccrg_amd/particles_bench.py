"""Particle step measurement: python -m dccrg_amd.particles_bench

One GPU, a 128^3 periodic base grid (R = 0), 16 particles per cell, 3 doubles
per particle, |v dt| = 0.3 cell lengths, 20 timed steps after warm-up.  Prints
one JSON line in the style of bench.py's: ms per step, particle-updates/s, the
algorithmic bytes of the pass structure (Particles) and their
fraction of the HBM peak, and the time of one VariableField.resize re-lay of
the same pool in the same run (the library's copy-once yardstick)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import time

import numpy as np

PEAK_HBM_GBS = 8000.0  # MI355X HBM3E peak
K = 3
VELOCITY = (0.2, 0.2, 0.1)  # |v| = 0.3 cell lengths with dt = 1

# bytes of one step by pass (K = 3: a record is 24 B), per particle / per mover
PER_PARTICLE = {
    "locate: record position read + written, source slot, destination slot, stay and mover flags": 24 + 24 + 16,
    "two scans: flags read, ranks written": 16,
    "mover keys: source, destination, flag, rank read": 16,
    "scatter of the stayers: source, flag, rank read": 12,
    "record copied into the new pool (read + write)": 48,
}
PER_MOVER = {
    "key + particle index written": 12,
    "radix sort of (key, index): 6 passes of 8 bits over 42 key bits, read + write, and the histogram read": 6 * 24 + 8,
    "run boundaries: key read": 8,
    "scatter of the movers: key + index read": 12,
}


def alg_bytes(n_particles, n_movers, n_cells, hood_entries):
    per_p, per_m = sum(PER_PARTICLE.values()), sum(PER_MOVER.values())
    # neighbors_of rows (id 8 B + slot 4 B per entry) of the cells that hold a mover, read once
    rows = n_cells * hood_entries * 12 if n_movers else 0
    return n_particles * per_p + n_movers * per_m + rows, per_p, per_m


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--base", type=int, default=128)
    p.add_argument("--ppc", type=int, default=16)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None, help="also write the line to this file")
    a = p.parse_args(argv)

    import torch  # noqa: F401  (one HIP runtime for the process)

    import dccrg_amd
    from dccrg_amd._lib import check, lib

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(0).set_periodic(True, True, True).initialize()
    fld = g.add_variable_field("particles", np.float64, True)
    ids = g.slot_ids()[: g.n_local]
    nc = ids.size
    # positions: uniform inside each cell (cell c's min corner from its id, unit cells)
    k = (ids - np.uint64(1)).astype(np.int64)
    corner = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1).astype(np.float64)
    rng = np.random.default_rng(1)
    pos = (corner[:, None, :] + rng.random((nc, a.ppc, 3))).reshape(-1)
    counts = np.full(nc, a.ppc * K, np.uint64)
    fld.resize(counts)
    check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, pos.ctypes.data_as(C.c_void_p), pos.nbytes))
    del pos, corner
    n_particles = nc * a.ppc

    for _ in range(a.warmup):
        st = g.particles_step(fld, K, VELOCITY, 1.0)
    g.synchronize()
    movers = 0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        st = g.particles_step(fld, K, VELOCITY, 1.0)
        movers += st["moved"]
    g.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / max(a.steps, 1)
    assert sum(st.values()) == n_particles and st["lost"] == 0, st

    # the yardstick: one re-lay of the same pool (every cell keeps its size)
    cur = fld.sizes(0, nc) // np.uint64(8)
    g.synchronize()
    relay = []
    for _ in range(3):
        t0 = time.perf_counter()
        fld.resize(cur)
        g.synchronize()
        relay.append((time.perf_counter() - t0) * 1e3)
    relay_ms = min(relay)

    m_step = movers / max(a.steps, 1)
    total, per_p, per_m = alg_bytes(n_particles, m_step, nc, 26)
    ach = total / (ms / 1e3) / 1e9
    line = {"metric": "particles_step", "value": n_particles / (ms / 1e3), "unit": "particle-updates/s", "n_gpus": 1,
            "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms, "higher_is_better": True, "dtype": "fp64",
            "config": {"workload": f"particles in cells, {n}^3 periodic, R = 0, neighborhood 1, {a.ppc} per cell, "
                                   f"K = {K}, |v dt| = 0.3 cell lengths", "cells": int(nc),
                       "particles": int(n_particles), "movers_per_step": m_step},
            "roofline": {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": ach / PEAK_HBM_GBS, "alg_bytes_per_step": total,
                         "alg_bytes_per_particle": per_p, "alg_bytes_per_mover": per_m,
                         "passes": {"per_particle": PER_PARTICLE, "per_mover": PER_MOVER}},
            "relay": {"what": "VariableField.resize of the same pool, sizes unchanged (copy once)",
                      "ms": relay_ms, "step_over_relay": ms / relay_ms}}
    g.close()
    txt = json.dumps(line)
    print(txt, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
