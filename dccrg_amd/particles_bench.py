"""Particle step measurement: python -m dccrg_amd.particles_bench

One GPU, a 128^3 periodic base grid (R = 0), 16 particles per cell, 3 doubles
per particle, |v dt| = 0.3 cell lengths, 20 timed steps after warm-up.  Prints
one JSON line in the style of bench.py's: ms per step, particle-updates/s, the
algorithmic bytes of the pass structure (Particles) and their
fraction of the HBM peak, and the time of one VariableField.resize re-lay of
the same pool in the same run (the library's copy-once yardstick).

--stretched measures the same grid under a Stretched_Cartesian_Geometry of
unequal cells (dccrgx_set_stretched_geometry) next to the Cartesian step, and
records the parent commit's Cartesian lines given with --parent.

--adapt measures what it costs that the particles follow the mesh
(Dccrg.particles_follow_mesh): on the same 128^3 base with R = 1 a z-slab of
one eighth of the cells is refined and merged again, and the two stop_refining
calls are timed with follow on and off, beside one re-lay of the pool.

--fields-adapt measures what it costs that fp64 cell fields follow the mesh
(Dccrg.field_follow_mesh) in --adapt's scenario: stop_refining with no cell
field (the parent commit's --adapt follow-off scenario, given with --parent),
with 1 and 6 fields that are only carried, that follow as MEAN and that follow
as LINEAR, alternating, and the host way (download the fields and the removed
store, the NumPy mean, upload) beside them.

--deposit measures the particle <-> mesh transfer on the same grid: CIC and
NGP Dccrg.particles_deposit (K = 4) and a CIC Dccrg.particles_gather of three
fields (K = 7), beside the default step and re-lay in the same run.

--pic measures one electrostatic particle-in-cell cycle on the same grid from
the public calls only (K = 10: position, velocity, q, E): CIC deposit per
volume, rhs = -(rho - mean rho) with torch on the fields' device arrays, a
Poisson solve of a fixed iteration count, Dccrg.gradient with scale -1, the
halo, a CIC gather of E, Dccrg.particles_accelerate and the step with
per-record velocities, each stage timed on its own, and Dccrg.gradient alone
on the uniform grid and on --adapt's refined one.

--moments measures Dccrg.particles_deposit_moments against the calls it
replaces, in one run on the same grid: particles_deposit of one double and the
fused call with 1, 4 (rho, J) and 10 (rho, J, P) moments on a K = 10 pool,
then on a K = 13 pool (position, velocity, q, E, B) the CIC gather of three
and of six fields and Dccrg.particles_boris beside particles_accelerate.  The
calls alternate, each synchronized; median and min - max of the timed ones.

--curl measures Dccrg.curl (plain and accumulating), Dccrg.divergence,
Dccrg.gradient and Dccrg.field_axpy beside the curl a caller composed before
them from three gradient calls into six scratch fields and three axpys, the
six alternating in one run on --pic's two gradient grids.

--reduce measures Dccrg.field_reduce on the same two grids: the seven-term
energy call (six squares by volume and max |div B|) against the same values
from seven single-term calls, Dccrg.field_axpy as the streaming yardstick and
the host way (download of the seven fields and NumPy), alternating in one run,
between device events and on the host clock; and Dccrg.particles_reduce of
count, charge, momenta and squares beside particles_accelerate on the K = 10
pool."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
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


def stretched_coordinates(n, seed=7):
    """Level-0 boundaries of unequal cells: widths 0.5 .. 1.5 in a fixed,
    seeded pattern of their own per dimension."""
    rng = np.random.default_rng(seed)
    return [np.concatenate([[0.0], np.cumsum(0.5 + rng.random(n))]) for _ in range(3)]


def measure(a, coords=None):
    """The timed steps on a fresh grid: Cartesian unit cells, or the stretched
    geometry of `coords` with the velocity scaled by the mean cell width, so
    that about the same share of the particles changes cell per step."""
    import dccrg_amd
    from dccrg_amd._lib import check, lib

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(0).set_periodic(True, True, True).initialize()
    velocity = VELOCITY
    if coords is not None:
        g.set_stretched_geometry(coords)
        # the seeded pattern (16 per cell, so denser in narrow cells) drifts through
        # several cells during the warm-up and the timed steps; averaged over that
        # drift a boundary sees the mean density, and the share of particles that
        # cross one per step is v / (mean cell width)
        velocity = tuple(float(v * np.mean(np.diff(c))) for v, c in zip(VELOCITY, coords))
    fld = g.add_variable_field("particles", np.float64, True)
    ids = g.slot_ids()[: g.n_local]
    nc = ids.size
    # positions: uniform inside each cell (cell c's min corner from its id)
    k = (ids - np.uint64(1)).astype(np.int64)
    ix = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1)
    if coords is None:
        corner, width = ix.astype(np.float64), np.ones((nc, 3))
    else:
        corner = np.stack([coords[d][ix[:, d]] for d in range(3)], axis=1)
        width = np.stack([np.diff(coords[d])[ix[:, d]] for d in range(3)], axis=1)
    rng = np.random.default_rng(1)
    pos = (corner[:, None, :] + width[:, None, :] * rng.random((nc, a.ppc, 3))).reshape(-1)
    counts = np.full(nc, a.ppc * K, np.uint64)
    fld.resize(counts)
    check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, pos.ctypes.data_as(C.c_void_p), pos.nbytes))
    del pos, corner, width
    n_particles = nc * a.ppc

    for _ in range(a.warmup):
        st = g.particles_step(fld, K, velocity, 1.0)
    g.synchronize()
    movers = 0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        st = g.particles_step(fld, K, velocity, 1.0)
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
    g.close()
    return dict(ms=ms, relay_ms=relay_ms, cells=int(nc), particles=int(n_particles),
                movers_per_step=movers / max(a.steps, 1))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--base", type=int, default=128)
    p.add_argument("--ppc", type=int, default=16)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None, help="also write the line to this file")
    p.add_argument("--stretched", action="store_true",
                   help="the same grid under a stretched geometry of unequal cells, next to the Cartesian step "
                        "(--repeats of each, alternating); writes profiles/particles_bench_stretched.json unless --out")
    p.add_argument("--adapt", action="store_true",
                   help="particles following the mesh: a z-slab of a base^3, R = 1 grid refined and merged again, "
                        "stop_refining with follow on against follow off (--repeats of each, alternating) and "
                        "against one re-lay of the pool; writes profiles/particles_bench_adapt.json unless --out")
    p.add_argument("--fields-adapt", action="store_true",
                   help="cell fields following the mesh (Dccrg.field_follow_mesh): on --adapt's grid stop_refining with "
                        "0, 1 and 6 fp64 fields carried only, following as MEAN and as LINEAR (--repeats of each, "
                        "alternating), the host way beside them, and with --parent the parent commit's --adapt "
                        "follow-off runs; writes profiles/particles_bench_fields_adapt.json unless --out")
    p.add_argument("--deposit", action="store_true",
                   help="charge deposition and field gather: CIC and NGP particles_deposit (K = 4) and a CIC "
                        "particles_gather of three fields (K = 7) beside the particle step and the re-lay in the "
                        "same run; writes profiles/particles_bench_deposit.json unless --out")
    p.add_argument("--pic", action="store_true",
                   help="the electrostatic particle-in-cell cycle stage by stage (deposit, rhs, solve, halo, gradient, "
                        "halo, gather, accelerate, step; K = 10) and dccrgx_gradient alone on the uniform and on "
                        "--adapt's refined grid; writes profiles/particles_bench_pic.json unless --out")
    p.add_argument("--moments", action="store_true",
                   help="particles_deposit_moments with 1, 4 and 10 moments beside particles_deposit of one double "
                        "(K = 10), and the CIC gather of six fields and particles_boris beside particles_accelerate "
                        "(K = 13), alternating in one run; writes profiles/particles_bench_moments.json unless --out")
    p.add_argument("--curl", action="store_true",
                   help="dccrgx_curl (plain and accumulating), dccrgx_divergence, dccrgx_gradient, dccrgx_field_axpy and "
                        "the curl composed from three gradients and three axpys, alternating in one run on the uniform "
                        "and on --adapt's refined grid; writes profiles/particles_bench_curl.json unless --out")
    p.add_argument("--reduce", action="store_true",
                   help="measure Dccrg.field_reduce (seven terms in one call against seven calls, field_axpy and the "
                        "host way) on the uniform and on --adapt's refined grid, and Dccrg.particles_reduce beside "
                        "particles_accelerate; writes profiles/particles_bench_reduce.json unless --out")
    p.add_argument("--pic-iterations", type=int, default=10, help="with --pic: BiCG iterations of a solve (min = max)")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--parent", default=None,
                   help="with --stretched: files of lines the parent commit's particles_bench printed in the same "
                        "machine visit (comma-separated), recorded as the parent's Cartesian step; with --adapt: "
                        "files of measure_adapt(follow=False) results taken with the parent commit's library")
    p.add_argument("--create", action="store_true",
                   help="Dccrg.particles_create into an empty pool and as an append of one record per cell to the full "
                        "pool (K = 10), beside the host way (NumPy generation and upload) and one re-lay of the pool, "
                        "alternating in one run; writes profiles/particles_bench_create.json unless --out")
    p.add_argument("--remove", action="store_true",
                   help="Dccrg.particles_remove on the full pool (K = 10): a velocity test, a mask plane, chance with "
                        "rescale, a test that removes nothing and the velocity test with `into`, beside one re-lay of "
                        "the pool and the host route; writes profiles/particles_bench_remove.json unless --out")
    a = p.parse_args(argv)

    import torch  # noqa: F401  (one HIP runtime for the process)

    if a.remove:
        return main_remove(a)
    if a.create:
        return main_create(a)
    if a.reduce:
        return main_reduce(a)
    if a.curl:
        return main_curl(a)
    if a.pic:
        return main_pic(a)
    if a.moments:
        return main_moments(a)
    if a.deposit:
        return main_deposit(a)
    if a.fields_adapt:
        return main_fields_adapt(a)
    if a.adapt:
        return main_adapt(a)
    if a.stretched:
        return main_stretched(a)
    r = measure(a)
    n, ms, relay_ms, nc, n_particles = a.base, r["ms"], r["relay_ms"], r["cells"], r["particles"]
    m_step = r["movers_per_step"]
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
    txt = json.dumps(line)
    print(txt, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


def main_stretched(a):
    """Stretched and Cartesian steps of this tree, alternating, each on a
    fresh grid; the medians, every run, and the parent commit's Cartesian
    lines when given."""
    coords = stretched_coordinates(a.base)
    runs = {"cartesian": [], "stretched": []}
    for _ in range(max(a.repeats, 1)):
        runs["cartesian"].append(measure(a))
        runs["stretched"].append(measure(a, coords))
    med = {k: float(np.median([r["ms"] for r in v])) for k, v in runs.items()}
    n_particles = runs["stretched"][0]["particles"]
    line = {"metric": "particles_step_stretched", "value": n_particles / (med["stretched"] / 1e3),
            "unit": "particle-updates/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": med["stretched"], "higher_is_better": True, "dtype": "fp64",
            "config": {"workload": f"particles in cells, {a.base}^3 periodic, R = 0, neighborhood 1, {a.ppc} per cell, "
                                   f"K = {K}; stretched: level-0 widths 0.5 .. 1.5 (seeded), the velocity scaled to "
                                   "the Cartesian run's share of movers",
                       "coordinates_in_lds": bool(sum(c.size for c in coords) <= 1536), "repeats": a.repeats},
            "stretched": {"ms_per_step": med["stretched"], "runs": runs["stretched"]},
            "cartesian": {"ms_per_step": med["cartesian"], "runs": runs["cartesian"]},
            "stretched_over_cartesian": med["stretched"] / med["cartesian"]}
    if a.parent:
        ms = []
        for path in a.parent.split(","):
            with open(path) as f:
                ms += [json.loads(ln)["ms_per_step"] for ln in f if ln.strip()]
        line["parent_cartesian"] = {"ms_per_step": float(np.median(ms)), "runs_ms": ms}
        line["cartesian_over_parent"] = med["cartesian"] / float(np.median(ms))
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_stretched.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


def measure_adapt(a, follow):
    """One refinement and one unrefinement of a z-slab (one eighth of the
    cells) of a fresh base^3 periodic grid with R = 1 and ppc particles per
    cell: the times of the two stop_refining calls, with the particle field
    following the mesh or not (then the slab's particles are dropped, as the
    default is), and one re-lay of the full pool before them."""
    import dccrg_amd
    from dccrg_amd._lib import check, lib

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(1).set_periodic(True, True, True).initialize()
    fld = g.add_variable_field("particles", np.float64, True)
    if follow:
        g.particles_follow_mesh(fld, K)
    ids = g.slot_ids()[: g.n_local]
    nc = ids.size
    k = (ids - np.uint64(1)).astype(np.int64)
    ix = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1)
    rng = np.random.default_rng(1)
    pos = (ix.astype(np.float64)[:, None, :] + rng.random((nc, a.ppc, 3))).reshape(-1)
    fld.resize(np.full(nc, a.ppc * K, np.uint64))
    check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, pos.ctypes.data_as(C.c_void_p), pos.nbytes))
    del pos
    cur = fld.sizes(0, nc) // np.uint64(8)
    g.synchronize()
    relay = []
    for _ in range(3):
        t0 = time.perf_counter()
        fld.resize(cur)
        g.synchronize()
        relay.append((time.perf_counter() - t0) * 1e3)

    def timed_stop_refining():
        g.synchronize()
        t0 = time.perf_counter()
        g.stop_refining()
        g.synchronize()
        return (time.perf_counter() - t0) * 1e3

    slab = ids[ix[:, 2] < max(n // 8, 1)]
    for c in slab:
        g.refine_completely(int(c))
    refine_ms = timed_stop_refining()
    st_refine = g.particles_adapt_stats(fld) if follow else None
    cells_refined = int(g.n_local)
    for c in g.mapping_batch(slab)["child"]:
        g.unrefine_completely(int(c))
    unrefine_ms = timed_stop_refining()
    st_unrefine = g.particles_adapt_stats(fld) if follow else None
    left = int(fld.sizes(0, g.n_local).sum()) // (8 * K)
    assert g.n_local == nc, (g.n_local, nc)
    if follow:
        moved = slab.size * a.ppc
        assert st_refine == dict(to_children=moved, to_parents=0, lost=0), st_refine
        assert st_unrefine == dict(to_children=0, to_parents=moved, lost=0), st_unrefine
        assert left == nc * a.ppc, left
    g.close()
    return dict(follow=bool(follow), refine_ms=refine_ms, unrefine_ms=unrefine_ms, relay_ms=min(relay),
                cells=int(nc), cells_refined=cells_refined, refined_parents=int(slab.size),
                particles=int(nc * a.ppc), particles_left=left)


def main_adapt(a):
    """Follow on and off on this tree, alternating, each on a fresh grid; the
    medians, every run, and the parent commit's follow-off runs when given."""
    runs = {"off": [], "on": []}
    for _ in range(max(a.repeats, 1)):
        runs["off"].append(measure_adapt(a, False))
        runs["on"].append(measure_adapt(a, True))
    med = {k: {w: float(np.median([r[w] for r in v])) for w in ("refine_ms", "unrefine_ms", "relay_ms")}
           for k, v in runs.items()}
    relay = float(np.median([r["relay_ms"] for v in runs.values() for r in v]))
    cost = {w: med["on"][w] - med["off"][w] for w in ("refine_ms", "unrefine_ms")}
    r0 = runs["on"][0]
    line = {"metric": "particles_follow_mesh", "value": cost["refine_ms"], "unit": "ms", "n_gpus": 1,
            "higher_is_better": False, "dtype": "fp64",
            "config": {"workload": f"{a.base}^3 periodic, R = 1, neighborhood 1, {a.ppc} particles per cell, K = {K}; "
                                   "a z-slab of one eighth of the cells refined by one stop_refining, the same "
                                   "families merged by the next; a fresh grid per run, follow off and on alternating",
                       "cells": r0["cells"], "refined_parents": r0["refined_parents"], "particles": r0["particles"],
                       "particles_carried": r0["refined_parents"] * a.ppc, "repeats": a.repeats},
            "follow_on": {**med["on"], "runs": runs["on"]}, "follow_off": {**med["off"], "runs": runs["off"]},
            "carry_cost_ms": {"refine": cost["refine_ms"], "unrefine": cost["unrefine_ms"],
                              "what": "median stop_refining with follow on minus with follow off"},
            "relay": {"what": "VariableField.resize of the full pool, sizes unchanged (copy once)", "ms": relay,
                      "refine_cost_over_relay": cost["refine_ms"] / relay,
                      "unrefine_cost_over_relay": cost["unrefine_ms"] / relay}}
    if a.parent:
        pr = []
        for path in a.parent.split(","):
            with open(path) as f:
                pr += [json.loads(ln) for ln in f if ln.strip()]
        line["parent_follow_off"] = {
            "what": "the parent commit's stop_refining of the same scenario (no follow members), same machine visit",
            "refine_ms": float(np.median([r["refine_ms"] for r in pr])),
            "unrefine_ms": float(np.median([r["unrefine_ms"] for r in pr])), "runs": pr}
        for w in ("refine_ms", "unrefine_ms"):
            v = [r[w] for r in pr]
            line["parent_follow_off"][w + "_spread"] = [min(v), max(v)]
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_adapt.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


def measure_fields_adapt(a, nf, mode, host=False):
    """measure_adapt(follow=False)'s scenario - the same grid, the same
    particle field, the same slab refined and merged again - with nf more
    fp64 cell fields that follow the mesh with `mode` (None: they are only
    carried).  host=True (mode None) also times the host way after the merge:
    download every field and its removed store, the NumPy mean per merged
    parent, upload."""
    import dccrg_amd
    from dccrg_amd._lib import check, lib

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(1).set_periodic(True, True, True).initialize()
    fld = g.add_variable_field("particles", np.float64, True)
    ids = g.slot_ids()[: g.n_local]
    nc = ids.size
    k = (ids - np.uint64(1)).astype(np.int64)
    ix = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1)
    rng = np.random.default_rng(1)
    pos = (ix.astype(np.float64)[:, None, :] + rng.random((nc, a.ppc, 3))).reshape(-1)
    fld.resize(np.full(nc, a.ppc * K, np.uint64))
    check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, pos.ctypes.data_as(C.c_void_p), pos.nbytes))
    del pos
    fields = []
    for j in range(nf):
        f = g.add_field(f"f{j}", np.float64, True)
        f.set(rng.random(g.n_slots))
        g.field_follow_mesh(f, mode)
        fields.append(f)
    first = fields[0].get(0, nc) if fields else None

    def timed_stop_refining():
        g.synchronize()
        t0 = time.perf_counter()
        g.stop_refining()
        g.synchronize()
        return (time.perf_counter() - t0) * 1e3

    slab = ids[ix[:, 2] < max(n // 8, 1)]
    for c in slab:
        g.refine_completely(int(c))
    refine_ms = timed_stop_refining()
    for c in g.mapping_batch(slab)["child"]:
        g.unrefine_completely(int(c))
    unrefine_ms = timed_stop_refining()
    assert g.n_local == nc, (g.n_local, nc)
    out = dict(fields=nf, mode=mode or "off", refine_ms=refine_ms, unrefine_ms=unrefine_ms, cells=int(nc),
               refined_parents=int(slab.size))
    if host:
        g.synchronize()
        t0 = time.perf_counter()
        rm = g.get_removed_cells()
        par, inv = np.unique(g.mapping_batch(rm)["parent"], return_inverse=True)
        sl = g.slot_ids()[:nc]
        order = np.argsort(sl)
        at = order[np.searchsorted(sl[order], par)]
        for f in fields:
            v = f.get(0, nc)
            v[at] = np.bincount(inv, weights=f.get_removed() / 8.0, minlength=par.size)
            f.set(v)
        g.synchronize()
        out["host_unrefine_ms"] = (time.perf_counter() - t0) * 1e3
        mode = "mean"  # what the fields now hold
    if fields and mode:
        # SUM of eighths, MEAN of copies and LINEAR's conservative children all give the parent back
        got = fields[0].get(0, nc)
        assert np.allclose(got, first, rtol=1e-13, atol=1e-15), float(np.max(np.abs(got - first)))
    g.close()
    return out


def main_fields_adapt(a):
    """stop_refining with 0, 1 and 6 fp64 cell fields, carried only, following
    as MEAN and following as LINEAR, alternating, each on a fresh grid; the
    host way beside them; the parent commit's follow-off runs when given."""
    configs = [("off_0", 0, None), ("off_1", 1, None), ("off_6", 6, None), ("mean_1", 1, "mean"),
               ("mean_6", 6, "mean"), ("linear_1", 1, "linear"), ("linear_6", 6, "linear")]
    runs = {name: [] for name, _, _ in configs}
    measure_fields_adapt(a, 1, "linear")  # warm-up: code objects, the pool's first blocks
    for _ in range(max(a.repeats, 1)):
        for name, nf, mode in configs:
            runs[name].append(measure_fields_adapt(a, nf, mode, host=mode is None and nf > 0))
    W = ("refine_ms", "unrefine_ms")
    med = {k: {w: float(np.median([r[w] for r in v])) for w in W} for k, v in runs.items()}
    spread = {k: {w: [min(r[w] for r in v), max(r[w] for r in v)] for w in W} for k, v in runs.items()}
    host = {nf: float(np.median([r["host_unrefine_ms"] for r in runs[f"off_{nf}"]])) for nf in (1, 6)}
    added = {}
    for mode in ("mean", "linear"):
        for nf in (1, 6):
            d = {w: med[f"{mode}_{nf}"][w] - med[f"off_{nf}"][w] for w in W}
            added[f"{mode}_{nf}"] = {
                "refine_ms": d["refine_ms"], "unrefine_ms": d["unrefine_ms"],
                "refine_over_off_0": d["refine_ms"] / med["off_0"]["refine_ms"],
                "unrefine_over_off_0": d["unrefine_ms"] / med["off_0"]["unrefine_ms"],
                "host_unrefine_over_added_unrefine": host[nf] / d["unrefine_ms"] if d["unrefine_ms"] > 0 else None}
    r0 = runs["off_0"][0]
    line = {"metric": "field_follow_mesh", "value": added["linear_6"]["refine_ms"], "unit": "ms", "n_gpus": 1,
            "higher_is_better": False, "dtype": "fp64",
            "config": {"workload": f"{a.base}^3 periodic, R = 1, neighborhood 1, {a.ppc} particles per cell (not "
                                   f"following), K = {K}; a z-slab of one eighth of the cells refined by one "
                                   "stop_refining, the same families merged by the next; a fresh grid per run, the "
                                   "configurations alternating",
                       "cells": r0["cells"], "refined_parents": r0["refined_parents"], "repeats": a.repeats},
            "stop_refining_ms": med, "spread_ms": spread, "runs": runs,
            "added_by_following": {"what": "median stop_refining with the fields following minus with the same "
                                           "fields only carried; over off_0: as a multiple of stop_refining "
                                           "without any cell field", **added},
            "host_way": {"what": "after the merge: get_removed_cells, every field and its removed store downloaded, "
                                 "the mean per merged parent in NumPy, every field uploaded",
                         "unrefine_ms": host},
            "slope_pass": "a list pass over the refined parents (field_slopes_kernel), not the full-grid gradient"}
    if a.parent:
        pr = []
        for path in a.parent.split(","):
            with open(path) as f:
                pr += [json.loads(ln) for ln in f if ln.strip()]
        pr = [r for ln in pr for r in (ln["follow_off"]["runs"] if "follow_off" in ln else [ln])]
        line["parent_follow_off"] = {
            "what": "the parent commit's stop_refining of off_0's scenario, same machine visit",
            "refine_ms": float(np.median([r["refine_ms"] for r in pr])),
            "unrefine_ms": float(np.median([r["unrefine_ms"] for r in pr])),
            "refine_ms_spread": [min(r["refine_ms"] for r in pr), max(r["refine_ms"] for r in pr)],
            "unrefine_ms_spread": [min(r["unrefine_ms"] for r in pr), max(r["unrefine_ms"] for r in pr)], "runs": pr}
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_fields_adapt.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


def _median_ms(g, call, warmup, steps):
    """The median of `steps` synchronized calls after `warmup` of them."""
    for _ in range(warmup):
        call()
    g.synchronize()
    t = []
    for _ in range(max(steps, 1)):
        t0 = time.perf_counter()
        call()
        g.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), t


def measure_deposit(a, Kd, what):
    """Deposit (Kd = 4: position and q) or gather (Kd = 7: position, q and
    three gathered doubles) on a fresh base^3 periodic grid with ppc records
    per cell, and one re-lay of that pool."""
    import dccrg_amd
    from dccrg_amd._lib import check, lib

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(0).set_periodic(True, True, True).initialize()
    fld = g.add_variable_field("particles", np.float64, True)
    ids = g.slot_ids()[: g.n_local]
    nc = ids.size
    k = (ids - np.uint64(1)).astype(np.int64)
    ix = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1)
    rng = np.random.default_rng(1)
    rec = np.zeros((nc, a.ppc, Kd))
    rec[:, :, 0:3] = ix.astype(np.float64)[:, None, :] + rng.random((nc, a.ppc, 3))
    rec[:, :, 3] = rng.random((nc, a.ppc))
    charge = float(rec[:, :, 3].sum())
    rec = rec.reshape(-1)
    fld.resize(np.full(nc, a.ppc * Kd, np.uint64))
    check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, rec.ctypes.data_as(C.c_void_p), rec.nbytes))
    del rec
    n_particles = nc * a.ppc
    res = dict(cells=int(nc), particles=int(n_particles), K=Kd)
    out = g.add_field("rho", np.float64, False)
    if what == "deposit":
        for shape in ("cic", "ngp"):
            ms, runs = _median_ms(g, lambda: g.particles_deposit(fld, out, Kd, 3, shape), a.warmup, a.steps)
            total = float(out.get(0, nc).sum())
            assert abs(total - charge) <= 1e-9 * charge, (shape, total, charge)  # a periodic grid keeps every share
            res[shape] = dict(ms=ms, runs_ms=runs, alg_bytes=n_particles * 8 * Kd + nc * 8)
    else:
        fields = [g.add_field(f"F{j}", np.float64, False) for j in range(3)]
        for j, f in enumerate(fields):
            f.set(np.full(g.n_slots, 1.0 + j))
        ms, runs = _median_ms(g, lambda: g.particles_gather(fld, fields, 4, Kd, "cic"), a.warmup, a.steps)
        got = fld.get(0, 1)[0].reshape(-1, Kd)
        assert np.allclose(got[:, 4:7], [1.0, 2.0, 3.0], rtol=1e-12), got[:2]  # constant fields come back
        res["cic"] = dict(ms=ms, runs_ms=runs, fields=3, alg_bytes=n_particles * (8 * Kd + 8 * 3) + nc * 8 * 3)
    cur = fld.sizes(0, nc) // np.uint64(8)
    relay, _ = _median_ms(g, lambda: fld.resize(cur), 1, 3)
    res["relay_ms"] = relay
    g.close()
    return res


def main_deposit(a):
    """CIC and NGP deposit (K = 4) and a CIC gather of three fields (K = 7:
    the three gathered doubles need their place in the record), each the
    median of the timed calls after the warm-up, beside the particle step and
    the re-lay of the default bench in the same run."""
    dep = measure_deposit(a, 4, "deposit")
    gat = measure_deposit(a, 7, "gather")
    step = measure(a)
    n_particles = dep["particles"]

    def row(r, pool):
        ach = r["alg_bytes"] / (r["ms"] / 1e3) / 1e9
        return dict(r, particle_updates_per_s=n_particles / (r["ms"] / 1e3), relays=r["ms"] / step["relay_ms"],
                    relays_of_its_own_pool=r["ms"] / pool["relay_ms"], over_step=r["ms"] / step["ms"],
                    roofline={"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                              "frac": ach / PEAK_HBM_GBS})

    line = {"metric": "particles_deposit", "value": n_particles / (dep["cic"]["ms"] / 1e3),
            "unit": "particle-updates/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
            "ms_per_call": dep["cic"]["ms"], "higher_is_better": True, "dtype": "fp64",
            "config": {"workload": f"particles in cells, {a.base}^3 periodic, R = 0, neighborhood 1, {a.ppc} per cell; "
                                   "deposit of double 3 with K = 4, gather of three fields into doubles 4..6 with "
                                   "K = 7; every call synchronized, the median of the timed calls",
                       "cells": dep["cells"], "particles": n_particles},
            "deposit_cic": row(dep["cic"], dep), "deposit_ngp": row(dep["ngp"], dep), "gather_cic": row(gat["cic"], gat),
            "alg_bytes": "deposit: 8 K per record read once + 8 per cell written; gather: 8 K + 8 n per record + "
                         "8 n per cell",
            "step": {"what": "particles_step of the default bench (K = 3) in the same run", "ms": step["ms"],
                     "movers_per_step": step["movers_per_step"]},
            "relay": {"what": "VariableField.resize, sizes unchanged (copy once): the default bench's K = 3 pool, "
                              "and the K = 4 and K = 7 pools measured here",
                      "ms": step["relay_ms"], "ms_K4": dep["relay_ms"], "ms_K7": gat["relay_ms"]}}
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_deposit.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


class _DeviceArray:
    """A fixed fp64 field's device array as torch sees it (no copy)."""

    def __init__(self, field, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(field.device_ptr()), False),
                                         "version": 2}


def _torch_view(field, n):
    import torch

    return torch.as_tensor(_DeviceArray(field, n), device="cuda")


PIC_K, PIC_Q, PIC_E = 10, 6, 7  # record: position, velocity, q, E
PIC_STAGES = ("deposit", "rhs", "solve", "halo_phi", "gradient", "halo_E", "gather", "accelerate", "step")
# gradient_kernel per local cell: phi 8 B + face row 24 B + three outputs 24 B, the minimum; its own level byte and
# the gathered neighbor values (6 x 8 B) and levels (6 x 1 B) are cache hits on a grid in slot order
GRADIENT_MIN_BYTES, GRADIENT_GATHER_BYTES = 56, 1 + 6 * 8 + 6


def _refine_slab(g, n):
    """--adapt's mesh: the z-slab of one eighth of a base^3, R = 1 grid refined."""
    ids = g.slot_ids()[: g.n_local]
    k = (ids - np.uint64(1)).astype(np.int64)
    for c in ids[k // (n * n) < max(n // 8, 1)]:
        g.refine_completely(int(c))
    g.stop_refining()


def measure_gradient(a, refined):
    """dccrgx_gradient alone on base^3 periodic cells (refined: R = 1 with
    --adapt's z-slab refined): the median of the synchronized calls."""
    import dccrg_amd

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(1 if refined else 0).set_periodic(True, True, True).initialize()
    if refined:
        _refine_slab(g, n)
    phi = g.add_field("phi", np.float64, False)
    out = [g.add_field(nm, np.float64, False) for nm in ("Ex", "Ey", "Ez")]
    phi.set(np.random.default_rng(2).random(g.n_slots))
    ms, runs = _median_ms(g, lambda: g.gradient(phi, out, -1.0), a.warmup, a.steps)
    # the same calls between device events (dccrgx_kernel_timing): the kernel without the launch and the
    # synchronization the host clock includes
    g.kernel_timing(1)
    for _ in range(max(a.steps, 1)):
        g.gradient(phi, out, -1.0)
    g.synchronize()
    kms, kn = g.kernel_timing(0)
    kernel_ms = kms / max(kn, 1)
    nc = int(g.n_local)
    g.close()

    def roofline(t):
        ach = nc * GRADIENT_MIN_BYTES / (t / 1e3) / 1e9
        return {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": ach / PEAK_HBM_GBS}

    return dict(ms=ms, runs_ms=runs, kernel_ms=kernel_ms, kernel_launches=int(kn), cells=nc,
                min_bytes_per_cell=GRADIENT_MIN_BYTES, gathered_bytes_per_cell=GRADIENT_GATHER_BYTES,
                roofline=roofline(ms), roofline_kernel=roofline(kernel_ms))


def measure_pic(a):
    """warmup + steps electrostatic cycles on base^3 periodic cells, R = 0, ppc
    records of K = 10 per cell: every stage synchronized and timed on its own,
    the medians over the timed cycles."""
    import torch

    import dccrg_amd
    from dccrg_amd._lib import check, lib

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(0).set_periodic(True, True, True).initialize()
    fld = g.add_variable_field("particles", np.float64, True)
    ids = g.slot_ids()[: g.n_local]
    nc = ids.size
    k = (ids - np.uint64(1)).astype(np.int64)
    ix = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1)
    rng = np.random.default_rng(1)
    rec = np.zeros((nc, a.ppc, PIC_K))
    rec[:, :, 0:3] = ix.astype(np.float64)[:, None, :] + rng.random((nc, a.ppc, 3))
    rec[:, :, 3:6] = 0.2 * (rng.random((nc, a.ppc, 3)) - 0.5)
    rec[:, :, PIC_Q] = 1 + 0.1 * np.cos(2 * np.pi * rec[:, :, 0] / n)
    rec = rec.reshape(-1)
    fld.resize(np.full(nc, a.ppc * PIC_K, np.uint64))
    check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, rec.ctypes.data_as(C.c_void_p), rec.nbytes))
    del rec
    n_particles = nc * a.ppc
    rho = g.add_field("rho", np.float64, False)
    rhs = g.add_field("rhs", np.float64, False)
    phi = g.add_field("solution", np.float64, True)
    E = [g.add_field(nm, np.float64, True) for nm in ("Ex", "Ey", "Ez")]
    solver = dccrg_amd.Poisson_Solve(max_iterations=a.pic_iterations, min_iterations=a.pic_iterations)
    solver.cache_system_info(ids, g, rhs=rhs, solution=phi)
    t_rho, t_rhs = _torch_view(rho, nc), _torch_view(rhs, nc)
    factor = [0.0]

    def make_rhs():
        torch.sub(t_rho.mean(), t_rho, out=t_rhs)  # -(rho - mean rho)
        torch.cuda.synchronize()

    stages = {
        "deposit": lambda: g.particles_deposit(fld, rho, PIC_K, PIC_Q, "cic", per_volume=True),
        "rhs": make_rhs,
        "solve": lambda: solver.solve(ids, g, cache_is_up_to_date=True, rhs=rhs, solution=phi),
        "halo_phi": g.update_copies_of_remote_neighbors,
        "gradient": lambda: g.gradient(phi, E, -1.0),
        "halo_E": g.update_copies_of_remote_neighbors,
        "gather": lambda: g.particles_gather(fld, E, PIC_E, PIC_K, "cic"),
        "accelerate": lambda: g.particles_accelerate(fld, PIC_E, PIC_K, factor[0], PIC_Q),
        "step": lambda: g.particles_step(fld, PIC_K, None, 1.0),
    }
    times = {s: [] for s in PIC_STAGES}
    cycles = a.warmup + max(a.steps, 1)
    st = None
    for cycle in range(cycles):
        for s in PIC_STAGES:
            g.synchronize()
            t0 = time.perf_counter()
            r = stages[s]()
            g.synchronize()
            if cycle >= a.warmup:
                times[s].append((time.perf_counter() - t0) * 1e3)
            if s == "gradient" and cycle == 0:
                # the kick of all cycles together stays below 0.01 cell lengths a step
                emax = max(float(_torch_view(f, nc).abs().max()) for f in E)
                factor[0] = 0.01 / (1.1 * max(emax, 1e-300) * cycles)
            if s == "step":
                st = r
    assert st["lost"] == 0 and st["stayed"] + st["moved"] == n_particles, st
    left = int(fld.sizes(0, nc).sum()) // (8 * PIC_K)
    assert left == n_particles, left
    g.close()
    med = {s: float(np.median(times[s])) for s in PIC_STAGES}
    return dict(cells=int(nc), particles=int(n_particles), K=PIC_K, solve_iterations=a.pic_iterations,
                ms=med, sum_ms=float(sum(med.values())), runs_ms=times, accelerate_factor=factor[0])


def main_pic(a):
    """The electrostatic cycle stage by stage, and dccrgx_gradient alone on
    the uniform grid and on --adapt's refined one."""
    pic = measure_pic(a)
    grad = measure_gradient(a, False)
    grad_refined = measure_gradient(a, True)
    new = pic["ms"]["gradient"] + pic["ms"]["accelerate"]
    line = {"metric": "pic_cycle", "value": pic["particles"] / (pic["sum_ms"] / 1e3), "unit": "particle-updates/s",
            "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "ms_per_cycle": pic["sum_ms"], "higher_is_better": True,
            "dtype": "fp64",
            "config": {"workload": f"electrostatic particle-in-cell cycle, {a.base}^3 periodic, R = 0, neighborhood 1, "
                                   f"{a.ppc} records of K = {PIC_K} per cell: CIC deposit per volume, rhs = -(rho - mean) "
                                   f"with torch on the fields' device arrays, {a.pic_iterations} BiCG iterations "
                                   "(min = max), gradient with scale -1, CIC gather of three fields, accelerate, step "
                                   "with per-record velocities; every stage synchronized, medians over the timed cycles",
                       "cells": pic["cells"], "particles": pic["particles"]},
            "stages_ms": pic["ms"], "sum_ms": pic["sum_ms"],
            "gradient_plus_accelerate": {"ms": new, "share_of_cycle": new / pic["sum_ms"]},
            "accelerate_factor": pic["accelerate_factor"], "runs_ms": pic["runs_ms"],
            "gradient": grad, "gradient_refined": grad_refined,
            "gradient_bytes": "minimum per cell: phi 8 + face row 24 + three outputs 24 = 56; gathered through the "
                              "caches: the cell's level byte, six neighbor values (48) and six level bytes"}
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_pic.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


MOMENTS_RHO_J_P = [(None, None), (3, None), (4, None), (5, None),
                   (3, 3), (3, 4), (3, 5), (4, 4), (4, 5), (5, 5)]


def _alternating_ms(g, calls, warmup, steps):
    """warmup + steps rounds over `calls` (name -> callable) in turn, each call
    synchronized; per name the median, min, max and every timed run."""
    t = {k: [] for k in calls}
    for i in range(warmup + max(steps, 1)):
        for name, call in calls.items():
            g.synchronize()
            t0 = time.perf_counter()
            call()
            g.synchronize()
            if i >= warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), runs_ms=v) for k, v in t.items()}


def _moments_pool(a, Kp):
    """base^3 periodic cells with ppc records of Kp doubles: uniform positions,
    small velocities, q = 1 + 0.1 cos, the rest zero."""
    import dccrg_amd
    from dccrg_amd._lib import check, lib

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(0).set_periodic(True, True, True).initialize()
    fld = g.add_variable_field("particles", np.float64, True)
    ids = g.slot_ids()[: g.n_local]
    nc = ids.size
    k = (ids - np.uint64(1)).astype(np.int64)
    ix = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1)
    rng = np.random.default_rng(1)
    rec = np.zeros((nc, a.ppc, Kp))
    rec[:, :, 0:3] = ix.astype(np.float64)[:, None, :] + rng.random((nc, a.ppc, 3))
    rec[:, :, 3:6] = 0.2 * (rng.random((nc, a.ppc, 3)) - 0.5)
    rec[:, :, PIC_Q] = 1 + 0.1 * np.cos(2 * np.pi * rec[:, :, 0] / n)
    sums = [float(rec[:, :, PIC_Q].sum()), float((rec[:, :, PIC_Q] * rec[:, :, 3]).sum())]
    rec = rec.reshape(-1)
    fld.resize(np.full(nc, a.ppc * Kp, np.uint64))
    check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, rec.ctypes.data_as(C.c_void_p), rec.nbytes))
    del rec
    return g, fld, int(nc), sums


def measure_moments(a):
    g, fld, nc, sums = _moments_pool(a, PIC_K)
    rho = g.add_field("rho", np.float64, False)
    outs = [g.add_field(f"m{j}", np.float64, False) for j in range(10)]
    calls = {"deposit": lambda: g.particles_deposit(fld, rho, PIC_K, PIC_Q, "cic")}
    for n in (1, 4, 10):
        calls[f"moments_{n}"] = (lambda n=n: g.particles_deposit_moments(fld, outs[:n], MOMENTS_RHO_J_P[:n], PIC_K,
                                                                        PIC_Q, "cic"))
    res = _alternating_ms(g, calls, a.warmup, a.steps)
    # the ten-moment call ran last: its charge has the deposit's bits, its current sums to the records'
    assert np.array_equal(rho.get(0, nc).view(np.uint64), outs[0].get(0, nc).view(np.uint64))
    assert abs(float(outs[0].get(0, nc).sum()) - sums[0]) <= 1e-9 * sums[0]
    assert abs(float(outs[1].get(0, nc).sum()) - sums[1]) <= 1e-9 * sums[0]
    g.close()
    return res, nc


def measure_kicks(a):
    Kb, E0, B0 = 13, 7, 10  # position, velocity, q, E, B
    g, fld, nc, _ = _moments_pool(a, Kb)
    fields = [g.add_field(nm, np.float64, False) for nm in ("Ex", "Ey", "Ez", "Bx", "By", "Bz")]
    for f, v in zip(fields, (1e-3, -2e-3, 5e-4, 0.05, -0.02, 1.0)):
        f.set(np.full(g.n_slots, v))
    calls = {"gather_3": lambda: g.particles_gather(fld, fields[:3], E0, Kb, "cic"),
             "gather_6": lambda: g.particles_gather(fld, fields, E0, Kb, "cic"),
             "accelerate": lambda: g.particles_accelerate(fld, E0, Kb, 1e-3, PIC_Q),
             "boris": lambda: g.particles_boris(fld, E0, B0, Kb, 1e-3, PIC_Q)}
    res = _alternating_ms(g, calls, a.warmup, a.steps)
    got = fld.get(0, 1)[0].reshape(-1, Kb)
    assert np.allclose(got[:, 7:13], [1e-3, -2e-3, 5e-4, 0.05, -0.02, 1.0], rtol=1e-12), got[:2]
    assert np.all(np.abs(got[:, 3:6]) < 0.2)  # the kicks stayed small
    g.close()
    return res


def main_moments(a):
    """The fused moments against single deposits, and the Boris kick and the
    six-field gather against their three-double counterparts."""
    dep, nc = measure_moments(a)
    kick = measure_kicks(a)
    d = dep["deposit"]

    def against(n):
        m = dep[f"moments_{n}"]
        return {"ratio_to_one_deposit": m["ms"] / d["ms"], "calls_replaced": n,
                "max_ms": m["max_ms"], "replaced_min_ms": n * d["min_ms"],
                "cheaper_beyond_the_spread": bool(m["max_ms"] < n * d["min_ms"])}

    line = {"metric": "particles_deposit_moments", "value": dep["moments_4"]["ms"], "unit": "ms", "n_gpus": 1,
            "steps": a.steps, "warmup": a.warmup, "higher_is_better": False, "dtype": "fp64",
            "config": {"workload": f"{a.base}^3 periodic, R = 0, neighborhood 1, {a.ppc} records per cell; CIC, not per "
                                   f"volume; deposit and moments on a K = {PIC_K} pool (weight double {PIC_Q}; moments "
                                   "rho, J, P in that order), gathers and kicks on a K = 13 pool (E at 7, B at 10); the "
                                   "calls of a pool alternate, every call synchronized, median and min - max of the "
                                   "timed calls", "cells": nc, "particles": nc * a.ppc},
            "deposit": d, "moments_1": dep["moments_1"], "moments_4": dep["moments_4"], "moments_10": dep["moments_10"],
            "moments_1_within_deposit_spread": bool(d["min_ms"] <= dep["moments_1"]["ms"] <= d["max_ms"]),
            "moments_4_against_4_deposits": against(4), "moments_10_against_10_deposits": against(10),
            "gather_3": kick["gather_3"], "gather_6": kick["gather_6"],
            "gather_6_over_gather_3": kick["gather_6"]["ms"] / kick["gather_3"]["ms"],
            "accelerate": kick["accelerate"], "boris": kick["boris"],
            "boris_over_accelerate": kick["boris"]["ms"] / kick["accelerate"]["ms"]}
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_moments.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


# curl_kernel per local cell: three inputs 24 B + face row 24 B + three outputs 24 B (read too when accumulating);
# divergence_kernel: 24 + 24 + 8; field_axpy_kernel: x and y read, y written; the composition the calls replace:
# three gradients of two outputs each (8 + 24 + 16) and three axpys
CURL_MIN_BYTES, CURL_ACC_BYTES, DIVERGENCE_MIN_BYTES, AXPY_BYTES = 72, 96, 56, 24
COMPOSED_CURL_BYTES = 3 * (8 + 24 + 16) + 3 * AXPY_BYTES
CURL_NEXT = (1, 2, 0)


def measure_curl(a, refined):
    """dccrgx_curl (plain and accumulating), dccrgx_divergence, dccrgx_gradient
    and dccrgx_field_axpy, and the curl composed from the calls there were
    before them (three gradients into six scratch fields, three axpys), on
    measure_gradient's grid; the calls alternate in one run, each synchronized."""
    import dccrg_amd

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(1 if refined else 0).set_periodic(True, True, True).initialize()
    if refined:
        _refine_slab(g, n)
    nc = int(g.n_local)
    rng = np.random.default_rng(2)
    F = [g.add_field(nm, np.float64, False) for nm in ("Fx", "Fy", "Fz")]
    for f in F:
        f.set(rng.random(g.n_slots))
    out = [g.add_field(nm, np.float64, False) for nm in ("Cx", "Cy", "Cz")]
    acc = [g.add_field(nm, np.float64, False) for nm in ("Bx", "By", "Bz")]
    for f in acc:
        f.set(np.zeros(g.n_slots))
    div = g.add_field("div", np.float64, False)
    grad = [g.add_field(nm, np.float64, False) for nm in ("Gx", "Gy", "Gz")]
    # P[k] = D_d1(F_d2), Q[k] = D_d2(F_d1) with (k, d1, d2) cyclic: the gradient of F_j fills P[j + 1] and Q[j + 2]
    P = [g.add_field(f"P{k}", np.float64, False) for k in range(3)]
    Q = [g.add_field(f"Q{k}", np.float64, False) for k in range(3)]
    y = g.add_field("y", np.float64, False)
    y.set(np.zeros(g.n_slots))

    def composed():
        for j in range(3):
            o = [None, None, None]
            k_p, k_q = CURL_NEXT[j], CURL_NEXT[CURL_NEXT[j]]  # j = d2 of k_p, j = d1 of k_q
            o[CURL_NEXT[k_p]] = P[k_p]
            o[CURL_NEXT[CURL_NEXT[k_q]]] = Q[k_q]
            g.gradient(F[j], o, 1.0)
        for k in range(3):
            g.field_axpy(P[k], -1.0, Q[k])

    calls = {"curl": lambda: g.curl(F, out, 1.0),
             "curl_accumulate": lambda: g.curl(F, acc, -1e-3, True),
             "divergence": lambda: g.divergence(F, div, 1.0),
             "gradient": lambda: g.gradient(F[0], grad, -1.0),
             "field_axpy": lambda: g.field_axpy(y, 1e-3, F[0]),
             "composed_curl": composed}
    res = _alternating_ms(g, calls, a.warmup, a.steps)
    # the composition's result is the fused call's, bit for bit
    for k in range(3):
        assert np.array_equal(out[k].get(0, nc).view(np.uint64), P[k].get(0, nc).view(np.uint64)), k
    # the fused kernels between device events (dccrgx_kernel_timing), as measure_gradient takes the gradient's
    for name in ("curl", "curl_accumulate", "divergence"):
        g.kernel_timing(1)
        for _ in range(max(a.steps, 1)):
            calls[name]()
        g.synchronize()
        kms, kn = g.kernel_timing(0)
        res[name]["kernel_ms"] = kms / max(kn, 1)
        res[name]["kernel_launches"] = int(kn)
    g.close()

    def roofline(t, b):
        ach = nc * b / (t / 1e3) / 1e9
        return {"bound": "hbm", "bytes_per_cell": b, "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": ach / PEAK_HBM_GBS}

    for name, b in (("curl", CURL_MIN_BYTES), ("curl_accumulate", CURL_ACC_BYTES), ("divergence", DIVERGENCE_MIN_BYTES),
                    ("gradient", GRADIENT_MIN_BYTES), ("field_axpy", AXPY_BYTES), ("composed_curl", COMPOSED_CURL_BYTES)):
        res[name]["roofline"] = roofline(res[name]["ms"], b)
        if "kernel_ms" in res[name]:
            res[name]["roofline_kernel"] = roofline(res[name]["kernel_ms"], b)
    res["cells"] = nc
    res["curl_over_composed_curl"] = res["curl"]["ms"] / res["composed_curl"]["ms"]
    res["curl_over_gradient"] = res["curl"]["ms"] / res["gradient"]["ms"]
    met = bool(res["curl"]["max_ms"] < res["composed_curl"]["min_ms"])
    res["fused_max_below_composed_min"] = {"curl_max_ms": res["curl"]["max_ms"],
                                           "composed_min_ms": res["composed_curl"]["min_ms"],
                                           "verdict": "met" if met else "not met"}
    return res


def main_curl(a):
    """The fused curl and divergence against the gradient and against the
    composition from gradients and axpys, on the uniform and the refined grid."""
    uni = measure_curl(a, False)
    ref = measure_curl(a, True)
    line = {"metric": "curl", "value": uni["curl"]["ms"], "unit": "ms", "n_gpus": 1, "steps": a.steps,
            "warmup": a.warmup, "higher_is_better": False, "dtype": "fp64",
            "config": {"workload": f"{a.base}^3 periodic, neighborhood 1: R = 0, and R = 1 with a z-slab of one eighth "
                                   "refined; the six calls alternate in one run, every call synchronized (host clock), "
                                   "median and min - max of the timed calls; kernel_ms: the same call between device "
                                   "events; composed_curl: three gradient calls of two outputs each into six scratch "
                                   "fields and three field_axpy calls, bitwise the fused curl's result"},
            "bytes_per_cell": {"curl": "3 inputs 24 + face row 24 + 3 outputs 24 = 72 (+ 24 accumulating)",
                               "divergence": "24 + 24 + 8 = 56", "field_axpy": "x 8 + y 8 read, y 8 written = 24",
                               "composed_curl": "3 x (8 + 24 + 16) + 3 x 24 = 216"},
            "uniform": uni, "refined": ref}
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_curl.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


# field_reduce_kernel per local cell: the seven fields of the energy call, 56 B (+ the level byte on a refined grid,
# where the volume follows the level); the particle reduce names 4 of a record's 10 doubles (32 B of its 80 B)
REDUCE_FIELD_BYTES = 56


def _event_and_host_ms(g, calls, warmup, steps):
    """warmup + steps rounds over `calls` in turn; per name the time between
    device events (dccrgx_kernel_timing, summed over the call's launches; None
    for a call that times nothing) and the synchronized host clock."""
    ev, host = {k: [] for k in calls}, {k: [] for k in calls}
    for i in range(warmup + max(steps, 1)):
        for name, call in calls.items():
            g.synchronize()
            g.kernel_timing(1)
            t0 = time.perf_counter()
            call()
            g.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            kms, kn = g.kernel_timing(0)
            if i >= warmup:
                host[name].append(dt)
                if kn:
                    ev[name].append(kms)
    res = {}
    for k in calls:
        res[k] = dict(host_ms=float(np.median(host[k])), host_min_ms=float(min(host[k])), host_max_ms=float(max(host[k])))
        if ev[k]:
            res[k].update(ms=float(np.median(ev[k])), min_ms=float(min(ev[k])), max_ms=float(max(ev[k])), runs_ms=ev[k])
    return res


def measure_reduce_fields(a, refined):
    """The seven-term energy call (six squares by volume and max |div B|)
    against the same values from seven single-term calls, field_axpy and the
    host way (download of the seven fields and NumPy), interleaved in one run."""
    import torch

    import dccrg_amd

    n = a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(1 if refined else 0).set_periodic(True, True, True).initialize()
    if refined:
        _refine_slab(g, n)
    g.set_geometry((0, 0, 0), (1, 1, 1))
    nc = int(g.n_local)
    rng = np.random.default_rng(2)
    F = [g.add_field(nm, np.float64, False) for nm in ("Ex", "Ey", "Ez", "Bx", "By", "Bz", "div")]
    for f in F:
        f.set(rng.random(g.n_slots) * 2 - 1)
    y = g.add_field("y", np.float64, False)
    y.set(np.zeros(g.n_slots))
    terms = [("sum", f, f) for f in F[:6]] + [("max_abs", F[6], None)]
    one, seven = torch.zeros(7, dtype=torch.float64, device="cuda"), torch.zeros(7, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    host = {}

    def host_way():
        v = [f.get(0, nc) for f in F]
        host["values"] = [float(np.dot(x, x)) for x in v[:6]] + [float(np.max(np.abs(v[6])))]

    calls = {"reduce_7_terms": lambda: g.field_reduce(terms, True, out=one),
             "reduce_7_calls": lambda: [g.field_reduce([t], True, out=seven[j:j + 1]) for j, t in enumerate(terms)],
             "field_axpy": lambda: g.field_axpy(y, 1e-3, F[0]),
             "host_way": host_way}
    res = _event_and_host_ms(g, calls, a.warmup, a.steps)
    g.synchronize()
    got, single = one.cpu().numpy(), seven.cpu().numpy()
    # one call and seven calls give the same bits (the order depends on the number of cells only)
    assert np.array_equal(got.view(np.uint64), single.view(np.uint64)), (got, single)
    assert got[6] == host["values"][6]
    if not refined:  # (V = 1: the host's sums are the same sums)
        assert np.allclose(got[:6], host["values"][:6], rtol=1e-12, atol=0), (got, host["values"])
    g.close()
    b = REDUCE_FIELD_BYTES + (1 if refined else 0)

    def roofline(t, bytes_per_cell):
        ach = nc * bytes_per_cell / (t / 1e3) / 1e9
        return {"bound": "hbm", "bytes_per_cell": bytes_per_cell, "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": ach / PEAK_HBM_GBS}

    for name, bb in (("reduce_7_terms", b), ("reduce_7_calls", b + (5 if refined else 0)), ("field_axpy", AXPY_BYTES)):
        res[name]["roofline"] = roofline(res[name]["ms"], bb)
    res["cells"] = nc
    res["host_way"]["bytes_moved"] = 7 * 8 * nc
    res["one_call_over_seven_calls"] = res["reduce_7_terms"]["ms"] / res["reduce_7_calls"]["ms"]
    res["one_call_over_seven_calls_host_clock"] = res["reduce_7_terms"]["host_ms"] / res["reduce_7_calls"]["host_ms"]
    res["one_call_over_host_way"] = res["reduce_7_terms"]["host_ms"] / res["host_way"]["host_ms"]
    res["frac_of_peak_over_field_axpy"] = (res["reduce_7_terms"]["roofline"]["frac"] /
                                           res["field_axpy"]["roofline"]["frac"])
    return res


def measure_reduce_particles(a):
    """Count, charge, three momenta and three squares of every record in one
    call beside particles_accelerate, which walks the same pool."""
    import torch

    Kb, E0 = 10, 7
    g, fld, nc, sums = _moments_pool(a, Kb)
    terms = [("sum", None, None), ("sum", PIC_Q, None), ("sum", 3, None), ("sum", 4, None), ("sum", 5, None),
             ("sum", 3, 3), ("sum", 4, 4), ("sum", 5, 5)]
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    calls = {"particles_reduce": lambda: g.particles_reduce(fld, terms, Kb, -1, out=out),
             "accelerate": lambda: g.particles_accelerate(fld, E0, Kb, 1e-3, PIC_Q)}
    res = _event_and_host_ms(g, calls, a.warmup, a.steps)
    g.synchronize()
    got = out.cpu().numpy()
    assert got[0] == float(nc * a.ppc) and abs(got[1] - sums[0]) <= 1e-9 * sums[0], (got, sums)
    g.close()
    n = nc * a.ppc
    for name, bb in (("particles_reduce", 32), ("accelerate", 8 * 8)):
        t = res[name].get("ms", res[name]["host_ms"])
        res[name]["named_bytes_per_record"] = bb
        res[name]["record_bytes"] = Kb * 8
        res[name]["frac_of_peak_named"] = n * bb / (t / 1e3) / 1e9 / PEAK_HBM_GBS
        res[name]["frac_of_peak_whole_records"] = n * Kb * 8 / (t / 1e3) / 1e9 / PEAK_HBM_GBS
    res["particles"] = n
    res["reduce_over_accelerate_host_clock"] = res["particles_reduce"]["host_ms"] / res["accelerate"]["host_ms"]
    return res


def main_reduce(a):
    """The reductions of a cycle's diagnostics: one call against single-term
    calls, field_axpy and the host way on the uniform and the refined grid,
    and the particle reduce beside particles_accelerate."""
    uni = measure_reduce_fields(a, False)
    ref = measure_reduce_fields(a, True)
    par = measure_reduce_particles(a)
    line = {"metric": "field_reduce", "value": uni["reduce_7_terms"]["ms"], "unit": "ms", "n_gpus": 1, "steps": a.steps,
            "warmup": a.warmup, "higher_is_better": False, "dtype": "fp64",
            "config": {"workload": f"{a.base}^3 periodic, neighborhood 1: R = 0, and R = 1 with a z-slab of one eighth "
                                   "refined; seven terms by volume (six squares, max |div B|); the calls alternate in "
                                   "one run; ms: between device events, summed over a call's launches (two kernels a "
                                   "reduce call); host_ms: the synchronized host clock; host_way: download of the seven "
                                   f"fields and NumPy; particles: {a.ppc} records of K = 10 per cell on the uniform "
                                   "grid, eight terms (count, charge, momenta, squares), weight -1"},
            "bytes_per_cell": {"reduce_7_terms": "7 fields x 8 = 56 (+ 1 level byte on the refined grid)",
                               "reduce_7_calls": "the same 56, + 1 level byte per by-volume call on the refined grid",
                               "field_axpy": "x 8 + y 8 read, y 8 written = 24", "host_way": "56 over PCIe"},
            "uniform": uni, "refined": ref, "particles": par}
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_reduce.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


def main_create(a):
    """particles_create on the benchmark's own pool (base^3 cells, ppc records
    of K = 10): (a) into an empty pool, (b) one more record per cell behind the
    full pool, (c) the host way (NumPy generation of the same content, resize
    and one flat upload), (d) one re-lay of the full pool; --repeats rounds of
    a, b, d in turn on one grid, c twice at most."""
    import dccrg_amd
    from dccrg_amd._lib import check, lib

    Kb, n = PIC_K, a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(0).set_periodic(True, True, True).initialize()
    fld = g.add_variable_field("particles", np.float64, True)
    ids = g.slot_ids()[: g.n_local]
    nc = int(ids.size)
    k = (ids - np.uint64(1)).astype(np.int64)
    ix = np.stack([k % n, (k // n) % n, k // (n * n)], axis=1).astype(np.float64)
    dens = g.add_field("density", np.float64, False)
    dens.set(1 + 0.1 * np.cos(2 * np.pi * (ix[:, 0] + 0.5) / n))
    recipe = {3: ("normal", 0.0, 0.1), 4: ("normal", 0.0, 0.1), 5: ("normal", 0.0, 0.1),
              PIC_Q: ("const", 1.0, dict(base_field=dens))}
    N = nc * a.ppc
    full = np.full(nc, a.ppc * Kb, np.uint64)
    empty = np.zeros(nc, np.uint64)

    def timed(call):
        g.synchronize()
        g.kernel_timing(1)
        t0 = time.perf_counter()
        r = call()
        g.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        kms, kn = g.kernel_timing(0)
        return dt, (kms if kn else None), r

    def host_way():
        tg = time.perf_counter()
        rng = np.random.default_rng(1)
        rec = np.zeros((nc, a.ppc, Kb))
        rec[:, :, 0:3] = ix[:, None, :] + rng.random((nc, a.ppc, 3))
        rec[:, :, 3:6] = 0.1 * rng.standard_normal((nc, a.ppc, 3))
        rec[:, :, PIC_Q] = (1 + 0.1 * np.cos(2 * np.pi * (ix[:, 0] + 0.5) / n))[:, None]
        gen_ms.append((time.perf_counter() - tg) * 1e3)
        rec = rec.reshape(-1)
        fld.resize(full)
        check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, rec.ctypes.data_as(C.c_void_p), rec.nbytes))

    # where the generate kernel's time goes: the same call with the three velocity doubles constant (positions
    # alone compute Philox blocks) and uniform (no log, sqrt, cos)
    by_content = {"velocities_constant": {PIC_Q: recipe[PIC_Q]},
                  "velocities_uniform": {**recipe, **{j: ("uniform", -0.1, 0.2) for j in (3, 4, 5)}}}
    runs = {k: dict(host_ms=[], kernel_ms=[]) for k in ("create_empty", "append_one", "host_way", "relay",
                                                         *by_content)}
    gen_ms = []
    for rnd in range(1 + max(a.repeats, 1)):  # the first round warms up
        fld.resize(empty)
        ta = timed(lambda: g.particles_create(fld, Kb, count=a.ppc, recipe=recipe, seed=rnd))
        assert ta[2] == N and int(fld.sizes(0, 4).sum()) == 4 * a.ppc * Kb * 8
        tb = timed(lambda: g.particles_create(fld, Kb, count=1.0, recipe=recipe, seed=1000 + rnd))
        assert tb[2] == nc
        fld.resize(full)
        td = timed(lambda: fld.resize(full))
        todo = [("create_empty", ta), ("append_one", tb), ("relay", td)]
        for name, rc in by_content.items():
            fld.resize(empty)
            todo.append((name, timed(lambda: g.particles_create(fld, Kb, count=a.ppc, recipe=rc, seed=rnd))))
        if rnd <= 2:
            fld.resize(empty)
            todo.append(("host_way", timed(host_way)))
        if rnd == 0:
            continue
        for name, (dt, kms, _) in todo:
            runs[name]["host_ms"].append(dt)
            if kms is not None:
                runs[name]["kernel_ms"].append(kms)
    # what was created: every record inside its cell, the weight the density's
    fld.resize(empty)
    g.particles_create(fld, Kb, count=a.ppc, recipe=recipe, seed=5)
    got = g.particles_reduce(fld, [("sum", None, None), ("sum", PIC_Q, None), ("sum", 3, None), ("sum", 3, 3)], Kb)
    st = g.particles_step(fld, Kb, (0.0, 0.0, 0.0), 0.0)
    assert got[0] == N and st["stayed"] == N and st["lost"] == 0, (got, st)
    g.close()
    res = {}
    for name, r in runs.items():
        res[name] = dict(host_ms=float(np.median(r["host_ms"])), host_runs_ms=r["host_ms"])
        if r["kernel_ms"]:
            res[name].update(kernel_ms=float(np.median(r["kernel_ms"])), kernel_runs_ms=r["kernel_ms"])
    res["host_way"]["numpy_generation_ms"] = float(np.median(gen_ms[1:] or gen_ms))
    rec_bytes = Kb * 8
    ce = res["create_empty"]
    ce["bytes_written"] = N * rec_bytes
    ce["frac_of_peak_whole_call"] = N * rec_bytes / (ce["host_ms"] / 1e3) / 1e9 / PEAK_HBM_GBS
    if "kernel_ms" in ce:
        ce["frac_of_peak_generate_kernel"] = N * rec_bytes / (ce["kernel_ms"] / 1e3) / 1e9 / PEAK_HBM_GBS
    line = {"metric": "particles_create", "value": N / (ce["host_ms"] / 1e3), "unit": "records/s", "n_gpus": 1,
            "steps": a.repeats, "warmup": 1, "higher_is_better": True, "dtype": "fp64",
            "config": {"workload": f"{n}^3 periodic cells, {a.ppc} records of K = {Kb} per cell: uniform positions, three "
                                   "normal velocity components, a weight scaled by a density field, three zero doubles "
                                   "(six of ten doubles compute a Philox block, three of them a normal); host_ms: the "
                                   "synchronized host clock around the whole call (its checks, the scan, the fresh pool "
                                   "and the re-lay included); kernel_ms: between device events around the generate kernel "
                                   "alone; host_way: NumPy generation of the same content, resize and one flat upload "
                                   "(the benchmark's own loader, quicker than VariableField.set's list of arrays); relay: "
                                   "VariableField.resize of the full pool, sizes unchanged",
                       "cells": nc, "records": N, "record_bytes": rec_bytes},
            "create_empty": ce, "append_one": res["append_one"], "host_way": res["host_way"], "relay": res["relay"],
            "create_empty_by_content": {k: res[k] for k in by_content},
            "create_over_host_way": ce["host_ms"] / res["host_way"]["host_ms"],
            "append_over_relay": res["append_one"]["host_ms"] / res["relay"]["host_ms"],
            "created_mean_v": got[2] / N, "created_var_v_over_thermal2": (got[3] / N - (got[2] / N) ** 2) / 0.01,
            "created_charge": got[1]}
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_create.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


def main_remove(a):
    """particles_remove on the benchmark's own pool (base^3 cells, ppc records
    of K = 10, made by particles_create before every timed call): (a) a
    velocity test that removes about half, (b) a mask slab of one plane of
    cells, (c) chance 0.5 with rescale, (d) a test that removes nothing, (e)
    case (a) with `into`; beside them one re-lay of the same pool
    (VariableField.resize, sizes unchanged) and, once, the host route for (a):
    flat download, NumPy filter, resize and flat upload."""
    import dccrg_amd
    from dccrg_amd._lib import check, lib

    Kb, n = PIC_K, a.base
    g = dccrg_amd.Dccrg(0, 1, 0).set_initial_length((n, n, n)).set_neighborhood_length(1)
    g.set_maximum_refinement_level(0).set_periodic(True, True, True).initialize()
    fld = g.add_variable_field("particles", np.float64, True)
    other = g.add_variable_field("removed", np.float64, False)
    ids = g.slot_ids()[: g.n_local]
    nc = int(ids.size)
    k = (ids - np.uint64(1)).astype(np.int64)
    mask = g.add_field("mask", np.float64, False)
    mask.set((k // (n * n) == n // 2).astype(np.float64))  # one plane of cells
    recipe = {3: ("normal", 0.0, 0.1), 4: ("normal", 0.0, 0.1), 5: ("normal", 0.0, 0.1), PIC_Q: ("const", 1.0)}
    N = nc * a.ppc
    full = np.full(nc, a.ppc * Kb, np.uint64)
    empty = np.zeros(nc, np.uint64)
    rec_bytes = Kb * 8
    inf = float("inf")

    def timed(call):
        g.synchronize()
        g.kernel_timing(1)
        t0 = time.perf_counter()
        r = call()
        g.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        kms, kn = g.kernel_timing(0)
        return dt, (kms if kn else None), r

    def fresh():
        fld.resize(empty)
        other.resize(empty)
        assert g.particles_create(fld, Kb, count=a.ppc, recipe=recipe, seed=1) == N

    cases = {"a_velocity_test_half": dict(tests=[(3, "drop", 0.0, inf)]),
             "b_mask_plane": dict(mask=mask),
             "c_chance_half_rescale": dict(prob=0.5, seed=7, rescale=True, weight=PIC_Q),
             "d_nothing_removed": dict(tests=[(3, "keep", -inf, inf)]),
             "e_velocity_test_half_into": dict(tests=[(3, "drop", 0.0, inf)], into=other)}

    def host_way():
        raw = np.empty(N * Kb, np.float64)
        got = C.c_size_t(0)
        check(lib().dccrgx_variable_field_download(g.h, fld.id, 0, nc, raw.ctypes.data_as(C.c_void_p), raw.nbytes,
                                                   C.byref(got)))
        rec = raw.reshape(nc, a.ppc, Kb)
        keep = ~(rec[:, :, 3] >= 0.0)
        kept = np.ascontiguousarray(rec[keep]).reshape(-1)
        fld.resize(keep.sum(axis=1).astype(np.uint64) * np.uint64(Kb))
        check(lib().dccrgx_variable_field_upload(g.h, fld.id, 0, nc, kept.ctypes.data_as(C.c_void_p), kept.nbytes))
        return int(keep.sum())

    runs = {name: dict(host_ms=[], kernel_ms=[]) for name in (*cases, "relay", "host_way")}
    counts = {}
    for rnd in range(1 + max(a.repeats, 1)):  # the first round warms up
        todo = []
        for name, kw in cases.items():
            fresh()
            t = timed(lambda: g.particles_remove(fld, Kb, **kw))
            counts[name] = t[2]
            todo.append((name, t))
        fresh()
        todo.append(("relay", timed(lambda: fld.resize(full))))
        if rnd == 1:
            fresh()
            t = timed(host_way)
            assert t[2] == counts["a_velocity_test_half"]["kept"], (t[2], counts)
            todo.append(("host_way", t))
        if rnd == 0:
            continue
        for name, (dt, kms, _) in todo:
            runs[name]["host_ms"].append(dt)
            if kms is not None:
                runs[name]["kernel_ms"].append(kms)
    for name, st in counts.items():
        assert sum(st.values()) == N, (name, st)
    assert counts["d_nothing_removed"]["kept"] == N and counts["b_mask_plane"]["by_mask"] == n * n * a.ppc
    g.close()
    res = {}
    for name, r in runs.items():
        res[name] = dict(host_ms=float(np.median(r["host_ms"])), host_runs_ms=r["host_ms"])
        if r["kernel_ms"]:
            res[name].update(kernel_ms=float(np.median(r["kernel_ms"])), kernel_runs_ms=r["kernel_ms"])
    relay, host = res["relay"]["host_ms"], res["host_way"]["host_ms"]
    chunks = (N + 63) // 64
    for name, kw in cases.items():
        st, r = counts[name], res[name]
        kept = st["kept"]
        removed = N - kept
        # the decision: one tested double per record (its 64-byte line is what HBM moves; the double is counted),
        # a mask or no field, the chunk bits and counts; (c) also reads and writes the weight of the kept
        decide = N * 8 * (1 if kw.get("tests") else 0) + (nc * 8 if "mask" in kw else 0) + chunks * 12
        if kw.get("rescale"):
            decide += 2 * 8 * kept
        moved = 0 if not removed else 2 * kept * rec_bytes + (2 * removed * rec_bytes if "into" in kw else 0)
        r.update(counts=st, decide_bytes=decide, copy_bytes=moved, alg_bytes=decide + moved,
                 over_relay=r["host_ms"] / relay, over_host_way=r["host_ms"] / host,
                 frac_of_peak_whole_call=(decide + moved) / (r["host_ms"] / 1e3) / 1e9 / PEAK_HBM_GBS)
        if "kernel_ms" in r:
            r["frac_of_peak_kernels"] = (decide + moved) / (r["kernel_ms"] / 1e3) / 1e9 / PEAK_HBM_GBS
    ra = res["a_velocity_test_half"]
    line = {"metric": "particles_remove", "value": N / (ra["host_ms"] / 1e3), "unit": "records/s", "n_gpus": 1,
            "steps": a.repeats, "warmup": 1, "higher_is_better": True, "dtype": "fp64",
            "config": {"workload": f"{n}^3 periodic cells, {a.ppc} records of K = {Kb} per cell from particles_create "
                                   "before every timed call; host_ms: the synchronized host clock around the whole call "
                                   "(checks, scans, the fresh pool and the swap included); kernel_ms: between device "
                                   "events around the decide, tally and copy kernels; relay: VariableField.resize of "
                                   "the same pool, sizes unchanged; host_way: case (a) by a flat download, a NumPy "
                                   "filter, resize and a flat upload, timed once; alg_bytes: the decision's reads, the "
                                   "kept records read and written once (and the removed ones with into), no remote "
                                   "part on one process",
                       "cells": nc, "records": N, "record_bytes": rec_bytes},
            **{name: res[name] for name in cases}, "relay": res["relay"], "host_way": res["host_way"]}
    txt = json.dumps(line)
    print(txt, flush=True)
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "particles_bench_remove.json")
    with open(out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
