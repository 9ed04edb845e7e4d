"""Every writer of a fixed-size cell field against every device cache that is
derived from field contents and kept by write epoch (dccrgx_internal.hpp:
Field::epoch, local_epoch, external, field_written, field_halo_written):

* Grid::DtCache   - advection_max_time_step(_device): the returned dt
* Grid::LenTable  - the tile sweeps' per-level lengths: advection_length_source
                    and the densities
* Grid::NbRecords - the tile sweeps' neighbor records (DCCRGX_NBREC=1): the
                    densities
* Grid::BandRec   - the face-table sweep's bands: advection_check_adaptation's
                    counts and the mesh after advection_adapt

A writer that forgets field_written raises no error: the next time step, flux
or refinement decision is computed from the field as it was before the write.

The oracle is a cold twin: a fresh grid with the same mesh that gets the warm
grid's fields, downloaded after the write, through Field.set and sweeps with
DCCRGX_LEN_TABLE=0 and without the records.  Table-fed and field-reading
sweeps, the face table and the tiles, and the time step and
advection_model.max_time_step are bitwise equal (tested elsewhere), so every
comparison here is bitwise: np.array_equal on float64, == on dt, no tolerance.
Every case also asserts that its write mattered: the time step or the next
step's densities of the twin differ from those of a twin that got the fields
as they were before the write - what a stale cache would have produced.

The mesh is test_gpu_advection_lengths.py's FB: (16, 16, 4), R = 2,
pre-refined: several tiles, out-of-tile neighbors and finer faces.

Departures from a literal reading of the writer list, each forced by the
library's own preconditions:
* CIC deposits need a neighborhood length of 1: the two deposit cases run on
  the same mesh built with neighborhood length 1 (warm grid and twin alike).
* comm_loopback needs the RCCL transport: that case builds its grids with a
  bootstrap id (a one-rank communicator), otherwise the same construction.
* load_grid_data initializes a grid and is refused on an initialized one, so
  no cache can be warm when it runs: the case loads the file into a fresh grid
  while the saving grid goes on with an edited vx, and requires the file's
  values to govern the loaded grid's time step and sweeps.
* The Poisson cases of poisson_cases.py and stretched_solver_cases.py come
  with meshes of their own (n^3 periodic boxes refined about a point, 1-D
  rows, stretched coordinates), none of which is FB: the solve runs on FB with
  poisson3d's right-hand side mapped onto FB's box, five iterations.
* A one-process grid has no outer cells: gradient with region="outer" (and
  "inner" beside it) is a writer of the two-view test, where both runs exist;
  region="inner" alone is also in the one-process matrix.
* The two views and the two processes are split in z, and a z-face's flux is
  zero while vz is: the writes there include vz, without which no remote
  copy's velocity or length could reach a density.
* With DCCRGX_NBREC=1 the sweeps never take the length table
  (ensure_len_table), so the verdict of the length check is asked with the
  variable unset for that one call (it is read per call)."""
import contextlib
import os

import numpy as np
import pytest

import advection_model as AM
import dccrg_amd
from dccrg_amd.particles_bench import _torch_view
from particles_model import seeded_particles
from poisson_cases import poisson3d_solution
from test_gpu_advection_lengths import FB, NAMES, gpu_grid, l0_of, len_table, prerefine
from test_gpu_advection_lengths import run as length_run

pytestmark = pytest.mark.gpu

SPARES = ("s0", "s1", "s2")


@contextlib.contextmanager
def nbrec(on):
    old = os.environ.pop("DCCRGX_NBREC", None)
    if on:
        os.environ["DCCRGX_NBREC"] = "1"
    try:
        yield
    finally:
        os.environ.pop("DCCRGX_NBREC", None)
        if old is not None:
            os.environ["DCCRGX_NBREC"] = old


@contextlib.contextmanager
def cold():
    """The twin's switches: the sweeps read the length fields, no records."""
    with len_table(False), nbrec(False):
        yield


def build(hood=0, rccl=False):
    """FB's mesh with three spare fp64 fields (operator inputs)."""
    base, R = FB
    if hood == 0 and not rccl:
        g, f = gpu_grid(base, R)
    else:
        g = dccrg_amd.Dccrg(0, 1, 0, dccrg_amd.Dccrg.unique_id()) if rccl else dccrg_amd.Dccrg(0, 1, 0)
        g.set_initial_length(base).set_neighborhood_length(hood)
        g.set_maximum_refinement_level(R).set_periodic(True, True, False).initialize()
        g.set_geometry((0, 0, 0), l0_of(base))
        f = [g.add_field(n, np.float64, n == "density") for n in NAMES]
    sp = [g.add_field(n, np.float64, False) for n in SPARES]
    prerefine(g, f, R)
    return g, f, sp


def fill_spares(g, sp):
    """Smooth fields of order one that depend on all three coordinates (so
    that every derivative, the z ones included, varies over the hump)."""
    c, _ = g.geometry(g.slot_ids())
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    tau = 2 * np.pi
    sp[0].set(np.sin(tau * x + 0.3) * np.cos(tau * y + 0.1) + 4.0 * z * z)
    sp[1].set(np.cos(tau * x) * np.sin(tau * y + 0.2) + 0.3 * z + 0.2 * z * z)
    sp[2].set(0.8 * (z - 0.3) + 0.3 * np.sin(tau * x) + 0.2 * np.cos(tau * y) * z)


def download(g, f):
    return np.stack([F.get() for F in f], axis=1)


def sweep(g, f, h, steps=2):
    out = []
    for _ in range(steps):
        g.advection_step(f, h)
        g.advection_commit(f[0])
        out.append(f[0].get(0, g.n_local))
    return out


def source(g, f):
    """The length check's verdict, asked without the records' switch."""
    with nbrec(False):
        return g.advection_length_source(f)


def device_dt(g, f):
    import torch

    t = torch.zeros(1, dtype=torch.float64, device="cuda")
    g.advection_max_time_step_device(f, t)
    g.synchronize()
    return float(t.cpu()[0])


def lengths_are_the_geometry(g, ids, cols):
    lvl = g.mapping_batch(ids)["level"]
    l0 = l0_of(FB[0])
    return all(np.array_equal(cols[:, 4 + d], l0[d] * (1.0 / np.ldexp(1.0, lvl))) for d in range(3))


def warm(g, f, sp, table=True):
    """Tiles, the length table, the records when switched on and the dt
    cache built; returns the initial time step and the step length used
    throughout the case."""
    fill_spares(g, sp)
    dt0 = g.advection_max_time_step(f)
    h = 0.25 * dt0
    sweep(g, f, h)
    assert source(g, f) == int(table)
    return dt0, h


def rewarm(g, f, h):
    g.advection_max_time_step(f)
    sweep(g, f, h)
    source(g, f)


_cold_runs = {}


def cold_run(make, ids, cols, h, share=False):
    """dt and the densities of two steps of a cold twin holding `cols`."""
    key = (ids.tobytes(), cols.tobytes(), h)
    if share and key in _cold_runs:
        return _cold_runs[key]
    with cold():
        g, f, _ = make()
        assert np.array_equal(g.slot_ids(), ids)
        for k in range(7):
            f[k].set(cols[:, k])
        lay = g.advection_layout()  # the first step already runs the tile kernels
        assert lay["tiles"] >= 2 and lay["finer_faces"] > 0, lay
        dt = g.advection_max_time_step(f)
        dens = sweep(g, f, h)
        assert g.advection_length_source(f) == 0
        g.close()
    if share:
        _cold_runs[key] = (dt, dens)
    return dt, dens


def differs_on_common_cells(ids_a, a, ids_b, b):
    """Whether two meshes' densities differ on the cells both have (the same
    mesh: anywhere)."""
    _, ia, ib = np.intersect1d(ids_a[: a.size], ids_b[: b.size], return_indices=True)
    assert ia.size > 0
    return not np.array_equal(a[ia], b[ib])


def check_after_write(writer, records, prepare=None, hood=0, rccl=False, replay=False):
    """The warm grid's consumers after `writer` against the cold twin's; the
    guard that the write mattered; returns the figures for the case's own
    assertions.  `prepare` runs before a second warm-up (state a case starts
    from); `replay`: the writer changes the mesh, so the twin gets its mesh by
    going through the same calls, and the guard compares the densities of the
    cells that both meshes have."""
    st = {}
    with nbrec(records):
        g, f, sp = build(hood, rccl)
        dt0, h = warm(g, f, sp)
        if prepare is not None:
            prepare(g, f, sp, st)
            rewarm(g, f, h)
        dt_before = g.advection_max_time_step(f)
        ids0, before = g.slot_ids(), download(g, f)
        writer(g, f, sp, st)
        ids, cols = g.slot_ids(), download(g, f)
        n = g.n_local
        dt_w = g.advection_max_time_step(f)
        dt_dev = device_dt(g, f)
        src = source(g, f)
        dens = sweep(g, f, h)
        src_end = source(g, f)
        expect_src = int(lengths_are_the_geometry(g, ids, cols))
        g.close()

    def make():
        return build(hood, rccl)

    def make_replayed():
        t, tf, tsp = build(hood, rccl)
        _, th = warm(t, tf, tsp, table=False)
        assert th == h
        ts = {}
        if prepare is not None:
            prepare(t, tf, tsp, ts)
            rewarm(t, tf, th)
        writer(t, tf, tsp, ts)
        return t, tf, tsp

    dt_t, dens_t = cold_run(make_replayed if replay else make, ids, cols, h)
    dt_s, dens_s = cold_run(make, ids0, before, h, share=True)
    dt_changed = dt_t != dt_before
    rho_changed = differs_on_common_cells(ids, dens_t[0], ids0, dens_s[0])
    print(f"dt0 {dt0!r} before {dt_before!r} warm {dt_w!r} device {dt_dev!r} twin {dt_t!r} stale twin {dt_s!r} "
          f"source {src} (expected {expect_src}) dt changed {dt_changed} densities changed {rho_changed}")
    assert dt_s == dt_before
    assert dt_t == AM.max_time_step(cols[:n])
    assert dt_w == dt_t, ("stale time step", dt_w, dt_t, dt_before)
    assert dt_dev == dt_w
    for k, (x, y) in enumerate(zip(dens, dens_t)):
        assert np.array_equal(x, y), ("densities differ from the twin's at step", k)
    assert src == expect_src and src_end == expect_src
    # the write mattered: a stale cache would have given dt_before / dens_s
    assert dt_changed or rho_changed
    return dict(dt0=dt0, dt_before=dt_before, dt=dt_w, src=src, dt_changed=dt_changed, rho_changed=rho_changed)


# ---- the writers --------------------------------------------------------------
def hump_run(g, f, n=100):
    """A run of n local slots around the top of the hump."""
    top = int(np.argmax(f[0].get(0, g.n_local)))
    return max(0, min(top - n // 2, g.n_local - n))


def w_set_whole(g, f, sp, st):
    f[2].set(f[2].get() * 1.5)


def w_set_run(g, f, sp, st):
    f[1].set(np.full(100, 3.0), hump_run(g, f))


def w_axpy(k):
    def w(g, f, sp, st):
        if k < 4:
            g.field_axpy(f[k], 4.0, sp[k - 1])
        else:
            g.field_axpy(f[k], 0.5, f[4 + (k - 3) % 3])  # a positive multiple of another length
    return w


def w_gradient(outs, region="all"):
    def w(g, f, sp, st):
        g.gradient(sp[0], [f[1 + d] if d in outs else None for d in range(3)], 0.5, region)
    return w


def w_curl(accumulate):
    def w(g, f, sp, st):
        g.curl(sp, f[1:4], 0.5, accumulate)
    return w


def w_divergence(accumulate):
    def w(g, f, sp, st):
        g.divergence(sp, f[1], 0.5, accumulate)
    return w


def particles(g, seed):
    """0..3 records of four doubles (position, a weight in [-8, 8]) per cell."""
    ids = g.slot_ids()
    c, L = g.geometry(ids)
    recs = seeded_particles(ids, c, L, np.random.default_rng(seed), 3, K=4)
    p = g.add_variable_field("particles", np.float64, False)
    p.set([(recs[int(i)] * (1.0, 1.0, 1.0, 8.0)).reshape(-1) for i in ids])
    return p


def w_deposit(g, f, sp, st):
    g.particles_deposit(particles(g, 5), f[3], 4, 3, "cic", False)


def w_moments(g, f, sp, st):
    g.particles_deposit_moments(particles(g, 6), (f[1], f[2]), [(None, None), (3, None)], 4, -1, "cic")


def p_scaled_lengths(g, f, sp, st):
    for k in (4, 5, 6):
        f[k].set(f[k].get() * 1.25)


def w_fill_geometry(g, f, sp, st):
    assert source(g, f) == 0  # the scaled lengths are read
    g.fill_geometry(length=f[4:7])
    assert source(g, f) == 1  # right after the fill


def w_poisson(g, f, sp, st):
    """Five BiCG iterations of the Poisson solve on FB itself, the solution
    field being vz.  The right-hand side is poisson_cases.py's poisson3d one
    with that case's box (2 pi, pi, 8 pi) mapped onto FB's: the case's own mesh
    (n^3, periodic in z, refined about one point) is not FB, and a converged
    solve is not needed to write the field."""
    c, _ = g.geometry(g.slot_ids())
    box = np.array(l0_of(FB[0])) * FB[0]
    sp[0].set(-(81.0 / 16.0) * poisson3d_solution(c / box * (2 * np.pi, np.pi, 8 * np.pi)))
    dccrg_amd.Poisson_Solve(5, 5).solve(g.local_cells(), g, rhs=sp[0], solution=f[3])
    v = f[3].get(0, g.n_local)
    assert np.all(np.isfinite(v)) and np.any(v != 0)


def w_loopback(g, f, sp, st):
    dst = hump_run(g, f)
    src = 0 if dst >= 100 else g.n_local - 100
    assert src + 100 <= dst or dst + 100 <= src
    g.comm_loopback(f[2], src, 100, dst)


def p_edited(g, f, sp, st):
    f[1].set(f[1].get() * 2.0)
    f[5].set(f[5].get() * 1.25)


def w_initialize(g, f, sp, st):
    g.advection_initialize(f)


def p_pointers_out(g, f, sp, st):
    """vx and ly external: a structural change moves the arrays and clears it."""
    f[1].device_ptr()
    f[5].device_ptr()


def w_refine(g, f, sp, st):
    """The unrefined cell that holds the most density: its children take its
    payload, and its neighbors' fluxes across the four finer faces that replace
    one face move their densities (the guard, on the cells both meshes have)."""
    n = g.n_local
    ids = g.slot_ids()[:n]
    rho = np.where(g.mapping_batch(ids)["level"] < FB[1], f[0].get(0, n), -1.0)
    assert rho.max() > 0
    g.refine_completely(int(ids[np.argmax(rho)]))
    g.stop_refining()
    assert g.n_local > n


def w_adapt(g, f, sp, st):
    """The level R - 1 cell of the largest |vy|: advection_adapt resets its
    children's ly to half, which lowers the time step's bound (the guard)."""
    n = g.n_local
    ids = g.slot_ids()[:n]
    vy = np.where(g.mapping_batch(ids)["level"] == FB[1] - 1, np.abs(f[2].get(0, n)), -1.0)
    g.refine_completely(int(ids[np.argmax(vy)]))
    created, _ = g.advection_adapt(f)
    assert created > 0


def p_view(k):
    def p(g, f, sp, st):
        st["view"] = _torch_view(f[k], g.n_slots)  # fetches the pointer; the caches are warmed again after it
    return p


def w_view(k, refetch):
    def w(g, f, sp, st):
        import torch

        st.pop("view").mul_(4.0 if k < 4 else 0.25)
        torch.cuda.synchronize()
        if refetch:
            f[k].device_ptr()  # the header's advice
    return w


def w_view_then(k, then):
    """The write through the pointer, then a structural change: until it the
    consumers follow the write (the field is external: no cache is built or
    believed), after it the pointer is void and the caches are kept again."""
    def w(g, f, sp, st):
        dt = g.advection_max_time_step(f)
        w_view(k, False)(g, f, sp, st)
        if k < 4:
            assert g.advection_max_time_step(f) < dt
        else:
            assert source(g, f) == 0
        then(g, f, sp, st)
    return w


CASES = {
    "set": dict(writer=w_set_whole),
    "set_run": dict(writer=w_set_run),
    **{f"axpy_{NAMES[k]}": dict(writer=w_axpy(k)) for k in range(1, 7)},
    "gradient": dict(writer=w_gradient((0, 1, 2))),
    "gradient_x": dict(writer=w_gradient((0,))),
    "gradient_y": dict(writer=w_gradient((1,))),
    "gradient_z": dict(writer=w_gradient((2,))),
    "gradient_inner": dict(writer=w_gradient((0, 1, 2), "inner")),
    "curl": dict(writer=w_curl(False)),
    "curl_accumulate": dict(writer=w_curl(True)),
    "divergence": dict(writer=w_divergence(False)),
    "divergence_accumulate": dict(writer=w_divergence(True)),
    "deposit": dict(writer=w_deposit, hood=1),
    "deposit_moments": dict(writer=w_moments, hood=1),
    "fill_geometry": dict(writer=w_fill_geometry, prepare=p_scaled_lengths),
    "poisson": dict(writer=w_poisson),
    "loopback": dict(writer=w_loopback, rccl=True),
    "initialize": dict(writer=w_initialize, prepare=p_edited),
    "refine": dict(writer=w_refine, prepare=p_pointers_out, replay=True),
    "adapt": dict(writer=w_adapt, prepare=p_pointers_out, replay=True),
    "pointer_vy": dict(writer=w_view(2, False), prepare=p_view(2)),
    "pointer_vy_refetched": dict(writer=w_view(2, True), prepare=p_view(2)),
    "pointer_ly": dict(writer=w_view(5, False), prepare=p_view(5)),
    "pointer_ly_refetched": dict(writer=w_view(5, True), prepare=p_view(5)),
    "pointer_vy_then_refine": dict(writer=w_view_then(2, w_refine), prepare=p_view(2), replay=True),
    "pointer_ly_then_adapt": dict(writer=w_view_then(5, w_adapt), prepare=p_view(5), replay=True),
}


# The writes that cannot move the time step in this state (the guard holds by
# their densities): lx and lz grown (the bound is a minimum and ly / |vy| of a
# level-2 cell holds it), a few iterations' small Poisson solution as vz, and
# a plain refinement, whose children take their parent's lengths and velocities.
NOT_AGAINST_DT = ("axpy_lx", "axpy_lz", "poisson", "refine")


@pytest.mark.parametrize("records", [False, True], ids=["fields", "records"])
@pytest.mark.parametrize("case", list(CASES))
def test_consumers_follow_the_writer(gpu, case, records):
    r = check_after_write(records=records, **CASES[case])
    if case not in NOT_AGAINST_DT:
        assert r["dt_changed"]
    if not case.endswith("adapt"):
        assert r["rho_changed"]  # (adapt: the cell is chosen for dt, no density need be near it)
    if case == "fill_geometry":
        assert r["src"] == 1
    if case == "initialize":
        assert r["dt"] == r["dt0"] and r["src"] == 1
    if case.endswith("adapt"):
        assert r["src"] == 1  # the reset lengths are the geometry's and ly is external no longer
    if case in ("pointer_ly", "pointer_ly_refetched") or case in ("axpy_lx", "axpy_ly", "axpy_lz"):
        assert r["src"] == 0


@pytest.mark.parametrize("records", [False, True], ids=["fields", "records"])
def test_two_field_sets_with_equal_write_counts(gpu, records):
    """Two sets of seven advection fields on one grid, added together and each
    field written once, so that the write epochs of the two sets are equal:
    only the field ids (and arrays) tell them apart.  Set b has other
    velocities and one hand-edited ly.  The time step, the length check's
    verdict and two sweeps, asked of the sets in turn, are each set's cold
    twin's; the twins' answers differ, so a cache kept by epochs alone (set
    a's answer for set b) would have been caught."""
    with nbrec(records):
        g, f, _ = build()
        ids, cols_a = g.slot_ids(), download(g, f)
        n = g.n_local
        cols_b = cols_a.copy()
        cols_b[:, 1] *= 2.0
        cols_b[:, 2] *= -0.5
        cols_b[int(np.argmax(cols_a[:n, 0])), 5] *= 1.25  # the cell at the top of the hump
        sets = {}
        for name in ("a", "b"):
            sets[name] = [g.add_field(f"{name}_{x}", np.float64, x == "density") for x in NAMES]
        for name, cols in (("a", cols_a), ("b", cols_b)):
            for k in range(7):
                sets[name][k].set(cols[:, k])
        assert g.advection_layout()["tiles"] >= 2  # the first step already runs the tile kernels
        order = ("a", "b", "a", "b")
        dts = [(x, g.advection_max_time_step(sets[x])) for x in order]
        h = 0.25 * min(dt for _, dt in dts)
        srcs = [(x, source(g, sets[x])) for x in order]
        dens = {"a": [], "b": []}
        for x in order:
            dens[x] += sweep(g, sets[x], h, steps=1)
        dts += [(x, device_dt(g, sets[x])) for x in order]
        srcs += [(x, source(g, sets[x])) for x in order]
        g.close()
    twin = {"a": cold_run(build, ids, cols_a, h), "b": cold_run(build, ids, cols_b, h)}
    print(f"dt {dts} twins {twin['a'][0]!r} {twin['b'][0]!r} sources {srcs}")
    # set a's answers are not set b's: a stale cache would have been seen
    assert twin["a"][0] != twin["b"][0]
    assert all(not np.array_equal(x, y) for x, y in zip(twin["a"][1], twin["b"][1]))
    for x, dt in dts:
        assert dt == twin[x][0], ("time step of set", x, dt, twin[x][0])
    for x, src in srcs:
        assert src == (1 if x == "a" else 0), ("length source of set", x, srcs)
    for x in ("a", "b"):
        for k, (got, exp) in enumerate(zip(dens[x], twin[x][1])):
            assert np.array_equal(got, exp), ("densities of set", x, "differ from the twin's at step", k)


def test_loaded_file_governs(gpu, tmp_path):
    """save_grid_data with the seven fields transferred, vx scaled on the
    saving grid and its caches warmed again, then load_grid_data into a fresh
    grid (it is refused on an initialized one): the file's values govern the
    loaded grid's dt and sweeps - bitwise those of a cold twin made from the
    same file - and differ from the edited grid's."""
    path = tmp_path / "grid.dc"
    g, f, sp = build()
    dt0, h = warm(g, f, sp)
    for F in f:
        F.set_transfer(True)
    g.save_grid_data(path)
    saved = dict(zip(g.slot_ids().tolist(), download(g, f).tolist()))
    f[1].set(f[1].get() * 8.0)  # (enough for lx / |vx| of a level-2 cell to take the bound over)
    rewarm(g, f, h)
    dt_edited = g.advection_max_time_step(f)
    g.close()

    def load():
        t = dccrg_amd.Dccrg(0, 1, 0)
        tf = [t.add_field(n, np.float64, True) for n in NAMES]
        t.load_grid_data(path)
        return t, tf, None

    t, tf, _ = load()
    ids = t.slot_ids()
    cols = download(t, tf)
    assert np.array_equal(cols, np.array([saved[int(c)] for c in ids]))
    dt = t.advection_max_time_step(tf)
    dens = sweep(t, tf, h)
    src = source(t, tf)
    assert src == int(lengths_are_the_geometry(t, ids, cols)) == 1
    t.close()
    dt_t, dens_t = cold_run(load, ids, cols, h)
    assert dt == dt_t == AM.max_time_step(cols[: len(dens[0])]) == dt0
    for x, y in zip(dens, dens_t):
        assert np.array_equal(x, y)
    assert dt != dt_edited  # the edit after the save mattered


# ---- remote copies --------------------------------------------------------------
def view_run(on, records, exchange_all, writer, steps=4):
    """(16, 16, 8), R = 2 split into two z-slabs on detached views, all seven
    fields transferred; before step 2 view 0 writes (`writer`), and the halo
    of every step carries all seven fields (exchange_all) or the density
    alone."""
    from test_gpu_multirank import emulated_exchange

    base, R, P = (16, 16, 8), 2, 2
    with len_table(on), nbrec(records):
        ref, rf = gpu_grid(base, R)
        prerefine(ref, rf, R)
        h = 0.25 * ref.advection_max_time_step(rf)
        leaves = np.sort(ref.slot_ids()[: ref.n_local])
        l0p = np.array([ref.get_cell_from_indices(ref.get_indices(int(c)), 0) for c in leaves], np.int64)
        ref.close()
        owners = ((l0p - 1) * P // int(np.prod(base))).astype(np.int32)
        gs = []
        for r in range(P):
            g = dccrg_amd.Dccrg(r, P, 0).set_initial_length(base).set_neighborhood_length(0)
            g.set_maximum_refinement_level(R).set_periodic(True, True, False).initialize()
            g.set_geometry((0, 0, 0), l0_of(base))
            for n in NAMES:
                g.add_field(n, np.float64, exchange_all or n == "density")
            g.set_cells(leaves, owners)
            g.advection_initialize([g.fields[n] for n in NAMES])
            gs.append(g)
        out = []
        for k in range(steps):
            if k == 2:
                writer(gs[0], [gs[0].fields[n] for n in NAMES])
            emulated_exchange(gs, list(NAMES) if exchange_all else ["density"])
            for g in gs:
                f = [g.fields[n] for n in NAMES]
                g.advection_step(f, h, "inner")
                g.advection_step(f, h, "outer")
                g.advection_commit(f[0])
            out.append([g.fields["density"].get(0, g.n_local) for g in gs])
        assert all(g.counts["outer"] > 0 and g.counts["inner"] > 0 for g in gs)
        assert all(g.advection_layout()["tiles"] >= 2 for g in gs)
        for g in gs:
            g.close()
    return out


def vw_axpy(g, f):
    """vx, vz and lx.  The views are z-slabs, so a remote copy is read across
    a z-face alone: its flux is the face's vz times the smaller of the two
    cells' lx ly, and vz is zero in the initial state - vx and lx alone could
    not reach the other view's densities, with vz they do (lx shrinks, so the
    smaller area is the written cell's)."""
    g.field_axpy(f[1], 0.5, f[2])
    g.field_axpy(f[3], 0.5, f[2])
    g.field_axpy(f[4], -0.25, f[5])


def vw_regions(g, f):
    """The operators by region, the inner run and the outer run in a call
    each: the x-derivative of the density into vx, its divergence-like sum of
    derivatives into vz (nonzero on the hump, see vw_axpy)."""
    for region in ("inner", "outer"):
        g.gradient(f[0], (f[1], None, None), 0.25, region)
        g.divergence((f[0], f[0], f[0]), f[3], 0.25, False, region)


@pytest.mark.parametrize("writer", [vw_axpy, vw_regions], ids=["axpy", "regions"])
def test_remote_copies_follow_the_writer(gpu, writer):
    """A write on one view reaches the other view's sweeps through the halo
    (field_halo_written): with the table, and with the records, the densities
    of both views are bitwise those of the run that reads the fields; without
    the exchange of the written fields they differ."""
    base = view_run(False, False, True, writer)
    for on, records in ((True, False), (True, True)):
        got = view_run(on, records, True, writer)
        for k, (a, b) in enumerate(zip(got, base)):
            for r in range(2):
                assert np.array_equal(a[r], b[r]), (on, records, "step", k, "view", r)
    stale = view_run(False, False, False, writer)
    assert all(np.array_equal(a, b) for k in (0, 1) for a, b in zip(stale[k], base[k]))
    assert not np.array_equal(stale[3][1], base[3][1])  # view 1 saw view 0's write only through the halo


def sc_write_tracking(rank, world):
    """Two real processes, all seven fields transferred, vx, vz and lx changed
    on process 0 alone before the halo of step 2 starts, so that on the other
    process the records' and the length table's keys can move through the
    halo's epoch bumps only (plan_start, halo_wait).  The overlapped order
    (start, inner sweep, wait, outer sweep), with and without the records,
    gives each process bitwise the densities of the blocking order (run with
    DCCRGX_LEN_TABLE=0 and no records, so it keeps nothing that could be stale); those
    differ from a run without the change, and on the receiving process from a
    run whose halo carries the density alone (the remote copies of the changed
    fields are read there)."""
    from test_gpu_transport import _gather, _grid, _prerefine

    base, R = (16, 16, 8), 2
    runs, outer = {}, 0
    for mode, overlap, records, edit in (("blocking", False, False, True), ("overlap", True, False, True),
                                         ("overlap_records", True, True, True), ("unedited", False, False, False),
                                         ("density_only", False, False, True)):
        # the blocking runs read the fields (no table, no records): a stale table cannot hide in the reference
        with nbrec(records), len_table(overlap):
            g = _grid(base, R, (True, True, False), 0)
            g.set_geometry((0, 0, 0), l0_of(base))
            f = [g.add_field(n, np.float64, mode != "density_only" or n == "density") for n in NAMES]
            _prerefine(g, f, R)
            h = 0.25 * g.advection_max_time_step(f)
            dens = []
            for k in range(4):
                if k == 2 and edit and rank == 0:
                    # the sender alone: on the other process these fields' epochs move through the halo only
                    g.field_axpy(f[1], 0.5, f[2])
                    g.field_axpy(f[3], 0.5, f[2])  # (a remote copy's vz is what a z-face between processes reads)
                    g.field_axpy(f[4], -0.25, f[5])  # (and the smaller lx ly of the two cells is the face's area)
                if overlap:
                    g.start_remote_neighbor_copy_updates()
                    g.advection_step(f, h, "inner")
                    g.wait_remote_neighbor_copy_update_receives()
                    g.advection_step(f, h, "outer")
                    g.wait_remote_neighbor_copy_update_sends()
                else:
                    g.update_copies_of_remote_neighbors()
                    g.advection_step(f, h, "inner")
                    g.advection_step(f, h, "outer")
                g.advection_commit(f[0])
                dens.append(f[0].get(0, g.n_local))
            runs[mode] = dens
            outer = g.counts["outer"]
            g.close()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(runs[a], runs[b]))

    return dict(outer=outer > 0, overlap=same("blocking", "overlap"), records=same("blocking", "overlap_records"),
                mattered=any(_gather(not same("blocking", "unedited"))),
                halo_mattered=all(_gather(not same("blocking", "density_only"))[1:]))


def test_writes_before_a_halo_in_flight(gpu, tmp_path):
    from test_gpu_transport import _run_group

    results = _run_group(2, tmp_path, names=["sc_write_tracking"], module="test_gpu_field_write_tracking")
    assert "sc_write_tracking" in results and len(results["sc_write_tracking"]) == 2
    for rank, (kind, out) in sorted(results["sc_write_tracking"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"


# ---- the bands ------------------------------------------------------------------
BAND_STEPS, BAND_EDITS = 12, (3, 7)


def band_run(base, split, cache, writer, edits, stop=None):
    """test_gpu_advection_adapt.py's adaptive run; at the steps `edits` the
    density is written between advection_step and advection_check_adaptation.
    Returns per step the check's counts, adapt's counts, the leaves and the
    densities; `stop`: the run ends with that step's check."""
    from test_gpu_advection import gpu_grid as grid1, prerefine as prerefine1

    R = 2
    old = os.environ.pop("DCCRGX_BAND_CACHE", None)
    if not cache:
        os.environ["DCCRGX_BAND_CACHE"] = "0"
    try:
        g, f = grid1(base, R)
        spare = g.add_field("spare", np.float64, False)
        prerefine1(g, f, R)
        di = 0.025 / R
        out = []
        for step in range(BAND_STEPS):
            dt = 0.5 * g.advection_max_time_step(f)
            view = None
            if writer == "pointer" and step in edits and step == BAND_EDITS[1]:
                view = _torch_view(f[0], g.n_slots)  # the pointer is out during the sweep
            if split:
                g.advection_step(f, dt, "inner")
                g.advection_step(f, dt, "outer")
            else:
                g.advection_step(f, dt)
            if step in edits:
                band_write(g, f, spare, writer, view)
            counts = g.advection_check_adaptation(f[0], di)
            if step == stop:
                out.append((counts,))
                break
            g.advection_commit(f[0])
            adapted = g.advection_adapt(f)
            out.append((counts, adapted, g.local_cells(), f[0].get(0, g.n_local)))
        g.close()
    finally:
        os.environ.pop("DCCRGX_BAND_CACHE", None)
        if old is not None:
            os.environ["DCCRGX_BAND_CACHE"] = old
    return out


def band_write(g, f, spare, writer, view):
    """rho += 0.5 x a hump of the initial one's height a few cells aside (by
    `writer`): steep enough to move cells across the band thresholds."""
    import torch

    n = g.n_slots
    c, _ = g.geometry(g.slot_ids())
    r = np.minimum(np.sqrt((c[:, 0] - 0.55) ** 2 + (c[:, 1] - 0.35) ** 2), 0.15) / 0.15
    bump = 0.25 * (1 + np.cos(np.pi * r))
    rho = f[0].get()
    if writer == "set":
        f[0].set(rho + 0.5 * bump)
    elif writer == "axpy":
        spare.set(bump)
        g.field_axpy(f[0], 0.5, spare)
    elif writer == "divergence":
        # the sum of the three derivatives of x * bump: bump + x (d/dx + d/dy) bump, a steeper write than the others
        spare.set(c[:, 0] * bump)
        g.divergence((spare, spare, spare), f[0], 0.5, True)
    elif writer == "deposit":
        p = g.fields.get("particles") or g.add_variable_field("particles", np.float64, False)
        recs = np.concatenate([c, (rho + 0.5 * bump)[:, None]], axis=1)  # one record at each cell's center
        p.set([recs[i] for i in range(n)])
        g.particles_deposit(p, f[0], 4, 3, "ngp", False)
    elif writer == "pointer":
        v = view if view is not None else _torch_view(f[0], n)
        v.add_(torch.as_tensor(0.5 * bump, device="cuda"))
        torch.cuda.synchronize()
    else:
        raise ValueError(writer)


@pytest.mark.parametrize("writer", ["set", "axpy", "divergence", "deposit", "pointer"])
@pytest.mark.parametrize("base,split", [((16, 16, 1), True), ((10, 10, 3), False)])
def test_bands_follow_density_writes(gpu, base, split, writer):
    """The sweep's bands stand for the check's own only while the density is
    as the sweep saw it.  Two runs, the second with DCCRGX_BAND_CACHE=0, the
    density written between the sweep and the check at two steps: counts,
    leaves and densities equal at every step.  At the edited steps the check's
    counts differ from those of a run that is the same up to that step but
    does not write there: stale bands would have been caught."""
    a = band_run(base, split, True, writer, BAND_EDITS)
    b = band_run(base, split, False, writer, BAND_EDITS)
    assert len(a) == len(b) == BAND_STEPS
    for step, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0] and x[1] == y[1], (step, x[:2], y[:2])
        assert np.array_equal(x[2], y[2]), step
        assert np.array_equal(x[3], y[3]), step
    for i, e in enumerate(BAND_EDITS):
        u = band_run(base, split, True, writer, BAND_EDITS[:i], stop=e)
        print(f"step {e}: counts with the write {a[e][0]}, without {u[e][0]}")
        assert all(u[k][:2] == a[k][:2] for k in range(e))  # the same run up to the step
        assert u[e][0] != a[e][0]


# ---- the length table's back-off ---------------------------------------------------
def test_length_check_backs_off_and_resumes(gpu):
    """ly rewritten before three consecutive steps (its own values, then
    scaled twice): ensure_len_table stops checking at the second changed key
    in a row and the sweeps read the fields; the geometry's values back and two
    steps without a write, the table is in use again.  Bitwise the forced-off
    run throughout."""
    def edit(g, f, k):
        if k == 2:
            edit.ly = f[5].get()
            f[5].set(edit.ly)
        elif k == 3:
            f[5].set(edit.ly * 1.25)
        elif k == 4:
            f[5].set(edit.ly * 1.5)
        elif k == 5:
            f[5].set(edit.ly)
        return g.advection_length_source(f) if k in (1, 7) else None

    a, src, _, seen = length_run(*FB, 8, True, edit=edit)
    b, src_b, _, _ = length_run(*FB, 8, False, edit=edit)
    c, _, _, _ = length_run(*FB, 8, True)
    assert seen[1] == 1 and seen[7] == 1 and src == 1 and src_b == 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(a[2], c[2]) and not np.array_equal(a[4], c[4])  # the scaled lengths mattered
