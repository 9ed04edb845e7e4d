"""Tile sweeps that take a uniform velocity component from a kernel argument
(ensure_vel_uniform, dccrgx_advection_velocity_source) against the same
sweeps reading the three velocity fields (DCCRGX_VEL_UNIFORM=0).

A component whose every slot holds one 64-bit pattern reaches the flux
expressions as the same bits from another place, so every comparison here is
bitwise (np.array_equal), never a tolerance.  Uniform components get 0.3,
-0.7, 0.45 - no powers of two, distinct, one negative, so a swapped axis or a
sign error changes bits; the others a smooth function of the cell centers
(a non-zero, varying vz included)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import dccrg_amd
from test_gpu_advection_lds import MESHES
from test_gpu_advection_lengths import FB, NAMES, gpu_grid, l0_of, len_table, prerefine
import test_gpu_field_write_tracking as WT

pytestmark = pytest.mark.gpu

STEPS = 4
UNIFORM = (0.3, -0.7, 0.45)


@contextlib.contextmanager
def vel_uniform(on):
    old = os.environ.pop("DCCRGX_VEL_UNIFORM", None)
    if not on:
        os.environ["DCCRGX_VEL_UNIFORM"] = "0"
    try:
        yield
    finally:
        os.environ.pop("DCCRGX_VEL_UNIFORM", None)
        if old is not None:
            os.environ["DCCRGX_VEL_UNIFORM"] = old


def set_velocities(g, f, mask):
    """Components of `mask` uniform, the others smooth in the cell centers."""
    c, _ = g.geometry(g.slot_ids())
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    tau = 2 * np.pi
    smooth = (0.4 + 0.3 * np.sin(tau * y) + 0.1 * z,
              -0.2 + 0.3 * np.cos(tau * x) - 0.15 * z,
              0.25 + 0.2 * np.sin(tau * x) * np.cos(tau * y) + 0.1 * z)
    for a in range(3):
        f[1 + a].set(np.full(x.size, UNIFORM[a]) if (mask >> a) & 1 else smooth[a])


MESH = dict(MESHES)
MESH["all_regular"] = ((16, 16, 16), 1, lambda g, f: g.advection_initialize(f))
MESH["fb"] = (FB[0], FB[1], lambda g, f: prerefine(g, f, FB[1]))


def run(name, mask, on, steps=STEPS, edit=None, external=()):
    """`steps` sweeps of mesh `name` (the face table at the first, the tiles
    from the second on) with the components of `mask` set uniform (None: the
    fields as advection_initialize leaves them); `edit(g, f, k)` runs before
    step k, its return value is recorded.  The velocity source is asked after
    every step."""
    base, R, make = MESH[name]
    with vel_uniform(on):
        g, f = gpu_grid(base, R)
        make(g, f)
        if mask is not None:
            set_velocities(g, f, mask)
        for k in external:
            f[k].device_ptr()
        dt = g.advection_max_time_step(f)
        out, src, seen = [], [], []
        for k in range(steps):
            if edit is not None:
                seen.append(edit(g, f, k))
            g.advection_step(f, 0.5 * dt)
            g.advection_commit(f[0])
            out.append(f[0].get(0, g.n_local))
            src.append(g.advection_velocity_source(f))
        res = dict(out=out, src=src, seen=seen, lay=g.advection_layout(), len_src=g.advection_length_source(f))
        g.close()
    return res


@functools.lru_cache(maxsize=None)
def pair(name, mask):
    """The run with the verdict and the forced-off run, computed once."""
    a, b = run(name, mask, True), run(name, mask, False)
    assert a["len_src"] == 1 and b["len_src"] == 1
    assert all(s == 0 for s in b["src"]), b["src"]
    return a, b


def assert_bitwise(a, b):
    assert len(a["out"]) == len(b["out"])
    for k, (x, y) in enumerate(zip(a["out"], b["out"])):
        assert np.array_equal(x, y), ("densities differ from the forced-off run's at step", k)
    assert not np.array_equal(a["out"][0], a["out"][-1])  # the sweeps moved something


@pytest.mark.parametrize("mask", range(8))
def test_all_masks_bitwise_equal_the_fields(gpu, mask):
    a, b = pair("prerefined", mask)
    lay = a["lay"]
    assert lay["regular_tiles"] > 0 and lay["tiles"] - lay["regular_tiles"] > 0 and lay["finer_faces"] > 0, lay
    assert a["src"][-1] == mask, a["src"]
    assert_bitwise(a, b)
    # the bench line's byte count follows the mask; SURVEY's counts do not
    if mask:
        assert lay["bytes_needed"] < b["lay"]["bytes_needed"]
    else:
        assert lay["bytes_needed"] == b["lay"]["bytes_needed"]
    assert lay["alg_bytes"] == b["lay"]["alg_bytes"] and lay["alg_bytes_core"] == b["lay"]["alg_bytes_core"]


def test_bytes_needed_counts_every_uniform_component(gpu):
    """8 B per own cell and component at the least, and more for each further
    component (its out-of-tile neighbors)."""
    need = [pair("prerefined", m)[0]["lay"]["bytes_needed"] for m in range(8)]
    off = pair("prerefined", 7)[1]["lay"]
    n = off["alg_bytes_core"] // 64  # local cells
    assert need[0] == off["bytes_needed"]
    for m in range(1, 8):
        for a in range(3):
            if (m >> a) & 1:
                assert need[m] + 8 * n <= need[m & ~(1 << a)], (m, a, need)


@pytest.mark.parametrize("name", ["all_regular", "nested", "ext640"])
@pytest.mark.parametrize("mask", [0, 4, 7])
def test_masks_on_other_meshes(gpu, name, mask):
    a, b = pair(name, mask)
    lay = a["lay"]
    if name == "all_regular":
        assert lay["tiles"] == lay["regular_tiles"] > 0, lay
    elif name == "nested":
        assert lay["tiles"] - lay["regular_tiles"] >= 1 and lay["finer_faces"] > 0, lay
    else:
        assert lay["ext_max"] == 640, lay
    assert a["src"][-1] == mask, a["src"]
    assert_bitwise(a, b)


def test_vz_as_initialize_leaves_it(gpu):
    """vz = +0.0 everywhere with no set call: the bench's case at small size."""
    a, b = run("prerefined", None, True), run("prerefined", None, False)
    assert a["src"][-1] == 4 and all(s == 0 for s in b["src"])
    assert_bitwise(a, b)
    assert a["lay"]["bytes_needed"] < b["lay"]["bytes_needed"]


# ---- verdict edges -------------------------------------------------------------
# (the source is asked right after an edit, before the sweep: the sweep then
# finds the key it was asked with, so the edits below never look like a field
# rewritten before every sweep)
def hump_top(g, f):
    return int(np.argmax(f[0].get(0, g.n_local)))


def edges(edit, steps=6, mask=4, external=()):
    a = run("fb", mask, True, steps, edit, external)
    b = run("fb", mask, False, steps, edit, external)
    c = run("fb", mask, True, steps)
    for k, (x, y) in enumerate(zip(a["out"], b["out"])):
        assert np.array_equal(x, y), k
    return a, b, c


def test_one_changed_slot_clears_the_bit_and_returns(gpu):
    def edit(g, f, k):
        if k == 2:
            v = f[3].get()
            edit.old = v.copy()
            v[hump_top(g, f)] = 0.6
            f[3].set(v)
            return g.advection_velocity_source(f)
        if k == 4:
            f[3].set(edit.old)
            return g.advection_velocity_source(f)

    a, b, c = edges(edit)
    assert a["src"] == [4, 4, 0, 0, 4, 4] and a["seen"][2] == 0 and a["seen"][4] == 4, (a["src"], a["seen"])
    assert not np.array_equal(a["out"][3], c["out"][3])  # the edit mattered


def test_negative_zero_is_not_uniform(gpu):
    def edit(g, f, k):
        if k == 2:
            v = f[3].get()
            assert not np.signbit(v).any() and not v.any()
            v[hump_top(g, f)] = -0.0
            f[3].set(v)
            return g.advection_velocity_source(f)

    a = run("fb", None, True, 4, edit)
    b = run("fb", None, False, 4, edit)
    assert a["src"] == [4, 4, 0, 0] and a["seen"][2] == 0, a["src"]
    for x, y in zip(a["out"], b["out"]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("k_field", [1, 2, 3])
def test_external_velocity_field_reads_the_fields(gpu, k_field):
    a, b, _ = edges(None, steps=3, mask=7, external=(k_field,))
    assert a["src"] == [0, 0, 0], a["src"]


def test_length_fields_read_means_mask_zero(gpu):
    with len_table(False):
        a = run("fb", 7, True, 3)
    b = run("fb", 7, False, 3)
    assert a["src"] == [0, 0, 0] and a["len_src"] == 0
    for x, y in zip(a["out"], b["out"]):
        assert np.array_equal(x, y)


def test_rewritten_before_every_sweep_backs_off(gpu):
    """The same values set again before each of three sweeps in a row: the
    key is found changed at the second, so no pass is made and the fields are
    read; the mask returns at the first sweep that finds them unwritten."""
    def edit(g, f, k):
        if k in (1, 2, 3):
            f[3].set(f[3].get())

    a, b, _ = edges(edit, steps=6, mask=6)
    # step 0 sweeps the face table (the verdict asked after it is a query's)
    assert a["src"] == [6, 6, 0, 0, 6, 6], a["src"]


def test_remote_copy_slot_clears_the_bit_on_its_view(gpu):
    """Two z-slabs on detached views (test_gpu_advection_lengths.py's slabs):
    one remote copy of vz changed on view 0 clears bit 2 there alone."""
    from test_gpu_multirank import emulated_exchange

    base, R, P = (16, 16, 8), 2, 2

    def views(on, edited):
        with vel_uniform(on):
            ref, rf = gpu_grid(base, R)
            prerefine(ref, rf, R)
            dt = ref.advection_max_time_step(rf)
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
                    g.add_field(n, np.float64, n == "density")
                g.set_cells(leaves, owners)
                g.advection_initialize([g.fields[n] for n in NAMES])
                gs.append(g)
            src = []
            for k in range(STEPS):
                emulated_exchange(gs, ["density"])
                if edited and k == 2:
                    g = gs[0]
                    rho = g.fields["density"].get()
                    assert rho.size > g.n_local
                    j = g.n_local + int(np.argmax(rho[g.n_local:]))
                    g.fields["vz"].set(np.array([0.6]), j)
                for g in gs:
                    f = [g.fields[n] for n in NAMES]
                    g.advection_step(f, 0.5 * dt, "inner")
                    g.advection_step(f, 0.5 * dt, "outer")
                    g.advection_commit(f[0])
                src.append([g.advection_velocity_source([g.fields[n] for n in NAMES]) for g in gs])
            out = [g.fields["density"].get(0, g.n_local) for g in gs]
            outer = [g.counts["outer"] for g in gs]
            for g in gs:
                g.close()
        return out, src, outer

    a, src, outer = views(True, True)
    b, src_b, _ = views(False, True)
    c, src_c, _ = views(True, False)
    assert all(n > 0 for n in outer)
    assert src[1] == [4, 4] and src[2] == [0, 4] and src[3] == [0, 4], src
    assert all(s == [0, 0] for s in src_b) and src_c[-1] == [4, 4]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])  # the remote copy's velocity reached a density


# ---- advection_adapt -------------------------------------------------------------
def adapt_run(on, requests, steps=6):
    base, R = (16, 16, 4), 2
    with vel_uniform(on):
        g, f = gpu_grid(base, R)
        prerefine(g, f, R)
        dt = g.advection_max_time_step(f)
        out, src, cells = [], [], []
        for _ in range(steps):
            g.advection_step(f, 0.5 * dt)
            if requests:
                g.advection_check_adaptation(f[0], 0.025 / R)
            g.advection_commit(f[0])
            # after the sweep, before the velocities are reset again
            src.append(g.advection_velocity_source(f) if not requests else None)
            g.advection_adapt(f)
            cells.append(g.local_cells().copy())
            out.append(f[0].get(0, g.n_local))
        g.advection_step(f, 0.5 * dt)
        g.advection_commit(f[0])
        g.advection_step(f, 0.5 * dt)  # a sweep that finds the velocities unwritten
        g.advection_commit(f[0])
        out.append(f[0].get(0, g.n_local))
        src.append(g.advection_velocity_source(f))
        g.close()
    return out, src, cells


@pytest.mark.parametrize("requests", [True, False])
def test_advection_adapt_bitwise(gpu, requests):
    """advection_adapt resets the velocities before every sweep.  With the
    check's requests the mesh follows the hump; without them the mesh stays,
    every sweep after the first runs the tile kernels and finds the key
    changed: the source is 0 from the second tile sweep on - a check pass
    would say 4, vz being zero - until a sweep finds the fields unwritten."""
    a, src, cells = adapt_run(True, requests)
    b, src_b, cells_b = adapt_run(False, requests)
    for x, y in zip(cells, cells_b):
        assert np.array_equal(x, y)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), k
    assert src[-1] == 4 and src_b[-1] == 0
    if not requests:
        # asked after sweep k: sweep 0 is the face table's (a query's pass),
        # sweep 1 the first of the tiles (one changed key so far), then the
        # back-off
        assert src[:2] == [4, 4] and all(s == 0 for s in src[2:-1]), src


# ---- write tracking -------------------------------------------------------------
def p_uniform(g, f, sp, st):
    for a in range(3):
        f[1 + a].set(np.full(g.slot_ids().size, UNIFORM[a]))


def after_uniform(w, expect):
    """Writer w on a grid whose verdict is mask 7; the mask it must leave."""
    def ww(g, f, sp, st):
        assert g.advection_velocity_source(f) == 7
        w(g, f, sp, st)
        assert g.advection_velocity_source(f) == expect
    return ww


WRITERS = [
    ("set_run", WT.w_set_run, 6),
    ("set_whole", lambda g, f, sp, st: f[2].set(f[2].get() + np.linspace(0.0, 0.5, g.slot_ids().size)), 5),
    ("axpy_vx", WT.w_axpy(1), 6),
    ("axpy_vz", WT.w_axpy(3), 3),
    ("gradient", WT.w_gradient((0, 1, 2)), 0),
    ("curl", WT.w_curl(False), 0),
    ("divergence", WT.w_divergence(False), 6),
    ("deposit", WT.w_deposit, 3),
    ("moments", WT.w_moments, 4),
    ("initialize", WT.w_initialize, 4),
]


@pytest.mark.parametrize("name,writer,expect", WRITERS, ids=[w[0] for w in WRITERS])
def test_tracked_writer_of_a_uniform_velocity(gpu, name, writer, expect):
    hood = 1 if name in ("deposit", "moments") else 0
    WT.check_after_write(after_uniform(writer, expect), False, prepare=p_uniform, hood=hood)
