"""Charge deposition and field gather on the device
(dccrgx_particles_deposit / dccrgx_particles_gather, dccrg_amd/csrc/particles.hip)
against the model of tests/deposit_model.py.

Both sides form bitwise equal terms q W and W F (one IEEE operation per step,
in the header's order); only the order of a sum is the kernel's.  The model
sums with math.fsum, so with m terms the device may differ from it by
  deposit: (m + 2) 2^-52 sum|term| / V     (V = 1 without per_volume)
  gather:  (j + 2) 2^-52 sum_c |W F_c|     (j candidates with W > 0)
(m - 1 additions of at most half a unit of the running sum each, the model's
own half unit, the division).  Exact zeros add nothing, so m and j count the
non-zero terms.  A miss is a bug, not noise."""
import math
import types

import numpy as np
import pytest

from deposit_model import DepositModel
from helpers import make_pair
from particles_model import ParticleModel, seeded_particles
from test_gpu_particles import REF_L0, REF_START, REFINED, _assert_model, _local_cells, _same

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SHAPES = {"ngp": 0, "cic": 1}
ODD_START, ODD_L0 = (0.1, -0.3, 0.2), (0.3, 0.7, 1.1)


def _pair(length, R=0, periodic=(True, True, True), hood=1, rounds=0, frac=0.1, start=(0, 0, 0), l0=(1, 1, 1), K=4,
          nprocs=1):
    g, o = make_pair(length, R, periodic, hood, rounds, frac, nprocs=nprocs)
    g.set_geometry(start, l0)
    m = ParticleModel(o, start, l0, K)
    fld = g.add_variable_field("particles", np.float64, True)
    return g, m, fld


def _seed(m, rng, max_per_cell):
    ctr, ln = m.o.geometry(m.leaves)
    for c, r in seeded_particles(m.leaves, ctr, ln, rng, max_per_cell, m.K).items():
        m.set(c, r)


def _upload_all(g, fld, m):
    """Every slot's records: the local cells' and the remote copies'."""
    fld.set([m.cells[int(c)].reshape(-1) for c in g.slot_ids()])


def _cell_field(g, name, values):
    """A float64 field holding values[cell] in every slot."""
    f = g.add_field(name, np.float64)
    f.set(np.array([values[int(c)] for c in g.slot_ids()], np.float64))
    return f


def _share_tol(m):
    """|sum_c W - 1| of the exact shares on a periodic grid (the CPU model test holds the model to it)."""
    return 64 * EPS * max(np.max(np.abs(m.start)), np.max(np.abs(m.end))) / np.min(m.cell_len)


def _check_deposit(g, fld, dm, out, shape, weight, exp=None, volumes=None):
    """Both per_volume settings against the model; returns (model, device sums)."""
    K = dm.pm.K
    exp = exp or dm.deposit(SHAPES[shape], weight)
    local = [int(c) for c in g.slot_ids()[: g.n_local]]
    got = None
    for pv in (True, False):
        g.particles_deposit(fld, out, K, weight, shape, per_volume=pv)
        got = out.get(0, g.n_local)
        worst = 0.0
        for c, v in zip(local, got):
            total, mag, cnt, _ = exp[c]
            V = np.float64(1)
            if pv:
                V = np.float64(volumes[c]) if volumes is not None else dm.volume(c)
                total = total / V
            bound = (cnt + 2) * EPS * mag / V
            worst = max(worst, abs(v - total) / bound if bound else abs(v - total))
            assert abs(v - total) <= bound, (shape, pv, c, v, total, bound)
        print(f"deposit {shape} per_volume={pv}: worst error {worst:.3f} of its bound")
    return exp, dict(zip(local, got))


def _check_gather(g, fld, dm, fields, values, first, shape, exact=False):
    """The gathered doubles against the model; everything else bitwise as before."""
    K = dm.pm.K
    nf = len(fields)
    before = _local_cells(g, fld, K)
    nr = g.n_slots - g.n_local
    remote = fld.get(g.n_local, nr) if nr else []
    g.particles_gather(fld, fields, first, K, shape)
    after = _local_cells(g, fld, K)
    exp = dm.gather(values, SHAPES[shape])
    keep = [k for k in range(K) if not first <= k < first + nf]
    worst = 0.0
    for c, a in after.items():
        val, mag, cnt = exp[c]
        assert a.shape == before[c].shape
        assert _same(np.ascontiguousarray(a[:, keep]), np.ascontiguousarray(before[c][:, keep])), c
        got = a[:, first:first + nf]
        if exact:
            assert _same(np.ascontiguousarray(got), val), (c, got, val)
            continue
        bound = (cnt[:, None] + 2) * EPS * mag
        assert np.all(np.abs(got - val) <= bound), (shape, c, got, val, bound)
        if got.size:
            worst = max(worst, float(np.max(np.abs(got - val) / np.where(bound > 0, bound, 1))))
    print(f"gather {shape}: worst error {worst:.3f} of its bound")
    for x, y in zip(remote, fld.get(g.n_local, nr) if nr else []):
        assert _same(x, y)  # records of remote copies are not written
    return exp, after


def _random_fields(g, m, rng, n, scale=None):
    vals = [{int(c): float(rng.random() * 2 - 1) for c in m.leaves} for _ in range(n)]
    if scale:
        vals = [{c: round(v * scale) / scale for c, v in F.items()} for F in vals]
    return [_cell_field(g, f"F{j}", F) for j, F in enumerate(vals)], vals


# ---- exact -----------------------------------------------------------------------
def test_exact_case_is_bitwise(gpu):
    """l0 = 1, start = 0, positions on eighths of the finest cell, q and F on
    2^-10: every product and sum is exact in any order."""
    g, m, fld = _pair(**REFINED)
    _seed(m, np.random.default_rng(41), 5)
    for rec in m.cells.values():
        rec[:, 0:3] = np.round(rec[:, 0:3] * 32) / 32
        rec[:, 3] = np.round(rec[:, 3] * 1024) / 1024
    _upload_all(g, fld, m)
    dm = DepositModel(m)
    out = g.add_field("rho", np.float64)
    for shape in ("cic", "ngp"):
        exp = dm.deposit(SHAPES[shape], 3)
        for pv in (False, True):
            g.particles_deposit(fld, out, 4, 3, shape, per_volume=pv)
            want = np.array([exp[int(c)][0] / (dm.volume(int(c)) if pv else 1.0) for c in g.slot_ids()[: g.n_local]])
            assert _same(out.get(0, g.n_local), want), (shape, pv)
    g.particles_deposit(fld, out, 4, None, "cic")
    cnt = dm.deposit(1, None)
    assert _same(out.get(0, g.n_local), np.array([cnt[int(c)][0] for c in g.slot_ids()[: g.n_local]]))
    assert math.fsum(out.get(0, g.n_local)) <= m.total()  # the open z faces drop shares
    fields, vals = _random_fields(g, m, np.random.default_rng(42), 1, scale=1024)
    _check_gather(g, fld, dm, fields, vals, 3, "cic", exact=True)
    g.close()


# ---- tiny periodic grid ------------------------------------------------------------
def test_tiny_periodic_grid(gpu):
    """3 x 1 x 1 fully periodic (tests/particles/simple.cpp): every row lists
    the cell itself and its two neighbors many times over, and y and z are one
    cell wide, so a cloud overlaps its own cell's images."""
    g, m, fld = _pair((3, 1, 1), start=ODD_START, l0=ODD_L0)
    rng = np.random.default_rng(43)
    _seed(m, rng, 4)
    m.set(2, np.concatenate([m.cells[2], [[0.1 + 0.3 + 0.01, -0.3 + 0.69, 0.2 + 0.02, 0.75]]]))  # near three faces
    _upload_all(g, fld, m)
    dm = DepositModel(m)
    out = g.add_field("rho", np.float64)
    exp, got = _check_deposit(g, fld, dm, out, "cic", 3)
    _check_deposit(g, fld, dm, out, "ngp", 3)
    q = np.concatenate([r[:, 3] for r in m.cells.values()])
    slack = sum((v[2] + 2) * EPS * v[1] for v in exp.values()) + (_share_tol(m) + 2 * EPS) * math.fsum(np.abs(q))
    assert abs(math.fsum(got.values()) - math.fsum(q)) <= slack  # nothing leaves a periodic grid
    fields, vals = _random_fields(g, m, rng, 2)
    fields.append(_cell_field(g, "one", {int(c): 1.0 for c in m.leaves}))
    vals.append({int(c): 1.0 for c in m.leaves})
    with pytest.raises(Exception, match="first_double"):
        g.particles_gather(fld, fields, 3, 4, "cic")  # three fields do not fit into K = 4
    _check_gather(g, fld, dm, fields[:1], vals[:1], 3, "cic")
    _check_gather(g, fld, dm, fields[2:], vals[2:], 3, "cic")
    ones = np.concatenate([a[:, 3] for a in _local_cells(g, fld, 4).values()])
    assert np.all(np.abs(ones - 1.0) <= _share_tol(m) + 29 * EPS)  # the whole cloud is inside, 27 terms
    g.close()


# ---- refined grid ------------------------------------------------------------------
def _refined_case(K, start, l0, seed):
    g, m, fld = _pair(start=start, l0=l0, K=K, **REFINED)
    rng = np.random.default_rng(seed)
    _seed(m, rng, 5)
    _upload_all(g, fld, m)
    return g, m, fld, rng


def _deposit_and_gather(g, m, fld, rng, out, fields, vals):
    dm = DepositModel(m)
    K = m.K
    weights = [3, 6, None] if K >= 7 else [3]
    for weight, exp in zip(weights, dm.deposit_many(1, weights)):
        _check_deposit(g, fld, dm, out, "cic", weight, exp)
    _check_deposit(g, fld, dm, out, "ngp", 3)
    if K >= 7:
        first, nf = 4, 3
    else:
        first, nf = 3, 1
    _, after = _check_gather(g, fld, dm, fields[:nf], vals[:nf], first, "cic")
    _check_gather(g, fld, dm, fields[:nf], vals[:nf], first, "ngp")
    for c, a in _local_cells(g, fld, K).items():  # ngp: the cell's own values
        assert np.all(a[:, first:first + nf] == np.array([F[c] for F in vals[:nf]]))
    for c, a in _local_cells(g, fld, K).items():
        m.set(c, a)  # the model follows the device's gathered doubles


@pytest.mark.parametrize("K", [4, 7])
def test_refined_grid(gpu, K):
    g, m, fld, rng = _refined_case(K, REF_START, REF_L0, 44 + K)
    out = g.add_field("rho", np.float64)
    fields, vals = _random_fields(g, m, rng, 3)
    _deposit_and_gather(g, m, fld, rng, out, fields, vals)
    v = tuple(2.0 * np.array([0.9, -0.7, 0.45]) * m.cell_len)
    moved = 0
    for _ in range(2):
        st = g.particles_step(fld, K, v, 0.5)
        ms = m.step(v, 0.5)
        assert (st["stayed"], st["moved"], st["lost"]) == (ms["stayed"], ms["moved"], ms["lost"])
        moved += ms["moved"]
    assert moved > 0
    _assert_model(g, fld, m)
    _deposit_and_gather(g, m, fld, rng, out, fields, vals)
    g.close()


def test_non_dyadic_geometry(gpu):
    g, m, fld, rng = _refined_case(7, ODD_START, ODD_L0, 46)
    out = g.add_field("rho", np.float64)
    fields, vals = _random_fields(g, m, rng, 3)
    _deposit_and_gather(g, m, fld, rng, out, fields, vals)
    g.close()


# ---- one full cell, empty pools ----------------------------------------------------
def test_one_full_cell_among_empty_cells(gpu):
    """300 records in the last cell (more than a wave and than a block), five
    in the first, 1 198 empty cells between them."""
    g, m, fld = _pair((12, 10, 10))
    rng = np.random.default_rng(47)
    last = int(m.leaves[-1])
    ctr, ln = m.o.geometry([1, last])
    for c, k, n in ((1, 0, 5), (last, 1, 300)):
        r = rng.random((n, 4)) * 2 - 1
        r[:, 0:3] = (ctr[k] - ln[k] / 2) + ln[k] * rng.random((n, 3))
        m.set(c, r)
    _upload_all(g, fld, m)
    dm = DepositModel(m)
    out = g.add_field("rho", np.float64)
    exp, got = _check_deposit(g, fld, dm, out, "cic", 3)
    assert sum(1 for v in got.values() if v != 0.0) > 27  # both clouds' neighborhoods, 1 and last are neighbors
    _check_deposit(g, fld, dm, out, "ngp", None)
    fields, vals = _random_fields(g, m, rng, 1)
    _check_gather(g, fld, dm, fields, vals, 3, "cic")
    g.close()


def test_empty_pool(gpu):
    g, m, fld = _pair((5, 4, 3))
    out = g.add_field("rho", np.float64)
    fields, vals = _random_fields(g, m, np.random.default_rng(48), 1)
    for upload in (False, True):
        if upload:
            _upload_all(g, fld, m)  # every cell sized to zero records
        out.set(np.full(g.n_slots, 7.0))
        g.particles_deposit(fld, out, 4, 3, "cic", per_volume=True)
        assert not out.get(0, g.n_local).any()
        g.particles_gather(fld, fields, 3, 4, "cic")
        assert int(fld.sizes().sum()) == 0
    g.close()


# ---- stretched geometry: NGP and per_volume ------------------------------------------
def test_ngp_per_volume_under_a_stretched_geometry(gpu):
    g, m, fld = _pair((4, 3, 2), R=1, periodic=(True, False, True), rounds=1, frac=0.2)
    g.set_stretched_geometry([[0.0, 0.5, 1.5, 3.0, 5.0], [-1.0, 0.0, 0.7, 2.0], [0.25, 1.0, 3.5]])
    rng = np.random.default_rng(49)
    _seed(m, rng, 5)  # NGP does not read the positions
    _upload_all(g, fld, m)
    L = [g.add_field(n, np.float64) for n in ("lx", "ly", "lz")]
    g.fill_geometry(length=L)
    lx, ly, lz = (f.get() for f in L)
    volumes = {int(c): (a * b) * d for c, a, b, d in zip(g.slot_ids(), lx, ly, lz)}
    assert len({round(v, 12) for v in volumes.values()}) > 4
    dm = DepositModel(m)
    out = g.add_field("rho", np.float64)
    _check_deposit(g, fld, dm, out, "ngp", 3, volumes=volumes)
    g.particles_deposit(fld, out, 4, None, "ngp", per_volume=True)
    want = np.array([np.float64(m.cells[int(c)].shape[0]) / volumes[int(c)] for c in g.slot_ids()[: g.n_local]])
    assert _same(out.get(0, g.n_local), want)
    with pytest.raises(Exception, match="Cartesian geometry"):
        g.particles_deposit(fld, out, 4, 3, "cic")
    with pytest.raises(Exception, match="Cartesian geometry"):
        g.particles_gather(fld, [out], 3, 4, "cic")
    g.particles_gather(fld, [L[0]], 3, 4, "ngp")
    for c, a in _local_cells(g, fld, 4).items():
        assert np.all(a[:, 3] == lx[list(g.slot_ids()).index(c)])
    g.close()


# ---- conservation, adjointness, reproducibility -------------------------------------
@pytest.fixture(scope="module")
def periodic_case(gpu):
    c = dict(REFINED, periodic=(True, True, True))
    g, m, fld = _pair(start=ODD_START, l0=ODD_L0, **c)
    rng = np.random.default_rng(50)
    _seed(m, rng, 5)
    _upload_all(g, fld, m)
    dm = DepositModel(m)
    out = g.add_field("rho", np.float64)
    exp, got = _check_deposit(g, fld, dm, out, "cic", 3)
    yield g, m, fld, dm, out, exp, got, rng
    g.close()


def test_conservation(periodic_case):
    g, m, fld, dm, out, exp, got, _ = periodic_case
    total = math.fsum(got.values())
    model = math.fsum(v[0] for v in exp.values())
    bound = sum((v[2] + 2) * EPS * v[1] for v in exp.values()) + 2 * EPS * abs(model)
    print("sum of out", total, "model", model, "bound", bound)
    assert abs(total - model) <= bound


def test_adjointness_on_the_device(periodic_case):
    """sum_c F_c rho_c against sum_p q_p G_p, both of device results: each
    rho_c and G_p is within its bound of the exact sum, the two outer sums
    are correctly rounded sums of rounded products."""
    g, m, fld, dm, out, exp, got, rng = periodic_case
    fields, vals = _random_fields(g, m, rng, 1)
    F = vals[0]
    gexp, after = _check_gather(g, fld, dm, fields, vals, 3, "cic")
    # (the gather overwrote double 3 on the device; the model still holds q)
    left = math.fsum(F[c] * got[c] for c in got)
    right = slack = T = 0.0
    terms = []
    for c, a in after.items():
        val, mag, cnt = gexp[c]
        q = m.cells[c][:, 3]
        terms.extend((q * a[:, 3]).tolist())
        slack += float(np.sum(np.abs(q) * ((cnt + 2) * EPS * mag[:, 0])))
        T += float(np.sum(np.abs(q) * mag[:, 0]))
    right = math.fsum(terms)
    slack += sum(abs(F[c]) * (exp[c][2] + 2) * EPS * exp[c][1] for c in got) + 4 * EPS * T
    print("adjointness", left, right, "bound", slack)
    assert T > 0 and abs(left - right) <= slack
    _upload_all(g, fld, m)  # q again, for the tests that follow


def test_reproducible(periodic_case):
    g, m, fld, dm, out, exp, got, _ = periodic_case
    other = g.add_field("rho2", np.float64)
    for pv in (False, True):
        g.particles_deposit(fld, out, 4, 3, "cic", per_volume=pv)
        a = out.get(0, g.n_local)
        g.particles_deposit(fld, other, 4, 3, "cic", per_volume=pv)
        g.particles_deposit(fld, out, 4, 3, "cic", per_volume=pv)
        assert _same(a, out.get(0, g.n_local)) and _same(a, other.get(0, g.n_local))


# ---- remote copies -------------------------------------------------------------------
def test_remote_copies_are_read_and_never_written(gpu):
    """The view of process 0 of 2 with the remote copies' records filled in:
    local cells take terms from them, their slots of `out` keep their values
    and their records are not gathered into."""
    g, m, fld = _pair(start=REF_START, l0=REF_L0, nprocs=2, **REFINED)
    rng = np.random.default_rng(51)
    _seed(m, rng, 5)
    _upload_all(g, fld, m)
    nl, nr = g.n_local, g.n_slots - g.n_local
    assert nr > 0
    dm = DepositModel(m)
    out = g.add_field("rho", np.float64)
    out.set(np.full(g.n_slots, -7.5))
    local = set(int(c) for c in g.slot_ids()[:nl])
    assert any(s not in local and m.cells[s].shape[0] and np.any(dm.weight(m.cells[s][:, 0:3], s, c) > 0)
               for c in local for s in dm.candidates(c)[1:])
    _check_deposit(g, fld, dm, out, "cic", 3)
    assert np.all(out.get(nl, nr) == -7.5)
    fields, vals = _random_fields(g, m, rng, 1)
    _check_gather(g, fld, dm, fields, vals, 3, "cic")  # compares the remote copies' records too
    g.close()


# ---- refusals ------------------------------------------------------------------------
def test_refusals(gpu):
    from oracle import oracle as O

    g, m, fld = _pair((4, 3, 2))
    out = g.add_field("rho", np.float64)
    u32 = g.add_field("u32", np.uint32)
    other = g.add_variable_field("other", np.float64, False)
    fld.set([np.zeros(4) for _ in range(g.n_slots)])
    g.particles_deposit(fld, out, 4, 3, "cic")
    for call in (lambda: g.particles_deposit(out, out, 4, 3, "cic"),
                 lambda: g.particles_gather(out, [out], 3, 4, "cic")):
        with pytest.raises(Exception, match="fixed-size"):
            call()
    for call in (lambda: g.particles_deposit(fld, other, 4, 3, "cic"),
                 lambda: g.particles_gather(fld, [out, other], 3, 5, "cic")):
        with pytest.raises(Exception, match="variable-size field has no fixed element layout"):
            call()
    for call in (lambda: g.particles_deposit(fld, u32, 4, 3, "cic"),
                 lambda: g.particles_gather(fld, [u32], 3, 4, "cic")):
        with pytest.raises(Exception, match="8-byte"):
            call()
    for call in (lambda: g.particles_deposit(fld, out, 2, None, "ngp"),
                 lambda: g.particles_gather(fld, [out], 3, 2, "ngp")):
        with pytest.raises(Exception, match="at least 3 doubles"):
            call()
    for call in (lambda: g.particles_deposit(fld, out, 3, None, "cic"),
                 lambda: g.particles_gather(fld, [out], 3, 5, "cic")):
        with pytest.raises(Exception, match="not a multiple of 8"):
            call()
    for w in (2, 4, -2, 0):
        with pytest.raises(Exception, match="weight_double"):
            g.particles_deposit(fld, out, 4, w, "cic")
    for first, n in ((2, 1), (4, 1), (3, 2)):
        with pytest.raises(Exception, match="first_double"):
            g.particles_gather(fld, [out] * n, first, 4, "cic")
    with pytest.raises(Exception, match="at least one cell field"):
        g.particles_gather(fld, [], 3, 4, "cic")
    ghost = types.SimpleNamespace(id=99)
    for call in (lambda: g.particles_deposit(ghost, out, 4, 3, "cic"),
                 lambda: g.particles_deposit(fld, ghost, 4, 3, "cic"),
                 lambda: g.particles_gather(fld, [ghost], 3, 4, "cic")):
        with pytest.raises(Exception, match="invalid field id"):
            call()
    for call in (lambda: g.particles_deposit(fld, out, 4, 3, 2),
                 lambda: g.particles_gather(fld, [out], 3, 4, -1)):
        with pytest.raises(Exception, match="shape must be 0"):
            call()
    # a stretched file block without coordinates: no geometry on the device
    g.set_geometry_block(O.stretched_geometry_block([[0.0, 0.5, 1.5, 3.0, 5.0], [0.0, 1.0, 2.0, 4.0], [0.0, 1.0, 2.0]]))
    for call in (lambda: g.particles_deposit(fld, out, 4, 3, "cic"),
                 lambda: g.particles_gather(fld, [out], 3, 4, "cic"),
                 lambda: g.particles_deposit(fld, out, 4, 3, "ngp", per_volume=True)):
        with pytest.raises(Exception, match="stretched geometry block"):
            call()
    g.particles_deposit(fld, out, 4, None, "ngp")  # neither positions nor lengths are needed
    assert np.all(out.get(0, g.n_local) == 1.0)
    g.close()
    g0, m0, f0 = _pair((4, 4, 4), hood=0)
    o0 = g0.add_field("rho", np.float64)
    f0.set([np.zeros(4) for _ in range(g0.n_slots)])
    for call in (lambda: g0.particles_deposit(f0, o0, 4, 3, "cic"),
                 lambda: g0.particles_gather(f0, [o0], 3, 4, "cic")):
        with pytest.raises(Exception, match="neighborhood length of at least 1"):
            call()
    g0.particles_deposit(f0, o0, 4, None, "ngp")
    assert np.all(o0.get(0, g0.n_local) == 1.0)
    g0.close()


# ---- several processes (host transport), run by the fixture below --------------------
def sc_deposit(rank, world):
    """The refined case across real processes with halo=True: the cells' sums
    and the records' gathered doubles, collected by id, are within the same
    bounds of the one-address-space model, and some local cell's sum has a
    term from the copy of a remote neighbor."""
    from oracle import oracle as O
    from helpers import random_refines
    from test_gpu_transport import _gather, _grid

    c = REFINED
    o = O.Grid(c["length"], c["R"], c["periodic"], c["hood"], world)
    rng = np.random.default_rng(0)
    for _ in range(c["rounds"]):
        ids, _ = o.cells()
        lv = o.mapping.batch(ids)["level"]
        for cell in random_refines(ids, lv, c["R"], rng, c["frac"]):
            o.refine_completely(cell)
        o.stop_refining()
    g = _grid(c["length"], c["R"], c["periodic"], c["hood"])
    g.set_cells(*o.cells())
    g.set_geometry(REF_START, REF_L0)
    K = 7
    m = ParticleModel(o, REF_START, REF_L0, K)
    fld = g.add_variable_field("particles", np.float64, True)
    _seed(m, np.random.default_rng(52), 5)
    local = [int(x) for x in g.slot_ids()[: g.n_local]]
    fld.set([m.cells[x].reshape(-1) for x in local])
    dm = DepositModel(m)
    frng = np.random.default_rng(53)
    vals = [{int(x): float(frng.random() * 2 - 1) for x in m.leaves} for _ in range(3)]
    fields = []
    for j, F in enumerate(vals):
        f = g.add_field(f"F{j}", np.float64)
        f.set(np.array([F[x] for x in local]), 0)  # the remote copies arrive with the halo
        fields.append(f)
    out = g.add_field("rho", np.float64)
    res = dict(remote_slots=g.n_slots > g.n_local)
    mine = set(local)
    res["remote_term"] = any(s not in mine and m.cells[s].shape[0] and np.any(dm.weight(m.cells[s][:, 0:3], s, x) > 0)
                             for x in local for s in dm.candidates(x)[1:])
    g.particles_deposit(fld, out, K, 3, "cic", per_volume=True, halo=True)
    rho = dict(zip(local, out.get(0, g.n_local)))
    g.particles_gather(fld, fields, 4, K, "cic", halo=True)
    recs = _local_cells(g, fld, K)
    parts = _gather((rho, recs))
    all_rho, all_recs = {}, {}
    for p in parts:
        all_rho.update(p[0])
        all_recs.update(p[1])
    exp = dm.deposit(1, 3)
    res["every_cell_once"] = sorted(all_rho) == sorted(m.cells) and sum(len(p[0]) for p in parts) == len(m.cells)
    ok = True
    for x, v in all_rho.items():
        total, mag, cnt, _ = exp[x]
        V = dm.volume(x)
        ok = ok and abs(v - total / V) <= (cnt + 2) * EPS * mag / V
    res["deposit"] = ok
    gexp = dm.gather(vals, 1)
    ok = keep = True
    for x, a in all_recs.items():
        val, mag, cnt = gexp[x]
        ok = ok and a.shape == m.cells[x].shape and bool(np.all(np.abs(a[:, 4:7] - val) <= (cnt[:, None] + 2) * EPS * mag))
        keep = keep and _same(np.ascontiguousarray(a[:, 0:4]), np.ascontiguousarray(m.cells[x][:, 0:4]))
    res["gather"] = ok
    res["untouched"] = keep
    res["any_remote_term"] = any(_gather(res.pop("remote_term")))
    res["any_remote_slots"] = any(_gather(res.pop("remote_slots")))
    g.close()
    return res


@pytest.fixture(scope="module")
def deposit_results(gpu, tmp_path_factory):
    from test_gpu_transport import _run_group

    return {w: _run_group(w, tmp_path_factory.mktemp(f"dw{w}"), names=["sc_deposit"],
                          module="test_gpu_particles_deposit") for w in (2, 3)}


@pytest.mark.parametrize("world", [2, 3])
def test_deposit_across_processes(deposit_results, world):
    results = deposit_results[world]
    assert "sc_deposit" in results and len(results["sc_deposit"]) == world
    for rank, (kind, out) in sorted(results["sc_deposit"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"
