"""dccrgx_particles_deposit_moments (particles_moments_kernel,
dccrg_amd/csrc/particles.hip) against the model of tests/moments_model.py.

Both sides form bitwise equal terms ((q u) v) W; only the order of a sum is
the kernel's, so with m non-zero terms the device may differ from the model's
fsum by (m + 2) 2^-52 sum|term| / V, the bound of test_gpu_particles_deposit.
The walk is the deposit's own, so an output with factors (-1, -1) has the
bits of particles_deposit's field.  A call of more than WIDTH moments runs
several passes: every width up to WIDTH, WIDTH + 1 (one output alone in a
second pass), 10 and 16 are all checked.  A miss is a bug, not noise."""
import math
import types

import numpy as np
import pytest

from deposit_model import DepositModel
from moments_model import RHO_J_P, MomentsModel
from particles_model import ParticleModel
from test_gpu_particles import REF_L0, REF_START, REFINED, _same
from test_gpu_particles_deposit import EPS, ODD_L0, ODD_START, SHAPES, _pair, _seed, _share_tol, _upload_all

pytestmark = pytest.mark.gpu

K = 10
WIDTH = 5  # kMW of particles.hip: the moments of one pass
# the charge, the current and the pressure, then repeats of record doubles, a
# square, the charge again (in the last pass) and factors in either place
SIXTEEN = RHO_J_P + [(7, 8), (9, None), (None, 9), (None, None), (8, 8), (6, 3)]
COUNTS = tuple(sorted({1, 2, 3, 4, WIDTH, WIDTH + 1, 10, 16}))  # every width has a kernel of its own


def _fields(g, n, prefix="m"):
    return [g.add_field(f"{prefix}{j}", np.float64) for j in range(n)]


def _check(g, fld, dm, outs, moments, exp, shape, weight, volumes=None, pvs=(True, False), exact=False):
    """outs after one call per per_volume setting against exp (the model's
    result for each moment); returns the device sums of the last call."""
    local = [int(c) for c in g.slot_ids()[: g.n_local]]
    got = None
    for pv in pvs:
        g.particles_deposit_moments(fld, outs, moments, K, weight, shape, per_volume=pv)
        got = [o.get(0, g.n_local) for o in outs]
        worst = 0.0
        for j, e in enumerate(exp):
            for c, v in zip(local, got[j]):
                total, mag, cnt = e[c]
                V = np.float64(1)
                if pv:
                    V = np.float64(volumes[c]) if volumes is not None else dm.volume(c)
                    total = total / V
                if exact:
                    assert np.float64(v).tobytes() == np.float64(total).tobytes(), (shape, pv, j, c, v, total)
                    continue
                bound = (cnt + 2) * EPS * mag / V
                worst = max(worst, abs(v - total) / bound if bound else abs(v - total))
                assert abs(v - total) <= bound, (shape, pv, moments[j], c, v, total, bound)
        print(f"moments {shape} n={len(outs)} weight={weight} per_volume={pv}: worst error {worst:.3f} of its bound")
    return [dict(zip(local, x)) for x in got]


# ---- refined grid ------------------------------------------------------------------
@pytest.fixture(scope="module")
def refined(gpu):
    g, m, fld = _pair(start=ODD_START, l0=ODD_L0, K=K, **REFINED)
    _seed(m, np.random.default_rng(81), 5)
    _upload_all(g, fld, m)
    dm = DepositModel(m)
    mm = MomentsModel(dm)
    outs = _fields(g, 16)
    yield g, m, fld, dm, mm, outs
    g.close()


@pytest.mark.parametrize("weight", [6, None])
@pytest.mark.parametrize("shape", ["cic", "ngp"])
def test_refined_grid(refined, shape, weight):
    g, m, fld, dm, mm, outs = refined
    exp = mm.moments(SHAPES[shape], weight, SIXTEEN)
    for n in COUNTS:
        _check(g, fld, dm, outs[:n], SIXTEEN[:n], exp[:n], shape, weight)
    # another order and other fields: a moment does not depend on its place
    order = [12, 3, 15, 0, 7]
    _check(g, fld, dm, [outs[15 - k] for k in range(5)], [SIXTEEN[j] for j in order], [exp[j] for j in order], shape,
           weight)


@pytest.mark.parametrize("weight", [6, None])
@pytest.mark.parametrize("shape", ["cic", "ngp"])
def test_charge_moment_has_the_bits_of_particles_deposit(refined, shape, weight):
    g, m, fld, dm, mm, outs = refined
    rho = g.add_field(f"rho_{shape}_{weight}", np.float64)
    charge = (None, None)
    two = [(3, None), (4, 4), (5, 6), (3, 4), (7, 8), (9, 9), (None, 5)][:WIDTH] * 2  # two passes
    for k in (0, WIDTH - 1, WIDTH, 2 * WIDTH - 1):  # the first and the last of either pass
        two[k] = charge
    lists = [[charge], two, [(3, 4)] * WIDTH + [charge]]  # ... and alone in a second pass
    for pv in (False, True):
        g.particles_deposit(fld, rho, K, weight, shape, per_volume=pv)
        want = rho.get(0, g.n_local)
        assert np.any(want != 0.0)
        for moments in lists:
            for o in outs[:len(moments)]:
                o.set(np.full(g.n_slots, 3.25))
            g.particles_deposit_moments(fld, outs[:len(moments)], moments, K, weight, shape, per_volume=pv)
            for o, mom in zip(outs, moments):
                if mom == charge:
                    assert _same(o.get(0, g.n_local), want), (shape, weight, pv, len(moments))


def test_two_calls_give_equal_bits_and_other_fields_keep_theirs(refined):
    g, m, fld, dm, mm, outs = refined
    moments = SIXTEEN[:6]
    for pv in (False, True):
        g.particles_deposit_moments(fld, outs[:6], moments, K, 6, "cic", per_volume=pv)
        first = [o.get(0, g.n_local) for o in outs[:6]]
        outs[6].set(np.full(g.n_slots, -2.5))
        outs[7].set(np.arange(g.n_slots, dtype=np.float64))
        g.particles_deposit_moments(fld, outs[8:14], moments, K, 6, "cic", per_volume=pv)
        g.particles_deposit_moments(fld, outs[:6], moments, K, 6, "cic", per_volume=pv)
        for a, o, p in zip(first, outs[:6], outs[8:14]):
            assert _same(a, o.get(0, g.n_local)) and _same(a, p.get(0, g.n_local))
        assert np.all(outs[6].get() == -2.5)
        assert np.array_equal(outs[7].get(), np.arange(g.n_slots, dtype=np.float64))


# ---- exact -----------------------------------------------------------------------
def test_exact_case_is_bitwise(gpu):
    """l0 = 1, start = 0, positions on eighths of the finest cell, q and v on
    2^-10: every product and sum is exact in any order."""
    g, m, fld = _pair(K=K, **REFINED)
    _seed(m, np.random.default_rng(82), 5)
    for rec in m.cells.values():
        rec[:, 0:3] = np.round(rec[:, 0:3] * 32) / 32
        rec[:, 3:] = np.round(rec[:, 3:] * 1024) / 1024
    _upload_all(g, fld, m)
    dm = DepositModel(m)
    mm = MomentsModel(dm)
    outs = _fields(g, 10)
    for shape in ("cic", "ngp"):
        exp = mm.moments(SHAPES[shape], 6, RHO_J_P)
        _check(g, fld, dm, outs, RHO_J_P, exp, shape, 6, pvs=(False, True), exact=True)
    g.close()


# ---- tiny periodic grid ------------------------------------------------------------
def test_tiny_periodic_grid(gpu):
    """3 x 1 x 1 fully periodic: every row lists the cell itself and its two
    neighbors many times over, and a cloud overlaps its own cell's images."""
    g, m, fld = _pair((3, 1, 1), start=ODD_START, l0=ODD_L0, K=K)
    rng = np.random.default_rng(83)
    _seed(m, rng, 4)
    extra = rng.random((1, K)) * 2 - 1
    extra[0, 0:3] = [0.1 + 0.3 + 0.01, -0.3 + 0.69, 0.2 + 0.02]  # near three faces
    m.set(2, np.concatenate([m.cells[2], extra]))
    _upload_all(g, fld, m)
    dm = DepositModel(m)
    mm = MomentsModel(dm)
    outs = _fields(g, 10)
    exp = mm.moments(1, 6, RHO_J_P)
    got = _check(g, fld, dm, outs, RHO_J_P, exp, "cic", 6)
    _check(g, fld, dm, outs, RHO_J_P, mm.moments(0, 6, RHO_J_P), "ngp", 6)
    _check(g, fld, dm, outs, RHO_J_P, mm.moments(1, None, RHO_J_P), "cic", None)
    # nothing leaves a periodic grid (the last call above was without per_volume; this one too)
    got = _check(g, fld, dm, outs, RHO_J_P, exp, "cic", 6, pvs=(False,))
    for j, (total, mag) in enumerate(mm.totals(6, RHO_J_P)):
        slack = sum((v[2] + 2) * EPS * v[1] for v in exp[j].values()) + (_share_tol(m) + 2 * EPS) * mag
        assert abs(math.fsum(got[j].values()) - total) <= slack, (j, slack)
    g.close()


# ---- one full cell, empty pools ----------------------------------------------------
def test_one_full_cell_among_empty_cells(gpu):
    """300 records in the last cell (more than a wave and than a block), five
    in the first, 1 198 empty cells between them."""
    g, m, fld = _pair((12, 10, 10), K=K)
    rng = np.random.default_rng(84)
    last = int(m.leaves[-1])
    ctr, ln = m.o.geometry([1, last])
    for c, k, n in ((1, 0, 5), (last, 1, 300)):
        r = rng.random((n, K)) * 2 - 1
        r[:, 0:3] = (ctr[k] - ln[k] / 2) + ln[k] * rng.random((n, 3))
        m.set(c, r)
    _upload_all(g, fld, m)
    dm = DepositModel(m)
    mm = MomentsModel(dm)
    outs = _fields(g, 10)
    got = _check(g, fld, dm, outs, RHO_J_P, mm.moments(1, 6, RHO_J_P), "cic", 6)
    assert sum(1 for v in got[0].values() if v != 0.0) > 27  # both clouds' neighborhoods
    _check(g, fld, dm, outs[:WIDTH + 1], RHO_J_P[:WIDTH + 1], mm.moments(0, None, RHO_J_P[:WIDTH + 1]), "ngp", None)
    g.close()


def test_empty_pool(gpu):
    g, m, fld = _pair((5, 4, 3), K=K)
    outs = _fields(g, 6)
    other = g.add_field("other", np.float64)
    other.set(np.full(g.n_slots, 9.0))
    for upload in (False, True):
        if upload:
            _upload_all(g, fld, m)  # every cell sized to zero records
        for shape in ("cic", "ngp"):
            for o in outs:
                o.set(np.full(g.n_slots, 7.0))
            g.particles_deposit_moments(fld, outs[:5], RHO_J_P[:5], K, 6, shape, per_volume=True)
            for o in outs[:5]:
                assert not o.get(0, g.n_local).any()
            assert np.all(outs[5].get() == 7.0) and np.all(other.get() == 9.0)
    g.close()


# ---- remote copies -------------------------------------------------------------------
def test_remote_copies_are_read_and_never_written(gpu):
    """The view of process 0 of 2 with the remote copies' records filled in:
    local cells take terms from them, their slots of every output keep a
    sentinel."""
    g, m, fld = _pair(start=REF_START, l0=REF_L0, K=K, nprocs=2, **REFINED)
    _seed(m, np.random.default_rng(85), 5)
    _upload_all(g, fld, m)
    nl, nr = g.n_local, g.n_slots - g.n_local
    assert nr > 0
    dm = DepositModel(m)
    mm = MomentsModel(dm)
    local = set(int(c) for c in g.slot_ids()[:nl])
    assert any(s not in local and m.cells[s].shape[0] and np.any(dm.weight(m.cells[s][:, 0:3], s, c) > 0)
               for c in local for s in dm.candidates(c)[1:])
    outs = _fields(g, 10)
    for o in outs:
        o.set(np.full(g.n_slots, -7.5))
    _check(g, fld, dm, outs, RHO_J_P, mm.moments(1, 6, RHO_J_P), "cic", 6)
    for o in outs:
        assert np.all(o.get(nl, nr) == -7.5)
    g.close()


# ---- stretched geometry: NGP and per_volume ------------------------------------------
def test_ngp_per_volume_under_a_stretched_geometry(gpu):
    g, m, fld = _pair((4, 3, 2), R=1, periodic=(True, False, True), rounds=1, frac=0.2, K=K)
    g.set_stretched_geometry([[0.0, 0.5, 1.5, 3.0, 5.0], [-1.0, 0.0, 0.7, 2.0], [0.25, 1.0, 3.5]])
    _seed(m, np.random.default_rng(86), 5)  # NGP does not read the positions
    _upload_all(g, fld, m)
    L = [g.add_field(n, np.float64) for n in ("lx", "ly", "lz")]
    g.fill_geometry(length=L)
    lx, ly, lz = (f.get() for f in L)
    volumes = {int(c): (a * b) * d for c, a, b, d in zip(g.slot_ids(), lx, ly, lz)}
    assert len({round(v, 12) for v in volumes.values()}) > 4
    dm = DepositModel(m)
    mm = MomentsModel(dm)
    outs = _fields(g, 5)
    _check(g, fld, dm, outs, RHO_J_P[:5], mm.moments(0, 6, RHO_J_P[:5]), "ngp", 6, volumes=volumes)
    rho = g.add_field("rho", np.float64)
    g.particles_deposit(fld, rho, K, 6, "ngp", per_volume=True)
    g.particles_deposit_moments(fld, outs, RHO_J_P[:5], K, 6, "ngp", per_volume=True)
    assert _same(outs[0].get(0, g.n_local), rho.get(0, g.n_local))  # the deposit's volumes
    with pytest.raises(Exception, match="Cartesian geometry"):
        g.particles_deposit(fld, rho, K, 6, "cic")
    with pytest.raises(Exception, match="CIC needs a Cartesian geometry"):
        g.particles_deposit_moments(fld, outs, RHO_J_P[:5], K, 6, "cic")
    g.close()


# ---- refusals ------------------------------------------------------------------------
def test_refusals(gpu):
    from dccrg_amd._lib import EINVAL
    from oracle import oracle as O

    g, m, fld = _pair((4, 3, 2), K=K)
    outs = _fields(g, 17)
    u32 = g.add_field("u32", np.uint32)
    other = g.add_variable_field("other", np.float64, False)
    fld.set([np.zeros(K) for _ in range(g.n_slots)])
    one = [(None, None)]
    g.particles_deposit_moments(fld, outs[:1], one, K, 6, "cic")
    ghost = types.SimpleNamespace(id=99)
    calls = [(lambda: g.particles_deposit_moments(outs[1], outs[:1], one, K, 6, "cic"), "fixed-size"),
             (lambda: g.particles_deposit_moments(ghost, outs[:1], one, K, 6, "cic"), "invalid field id"),
             (lambda: g.particles_deposit_moments(fld, [ghost], one, K, 6, "cic"), "invalid field id"),
             (lambda: g.particles_deposit_moments(fld, outs[:1], one, 2, None, "ngp"), "at least 3 doubles"),
             (lambda: g.particles_deposit_moments(fld, outs[:1], one, 3, None, "cic"), "not a multiple of 8"),
             (lambda: g.particles_deposit_moments(fld, outs[:1], one, K, 6, 2), "shape must be 0"),
             # n outside 1 .. 16
             (lambda: g.particles_deposit_moments(fld, [], [], K, 6, "cic"), "number of moments"),
             (lambda: g.particles_deposit_moments(fld, outs, [(3, 4)] * 17, K, 6, "cic"), "number of moments"),
             # an output that is no fixed 8-byte field
             (lambda: g.particles_deposit_moments(fld, [outs[0], u32], one * 2, K, 6, "cic"), "8-byte"),
             (lambda: g.particles_deposit_moments(fld, [other], one, K, 6, "cic"),
              "variable-size field has no fixed element layout"),
             # two equal outputs
             (lambda: g.particles_deposit_moments(fld, [outs[0], outs[1], outs[0]], [(3, 4)] * 3, K, 6, "cic"),
              "share an output")]
    calls += [(lambda w=w: g.particles_deposit_moments(fld, outs[:1], one, K, w, "cic"), "weight_double")
              for w in (2, K, -2, 0)]
    # a factor that is neither -1 nor in [3, K)
    calls += [(lambda f=f: g.particles_deposit_moments(fld, outs[:2], [(3, None), f], K, 6, "cic"), "moment factor")
              for f in ((2, None), (None, K), (-2, 3), (0, 0), (5, K + 3))]
    for call, match in calls:
        with pytest.raises(Exception, match=match) as e:
            call()
        assert e.value.code == EINVAL, match
    g.particles_deposit_moments(fld, outs[:16], [(3, 4)] * 16, K, 6, "cic")  # 16 are allowed
    # a stretched file block without coordinates: no geometry on the device
    g.set_geometry_block(O.stretched_geometry_block([[0.0, 0.5, 1.5, 3.0, 5.0], [0.0, 1.0, 2.0, 4.0], [0.0, 1.0, 2.0]]))
    for call in (lambda: g.particles_deposit_moments(fld, outs[:1], one, K, 6, "cic"),
                 lambda: g.particles_deposit_moments(fld, outs[:1], one, K, 6, "ngp", per_volume=True)):
        with pytest.raises(Exception, match="stretched geometry block"):
            call()
    g.particles_deposit_moments(fld, outs[:1], one, K, None, "ngp")  # neither positions nor lengths are needed
    assert np.all(outs[0].get(0, g.n_local) == 1.0)
    g.close()
    g0, m0, f0 = _pair((4, 4, 4), hood=0, K=K)
    o0 = g0.add_field("rho", np.float64)
    f0.set([np.zeros(K) for _ in range(g0.n_slots)])
    with pytest.raises(Exception, match="neighborhood length of at least 1"):
        g0.particles_deposit_moments(f0, [o0], one, K, 6, "cic")
    g0.particles_deposit_moments(f0, [o0], one, K, None, "ngp")
    assert np.all(o0.get(0, g0.n_local) == 1.0)
    g0.close()


# ---- real processes (host transport), run by the fixture below -----------------------
def sc_moments(rank, world):
    """The refined case across real processes with halo=True: four moments
    collected by id are within the bounds of the one-address-space model, and
    some local cell's sum has a term from the copy of a remote neighbor."""
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
    m = ParticleModel(o, REF_START, REF_L0, K)
    fld = g.add_variable_field("particles", np.float64, True)
    _seed(m, np.random.default_rng(87), 5)
    local = [int(x) for x in g.slot_ids()[: g.n_local]]
    fld.set([m.cells[x].reshape(-1) for x in local])  # the remote copies arrive with the halo
    dm = DepositModel(m)
    mm = MomentsModel(dm)
    moments = RHO_J_P[:4]
    outs = [g.add_field(f"m{j}", np.float64) for j in range(4)]
    res = dict(remote_slots=g.n_slots > g.n_local)
    mine = set(local)
    res["remote_term"] = any(s not in mine and m.cells[s].shape[0] and np.any(dm.weight(m.cells[s][:, 0:3], s, x) > 0)
                             for x in local for s in dm.candidates(x)[1:])
    g.particles_deposit_moments(fld, outs, moments, K, 6, "cic", per_volume=True, halo=True)
    parts = _gather([dict(zip(local, f.get(0, g.n_local))) for f in outs])
    exp = mm.moments(1, 6, moments)
    ok = once = True
    for j in range(4):
        every = {}
        for p in parts:
            every.update(p[j])
        once = once and sorted(every) == sorted(m.cells) and sum(len(p[j]) for p in parts) == len(m.cells)
        for x, v in every.items():
            total, mag, cnt = exp[j][x]
            V = dm.volume(x)
            ok = ok and abs(v - total / V) <= (cnt + 2) * EPS * mag / V
    res["every_cell_once"] = once
    res["moments"] = ok
    res["any_remote_term"] = any(_gather(res.pop("remote_term")))
    res["any_remote_slots"] = any(_gather(res.pop("remote_slots")))
    g.close()
    return res


@pytest.fixture(scope="module")
def moments_results(gpu, tmp_path_factory):
    from test_gpu_transport import _run_group

    return _run_group(2, tmp_path_factory.mktemp("mw2"), names=["sc_moments"], module="test_gpu_particles_moments")


def test_moments_across_processes(moments_results):
    results = moments_results
    assert "sc_moments" in results and len(results["sc_moments"]) == 2
    for rank, (kind, out) in sorted(results["sc_moments"].items()):
        assert kind == "ok", f"rank {rank}:\n{out}"
        for k, v in out.items():
            assert v, f"rank {rank}: {k} failed ({out})"
