"""bench.py's --full and --dump-outputs (no GPU needed): the options parse,
a plain run asks for no CPU baseline, and dump_outputs writes the local
cells' result in cell-id order as float32 / float64, cut to a fixed seeded
sample when larger than its share of the budget."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


class Field:
    def __init__(self, v):
        self.v = v

    def get(self, lo, n):
        return self.v[lo:lo + n]


class Grid:
    """Slots in a scrambled order, two halo slots behind the local ones."""

    def __init__(self, n, seed=3):
        self.n_local = n
        self.ids = np.concatenate([np.random.default_rng(seed).permutation(n).astype(np.uint64) + 1,
                                   np.array([10 ** 9, 10 ** 9 + 1], np.uint64)])

    def slot_ids(self):
        return self.ids


def test_options_parse_and_plain_run_is_lean():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert not bench.want_cpu_baseline(a, 1)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    assert bench.want_cpu_baseline(a, 1) and not bench.want_cpu_baseline(a, 2)
    assert not bench.want_cpu_baseline(bench.parse(["--full", "--no-cpu-baseline"]), 1)


def test_dump_outputs_orders_by_cell_id(tmp_path):
    g = Grid(1000)
    ids = g.ids[:1000]
    rho = Field(np.concatenate([ids.astype(np.float64) * 0.5, [-1.0, -1.0]]))
    alive = Field(np.concatenate([(ids % np.uint64(3) == 0).astype(np.uint32), np.zeros(2, np.uint32)]))
    a = bench.parse(["--dump-outputs", str(tmp_path / "o")])
    bench.dump_outputs(a, g, 0, 1, {"density": rho, "is_alive": alive})
    d = np.load(tmp_path / "o" / "density.npy")
    s = np.load(tmp_path / "o" / "is_alive.npy")
    assert d.dtype == np.float64 and s.dtype == np.float32
    assert np.array_equal(d, np.arange(1, 1001) * 0.5)
    assert np.array_equal(s, (np.arange(1, 1001) % 3 == 0).astype(np.float32))
    bench.dump_outputs(bench.parse([]), g, 0, 1, {"density": rho})  # no option: nothing written
    assert sorted(os.listdir(tmp_path / "o")) == ["density.npy", "is_alive.npy"]


def test_dump_outputs_samples_large_arrays_the_same_way(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8 * 300)
    n = 5000
    outs = []
    for seed in (3, 4):  # two slot orders of the same cells
        g = Grid(n, seed)
        f = Field(np.concatenate([np.sqrt(g.ids[:n].astype(np.float64)), [0.0, 0.0]]))
        a = bench.parse(["--dump-outputs", str(tmp_path / str(seed))])
        bench.dump_outputs(a, g, 1, 2, {"density": f})
        outs.append(np.load(tmp_path / str(seed) / "density.rank1.npy"))
    assert 200 < outs[0].size <= 300 and outs[0].nbytes <= 8 * 300
    assert np.array_equal(outs[0], outs[1])
    assert np.all(np.diff(outs[0]) > 0)  # id order, every sampled cell once
