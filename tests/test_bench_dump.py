"""bench.py --dump-outputs without a GPU: what it writes for a fleet of stand-in engines - every
array float64, one row per chain, and past the size limit a fixed sample of the chains whose ids
are written beside them."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Engine:
    def __init__(self, first, n, d):
        self.first, self.n, self.d = first, n, d

    def lmatrix(self):
        c = np.arange(self.first, self.first + self.n, dtype=np.float64)
        return c[:, None, None] + np.zeros((self.n, self.d, self.d))

    def temperature(self):
        return np.arange(self.first, self.first + self.n, dtype=np.float64) + 0.5


class _Fleet:
    """the Fleet surface dump_outputs reads: obj.state() over all chains, per-engine read-backs"""

    def __init__(self, n_engines, n, d):
        self.engines = [_Engine(i * n, n, d) for i in range(n_engines)]
        total = n_engines * n
        c = np.arange(total, dtype=np.float64)

        class _Obj:
            def state(self_):
                return dict(theta=c[:, None] + np.zeros((total, d)), logpost=-c,
                            best_theta=c[:, None] + np.ones((total, d)), best_logpost=-c - 1,
                            length=np.arange(total, dtype=np.int64), age=np.arange(total, dtype=np.int64))
        self.obj = _Obj()


def _read(out_dir, names):
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in names)
    return {n: np.load(os.path.join(out_dir, n + ".npy")) for n in names}


def test_dump_of_every_chain(tmp_path):
    b = load_bench()
    names = b.dump_outputs(_Fleet(2, 300, 8), str(tmp_path))
    a = _read(str(tmp_path), names)
    assert "chain_index" not in a
    assert a["theta"].shape == (600, 8) and a["lmatrix"].shape == (600, 8, 8)
    for n, x in a.items():
        assert x.dtype == np.float64 and len(x) == 600, n
    # the engines' read-backs line up with the group's state, chain for chain
    assert np.array_equal(a["lmatrix"][:, 0, 0], a["theta"][:, 0])
    assert np.array_equal(a["temperature"] - 0.5, a["length"])


def test_dump_past_the_limit_is_a_fixed_sample(tmp_path):
    b = load_bench()
    n, d = 65536, 16   # config 3's chains and parameters: ~150 MB in full
    written = []
    for i in range(2):
        out_dir = str(tmp_path / ("run%d" % i))
        names = b.dump_outputs(_Fleet(1, n, d), out_dir)
        assert sum(os.path.getsize(os.path.join(out_dir, k + ".npy")) for k in names) < 64e6
        written.append(_read(out_dir, names))
    a, again = written
    idx = a["chain_index"]
    assert a["chain_index"].dtype == np.float64 and 1000 < len(idx) < n
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
    for k, x in a.items():
        assert len(x) == len(idx), k
        assert np.array_equal(x, again[k]), k
    assert np.array_equal(a["theta"][:, 0], idx) and np.array_equal(a["lmatrix"][:, 3, 5], idx)
