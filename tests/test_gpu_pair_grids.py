"""Pair-count grids of every chain on the device (mhx_get_pair_grids, Engine.pair_grids,
walker_set_corner_grid; walker-plot-corner mcmc-fitting.lisp:1333-1359 as counts).  The yardstick
is the chain's own trace, e.trace(c, take), binned on the host by the rule of the histograms and
counted in two dimensions; every comparison is np.array_equal on integers over ALL chains."""
import ctypes

import numpy as np
import pytest

import histo_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def test_crafted_walks_d2_reference_edges(mhx):
    e = hc.crafted_d2(mhx)
    pairs = [(0, 1), (1, 0)]
    for take in (1, 57, 1000, 2048):
        windows = hc.traces(e, take)
        for bins in (1, 2, 20, 64):
            edges = hc.reference_edges(mhx, e, take, [0, 1], bins)
            r = e.pair_grids(take, [0, 1], pairs, edges)
            assert hc.same(r, hc.want_pair_grids(windows, [0, 1], pairs, edges)), (take, bins)
            assert np.array_equal(r["counts"].sum(axis=(2, 3)), r["n_inside"])
            assert np.array_equal(r["counts"][:, 1], r["counts"][:, 0].transpose(0, 2, 1))
            assert (r["n_inside"] <= r["n_used"][:, None]).all() and (r["status"] == 0).all()
    e.close()


def test_wide_vector_pairs_over_some_columns_shared_edges(mhx):
    e = hc.crafted_d33(mhx)
    for take in (57, 2048):
        windows = hc.traces(e, take)
        for bins in (7, 64):
            edges = hc.narrow_edges(3, bins)
            r = e.pair_grids(take, hc.COLS33, hc.PAIRS, edges)
            assert hc.same(r, hc.want_pair_grids(windows, hc.COLS33, hc.PAIRS, edges)), (take, bins)
            assert (r["n_inside"] < r["n_used"][:, None]).any()       # the edges are narrower
            assert np.array_equal(r["counts"].sum(axis=(2, 3)), r["n_inside"])
    # no pair at all: the windows are still reported
    r = e.pair_grids(57, hc.COLS33, [], hc.narrow_edges(3, 7))
    assert r["counts"].shape == (40, 0, 7, 7) and np.array_equal(r["n_used"], [len(t) for t in hc.traces(e, 57)])
    e.close()


def test_a_column_with_a_nan(mhx):
    rng = np.random.default_rng(4)
    e = hc.line_engine(mhx, 3, d=3, used=(0, 2), history_capacity=64)
    e.init_chains([-1.0, 0.5, 2.0])
    walks = [rng.normal(0.0, 1.0, (50, 3)) for _ in range(3)]
    walks[1][7, 2], walks[1][9, 0] = np.nan, np.inf
    for c, th in enumerate(walks):
        e.set_history(c, rng.normal(-5.0, 1.0, 50), th)
    edges = np.array([np.linspace(-2.0, 2.0, 9)] * 3)
    pairs = [(0, 1), (0, 2), (2, 1)]
    r = e.pair_grids(50, [0, 1, 2], pairs, edges)
    assert hc.same(r, hc.want_pair_grids(hc.traces(e, 50), [0, 1, 2], pairs, edges))
    assert r["status"].tolist() == [[0, 0, 0], [0, 1, 1], [0, 0, 0]]
    e.close()


def test_corner_grid_of_a_walker_set(mhx):
    """walker_set_corner_grid at d = 4: the 6 pairs in the reference's order, every chain's grids on
    make-histo's own edges for that chain; a window past the ring is warned about once"""
    import warnings
    rng = np.random.default_rng(6)
    n, d = 5, 4
    e = hc.line_engine(mhx, n, d=d, used=(0, 1), history_capacity=64)
    e.init_chains([-1.0, 2.0, 0.0, 1.0])
    for c in range(n):
        e.set_history(c, *hc.crafted_walk(rng, 40 + 200 * c, d, 2 * (c % 2)))
    ring = e.history_capacity()
    keys = ["b", "m", "much_better_name", "w"]
    w = mhx.Walker(e, None, keys, None, None, None, None)
    order = [("b", "m"), ("b", "much_better_name"), ("b", "w"), ("m", "much_better_name"), ("m", "w"),
             ("much_better_name", "w")]
    for take, bins in ((None, 20), (30, 5)):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got = mhx.walker_set_corner_grid(w, take=take, bins=bins)
        trunc = [x for x in rec if issubclass(x.category, mhx.walker.HistoryTruncated)]
        assert len(trunc) == (1 if take is None and 40 + 200 * (n - 1) > ring else 0)
        window = ring if take is None else take
        edges = hc.reference_edges(mhx, e, window, range(d), bins)
        places = [(a, b) for a in range(d) for b in range(a + 1, d)]
        want = hc.want_pair_grids(hc.traces(e, window), range(d), places, edges)
        assert len(got) == n
        for c in range(n):
            assert [p for p, _ in got[c]] == order
            for q in range(6):
                assert np.array_equal(got[c][q][1], want["counts"][c, q]), (take, c, q)
    only = mhx.walker_set_corner_grid(w, take=30, bins=5, keys=[":w", ":b"])
    assert [p for p, _ in only[0]] == [("w", "b")]
    assert np.array_equal(only[2][0][1], got[2][2][1].T)
    e.close()


def test_a_ring_that_has_wrapped(mhx):
    e = hc.line_engine(mhx, 8, seed=5)
    e.init_chains(np.array([-1.0, 2.0]) + 0.01 * np.arange(8)[:, None])
    e.many_steps(1500, np.diag([0.05, 0.05]))
    for take in (1000, 1024):
        edges = hc.reference_edges(mhx, e, take, [0, 1], 20)
        r = e.pair_grids(take, [0, 1], [(0, 1)], edges)
        assert hc.same(r, hc.want_pair_grids(hc.traces(e, take), [0, 1], [(0, 1)], edges)), take
    e.close()


def test_counting_in_memory_gives_the_counts_of_lds(mhx, tmp_path_factory):
    here, child = hc.lds_results(mhx), hc.no_lds_results(tmp_path_factory)
    names = [n for n in here if n.startswith("g")]
    assert len(names) == 3
    for n in names:
        assert hc.same(child[n], here[n]), n
        assert here[n]["counts"].sum() > 0


def free_device_bytes():
    """hipMemGetInfo of the runtime the library runs on"""
    hip = ctypes.CDLL("libamdhip64.so.7")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_arguments_and_a_call_too_large_for_one_chain(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = hc.line_engine(mhx, 1)
    e.init_chains([-1.0, 2.0])
    edges = np.array([np.linspace(-4.0, 4.0, 65)] * 2)

    def refused(fn):
        with pytest.raises(mhx.MhxError) as err:
            fn()
        assert err.value.code == capi.EINVAL and str(err.value)
        return str(err.value)

    small = e.pair_grids(1, [0, 1], [(0, 1)], edges)
    assert small["n_inside"].tolist() == [[1]] and small["counts"].sum() == 1
    refused(lambda: e.pair_grids(1, [0, 1], [(0, 1)], np.array([np.linspace(-4.0, 4.0, 66)] * 2)))   # 65 bins
    refused(lambda: e.pair_grids(1, [0, 1], [(0, 0)], edges))
    refused(lambda: e.pair_grids(1, [0, 1], [(0, 2)], edges))
    refused(lambda: e.pair_grids(1, [0, 1], [(0, 1)] * 4097, edges))
    refused(lambda: e.pair_grids(0, [0, 1], [(0, 1)], edges))
    refused(lambda: e.pair_grids(1, [1, 1], [(0, 1)], edges))
    # 4096 pairs of 64 x 64 cells are 64 MiB of counts for ONE chain: refused, and nothing grows
    before = free_device_bytes()
    msg = refused(lambda: e.pair_grids(1, [0, 1], [(0, 1), (1, 0)] * 2048, edges))
    assert "ONE chain" in msg
    assert free_device_bytes() > before - (32 << 20)
    # ... 4090 pairs fit: their counts and the rest are 67078580 bytes of the 67108864
    r = e.pair_grids(1, [0, 1], [(0, 1), (1, 0)] * 2045, edges)
    assert (r["n_inside"] == 1).all() and np.array_equal(r["counts"][0, 0], small["counts"][0, 0])
    assert free_device_bytes() < before - (32 << 20)     # (that call did need the room)
    fresh = hc.line_engine(mhx, 2)
    with pytest.raises(mhx.MhxError) as err:
        fresh.pair_grids(1, [0, 1], [(0, 1)], edges)
    assert err.value.code == capi.ESTATE
    fresh.close()
    e.close()


def test_group_equals_a_single_engine(mhx):
    rng = np.random.default_rng(50)
    n, d = 49, 3
    e = hc.line_engine(mhx, n, d=d, used=(0, 2), history_capacity=256)
    g = mhx.Group(n, d, 1, devices=[0, 0], history_capacity=256)
    g.set_function(0, mhx.capi.MODEL_POLY, (), [0, 2])
    g.set_dataset(0, hc.LF_X, hc.LF_Y, np.full(5, 0.2))
    for obj in (e, g):
        obj.init_chains([-1.0, 0.5, 2.0])
    walks = [hc.crafted_walk(rng, int(rng.integers(1, 257)), d, c % 3) for c in range(n)]
    for part, (first, count) in zip([e] + g.engines, [(0, n)] + g.ranges):
        for c in range(count):
            part.set_history(c, *walks[first + c])
    cols, pairs = [2, 0, 1], [(0, 1), (2, 0), (1, 2)]
    for take in (1, 100, 256):
        for edges in (hc.reference_edges(mhx, e, take, cols, 20), hc.narrow_edges(3, 20)):
            single, whole = e.pair_grids(take, cols, pairs, edges), g.pair_grids(take, cols, pairs, edges)
            assert hc.same(whole, single), take
            assert hc.same(single, hc.want_pair_grids(hc.traces(e, take), cols, pairs, edges)), take
    e.close()
    g.close()
