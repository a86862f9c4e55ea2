"""Posterior histograms of every chain on the device (mhx_get_histograms, Engine.histograms,
walker_set_param_histo; walker-param-histo mcmc-fitting.lisp:1361-1369, make-histo 1541-1564).
The yardstick is always the chain's own trace, e.trace(c, take), and the bin rule on the host (a
value falls in bin n = the smallest n in 1..B with v <= edge n); every comparison is
np.array_equal on integers and covers ALL chains of its engine."""
import numpy as np
import pytest

import histo_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


@pytest.fixture(scope="module")
def d2(mhx):
    e = hc.crafted_d2(mhx)
    yield e
    e.close()


@pytest.fixture(scope="module")
def d33(mhx):
    e = hc.crafted_d33(mhx)
    yield e
    e.close()


def as_walker(mhx, e):
    keys = ["p%d" % j for j in range(e.d)]
    return mhx.Walker(e, None, keys, None, None, None, None), keys


def test_crafted_walks_reference_edges_every_chain_and_key(mhx, d2):
    """300 chains, d = 2, windows of 1 to 2048 steps, 1 to 1024 bins, make-histo's own edges per
    chain: walker_set_param_histo is make_histo of the trace column; Engine.histograms is the bin
    rule, nothing falls below, and what make-histo drops above its last edge is counted there"""
    e = d2
    w, keys = as_walker(mhx, e)
    dropped = 0
    for take in (1, 57, 1000, 2048):
        windows = hc.traces(e, take)
        for bins in (1, 2, 20, 1024):
            got = mhx.walker_set_param_histo(w, None, take, bins)
            assert len(got) == e.n_chains
            for c, th in enumerate(windows):
                assert list(got[c]) == keys
                for j, k in enumerate(keys):
                    col = np.sort(th[:, j])
                    assert got[c][k][1] == mhx.make_histo(col, bins), (take, bins, c, k)
                    assert got[c][k][0] == mhx.make_histo_x(col, bins), (take, bins, c, k)
            edges = hc.reference_edges(mhx, e, take, [0, 1], bins)
            r = e.histograms(take, [0, 1], edges)
            assert hc.same(r, hc.want_histograms(windows, [0, 1], edges)), (take, bins)
            assert np.array_equal(r["counts"].sum(axis=2) + r["outside"][:, :, 1],
                                  np.broadcast_to(r["n_used"][:, None], (e.n_chains, 2))), (take, bins)
            assert (r["outside"][:, :, 0] == 0).all() and (r["status"] == 0).all()
            assert np.array_equal(r["counts"], np.array([[got[c][k][1] for k in keys]
                                                         for c in range(e.n_chains)]))
            dropped += int((r["outside"][:, :, 1] > 0).sum())
    assert dropped > 0    # a last edge rounded below the greatest value somewhere


def test_wide_vector_some_columns_out_of_order_shared_edges(d33):
    e = d33
    for take in (57, 2048):
        windows = hc.traces(e, take)
        for bins in (1, 20):
            edges = hc.narrow_edges(3, bins)
            r = e.histograms(take, hc.COLS33, edges)
            assert hc.same(r, hc.want_histograms(windows, hc.COLS33, edges)), (take, bins)
            assert (r["outside"][:, :, 0] > 0).any() and (r["outside"][:, :, 1] > 0).any()
            assert np.array_equal(r["counts"].sum(axis=2) + r["outside"].sum(axis=2),
                                  np.broadcast_to(r["n_used"][:, None], (e.n_chains, 3)))


def test_values_that_are_not_finite(mhx):
    rng = np.random.default_rng(3)
    e = hc.line_engine(mhx, 4, history_capacity=64)
    e.init_chains([-1.0, 2.0])
    walks = [rng.normal(0.0, 2.0, (40, 2)) for _ in range(4)]
    walks[1][3, 0], walks[1][5, 0], walks[1][17, 0] = np.nan, np.inf, -np.inf
    walks[2][0, 1], walks[2][39, 1], walks[2][20, 1] = -np.inf, np.nan, np.inf
    for c, th in enumerate(walks):
        e.set_history(c, rng.normal(-5.0, 1.0, 40), th)
    finite = np.array([np.linspace(-3.0, 3.0, 11)] * 2)
    open_ended = finite.copy()
    open_ended[:, 0], open_ended[:, -1] = -np.inf, np.inf
    windows = hc.traces(e, 40)
    for edges in (finite, open_ended):
        r = e.histograms(40, [0, 1], edges)
        assert hc.same(r, hc.want_histograms(windows, [0, 1], edges))
        assert r["status"].tolist() == [[0, 0], [1, 0], [0, 1], [0, 0]]
        total = r["counts"].sum(axis=2) + r["outside"].sum(axis=2)
        assert total.tolist() == [[40, 40], [39, 40], [40, 39], [40, 40]]    # the NaN is nowhere
    r = e.histograms(40, [0, 1], finite)
    assert r["outside"][1, 0, 0] >= 1 and r["outside"][1, 0, 1] >= 1         # -inf below, +inf above
    r = e.histograms(40, [0, 1], open_ended)
    # -inf equals the first edge: bin 1; +inf equals the last: the last bin
    assert (r["outside"] == 0).all() and r["counts"][1, 0, 0] >= 1 and r["counts"][1, 0, -1] >= 1
    e.close()


def test_a_ring_that_has_wrapped(mhx):
    e = hc.line_engine(mhx, 8, seed=5)
    e.init_chains(np.array([-1.0, 2.0]) + 0.01 * np.arange(8)[:, None])
    assert e.history_capacity() == 1024
    e.many_steps(1500, np.diag([0.05, 0.05]))
    assert (e.state()["length"] > 1024).all()
    for take in (1000, 1024):
        windows = hc.traces(e, take)
        assert all(len(th) == take for th in windows)
        for bins in (20, 1024):
            edges = hc.reference_edges(mhx, e, take, [1, 0], bins)
            r = e.histograms(take, [1, 0], edges)
            assert hc.same(r, hc.want_histograms(windows, [1, 0], edges)), (take, bins)
            assert (r["counts"].sum(axis=2) + r["outside"][:, :, 1] == take).all()
    e.close()


def test_counting_in_memory_gives_the_counts_of_lds(mhx, tmp_path_factory):
    here, child = hc.lds_results(mhx), hc.no_lds_results(tmp_path_factory)
    assert set(here) == set(child)
    names = [n for n in here if n.startswith("h")]
    assert len(names) == 5
    for n in names:
        assert hc.same(child[n], here[n]), n
        assert here[n]["counts"].sum() > 0


def test_chains_beyond_one_portion(mhx):
    """d = 33, all columns, 1024 bins, edges per chain: a chain's pieces are 33 x 1025 doubles of
    edges, 33 x 1024 counts, 33 x 2 outside, n_used and 33 status, 406168 bytes, so 165 chains
    fill the 64 MiB of a portion and 200 chains are worked through in two.  (These pieces exceed
    the LDS of a workgroup: the counts go straight to memory.)"""
    rng = np.random.default_rng(165)
    d, nb, n, ring = 33, 1024, 200, 8
    per_chain = 8 * d * (nb + 1) + 4 * d * nb + 8 * d + 4 + 4 * d
    assert per_chain == 406168 and ((1 << 26) - 5 * 256) // per_chain == 165 < n
    e = hc.line_engine(mhx, n, d=d, used=range(0, 32, 4), history_capacity=ring)
    e.init_chains(np.linspace(-1.0, 2.0, d))
    for c in range(n):
        steps = 1 + c % ring
        e.set_history(c, rng.normal(-5.0, 1.0, steps), rng.normal(0.0, 2.0, (steps, d)))
    cols = list(range(d))
    edges = np.sort(rng.normal(0.0, 2.0, (n, d, nb + 1)), axis=2)
    r = e.histograms(ring, cols, edges)
    want = hc.want_histograms(hc.traces(e, ring), cols, edges)
    for c in (0, 1, 163, 164, 165, 166, 198, 199):      # first, last, either side of the boundary
        assert all(np.array_equal(r[k][c], want[k][c]) for k in want), c
    assert hc.same(r, want)
    assert np.array_equal(r["n_used"], 1 + np.arange(n) % ring)
    assert (r["counts"].sum(axis=2) + r["outside"].sum(axis=2) == r["n_used"][:, None]).all()
    e.close()


def test_arguments_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    n, d, nb = 3, 2, 4
    e = hc.line_engine(mhx, n)
    _c, cols = capi.as_i32([1, 0])
    edges = np.array([[[0.0, 1.0, 2.0, 3.0, 4.0]] * 2] * n)
    counts = np.full((n, 2, nb), -7, dtype=np.int32)
    outside = np.full((n, 2, 2), -7, dtype=np.int32)
    used, status = np.full(n, -7, dtype=np.int32), np.full((n, 2), -7, dtype=np.int32)
    outs = [a.ctypes.data_as(capi.i32p) for a in (counts, outside, used, status)]

    def call(take=10, cols_=cols, n_cols=2, n_bins=nb, edges_=edges, per_chain=1, outs_=outs):
        rc = lib.mhx_get_histograms(e._h, take, cols_, n_cols, n_bins, edges_.ctypes.data_as(capi.f64p),
                                    per_chain, *outs_)
        return rc, lib.mhx_last_error().decode()

    assert call()[0] == capi.ESTATE                       # before mhx_init_chains
    e.init_chains([-1.0, 2.0])
    ring = e.history_capacity()
    wide = np.zeros((n, 2, 1026)) + np.arange(1026)

    def refused(**kw):
        rc, msg = call(**kw)
        assert rc == capi.EINVAL and msg, kw
        assert call()[0] == capi.OK                       # the engine works as before
        assert (used == 1).all()
        return msg

    refused(take=0)
    refused(take=ring + 1)
    refused(n_bins=0)
    refused(n_bins=1025, edges_=wide)
    _d, twice = capi.as_i32([1, 1])
    refused(cols_=twice)
    _e, beyond = capi.as_i32([0, d])
    refused(cols_=beyond)
    refused(n_cols=0)
    refused(n_cols=d + 1)
    bad = edges.copy()
    bad[2, 1, 3] = 1.5                                    # below the edge before it
    msg = refused(edges_=bad)
    assert "chain 2" in msg and "column 1" in msg
    bad = edges.copy()
    bad[1, 0, 4] = np.nan
    msg = refused(edges_=bad)
    assert "chain 1" in msg and "column 0" in msg and "NaN" in msg
    # ... a bad row of a chain's edges is none of the shared set's business
    assert call(edges_=bad, per_chain=0)[0] == capi.OK
    assert call(outs_=[None] * 4)[0] == capi.OK           # every output may be NULL
    assert call(n_bins=1024, edges_=wide[:, :, :1025].copy(), outs_=[None] * 4)[0] == capi.OK
    assert lib.mhx_group_get_histograms(None, 10, cols, 2, nb, edges.ctypes.data_as(capi.f64p), 1,
                                        *outs) == capi.EINVAL
    # the one step every chain has, theta = (-1, 2): column 1 (cols[0]) is 2, on edge 2 -> bin 2;
    # column 0 is -1: below
    assert call()[0] == capi.OK
    assert counts[:, 0].tolist() == [[0, 1, 0, 0]] * n and (counts[:, 1] == 0).all()
    assert outside[:, 0].tolist() == [[0, 0]] * n and outside[:, 1].tolist() == [[1, 0]] * n
    assert (status == 0).all()
    e.close()


def test_group_equals_a_single_engine(mhx):
    rng = np.random.default_rng(49)
    n, d = 49, 3
    e = hc.line_engine(mhx, n, d=d, used=(0, 2), history_capacity=256)
    g = mhx.Group(n, d, 1, devices=[0, 0], history_capacity=256)
    g.set_function(0, mhx.capi.MODEL_POLY, (), [0, 2])
    g.set_dataset(0, hc.LF_X, hc.LF_Y, np.full(5, 0.2))
    for obj in (e, g):
        obj.init_chains([-1.0, 0.5, 2.0])
    assert g.ranges == [(0, 25), (25, 24)]
    walks = [hc.crafted_walk(rng, int(rng.integers(1, 257)), d, c % 3) for c in range(n)]
    for part, (first, count) in zip([e] + g.engines, [(0, n)] + g.ranges):
        for c in range(count):
            part.set_history(c, *walks[first + c])
    for take in (1, 100, 256):
        per_chain = hc.reference_edges(mhx, e, take, [2, 0], 20)
        if take > 1:    # the chains' edges differ: their order matters
            assert len({per_chain[c].tobytes() for c in range(n)}) > n // 2
        for edges in (per_chain, hc.narrow_edges(2, 20)):
            single, whole = e.histograms(take, [2, 0], edges), g.histograms(take, [2, 0], edges)
            assert hc.same(whole, single), take
            assert hc.same(single, hc.want_histograms(hc.traces(e, take), [2, 0], edges)), take
    e.close()
    g.close()
