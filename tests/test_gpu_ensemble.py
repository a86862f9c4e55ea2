"""Ensemble percentiles: ONE posterior from all chains of a walker set, selected exactly on the
device (mhx_get_ensemble_percentiles, Engine/Group.ensemble_percentiles, walker_set_ensemble_get).
The yardstick is walker._percentile (nth-percentile M:1495-1506) on the concatenation of the
chains' windows as e.trace(c, take) delivers them; every comparison is np.array_equal (a NaN equal
to a NaN) over all percentiles and columns of the call."""
import ctypes as C
import warnings

import numpy as np
import pytest

import ensemble_cases as ec
import histo_cases as hc
import problems as pb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


@pytest.fixture(scope="module")
def d3(mhx):
    e = ec.crafted_d3(mhx)
    yield e
    e.close()


_windows = {}


def windows_of(e, take):
    key = (id(e), take)
    if key not in _windows:
        _windows[key] = hc.traces(e, take)
    return _windows[key]


def as_walker(mhx, e):
    keys = ["p%d" % j for j in range(e.d)]
    return mhx.Walker(e, None, keys, None, None, None, None), keys


def check(mhx, got, windows, cols=None, include=None, pcts=ec.PCTS):
    """a result against the yardstick on `windows`: out, n_pooled, n_used, status"""
    d = windows[0].shape[1]
    cols = list(range(d)) if cols is None else cols
    pool = ec.pooled(windows, include)[:, cols]
    assert ec.same(got["out"], ec.yardstick(mhx, pool, pcts).reshape(len(pcts), len(cols)))
    used = [len(th) if include is None or include[c] else 0 for c, th in enumerate(windows)]
    assert got["n_used"].tolist() == used and got["n_pooled"] == sum(used) == len(pool)
    assert got["status"].tolist() == [int(np.isnan(pool[:, j]).any()) for j in range(len(cols))]


@pytest.mark.parametrize("take", ec.TAKES)
def test_crafted_walks_of_every_length(mhx, d3, take):
    """walks of 1 to 2048 steps on a ring of 2048, d = 3: repeated steps, ties, neighbours in the
    last bit; the pool is the sum of the windows, whatever their lengths"""
    got = ec.call(d3, take)
    check(mhx, got, windows_of(d3, take))
    assert got["n_pooled"] == sum(min(take, n) for n in hc.LENGTHS)
    assert got["n_used"].tolist() == [min(take, n) for n in hc.LENGTHS]
    if take >= 64:      # the runs of equal steps put `between` ranks inside runs and at their ends
        assert len(np.unique(got["out"])) > 12


def special_engine(mhx, walks):
    e = hc.line_engine(mhx, len(walks), d=walks[0].shape[1], history_capacity=64)
    e.init_chains([-1.0, 2.0])
    for c, th in enumerate(walks):
        e.set_history(c, -np.arange(1.0, len(th) + 1), th)
    return e


def test_special_pools(mhx):
    rng = np.random.default_rng(5)
    sp = ec.special_values()
    # column 0: one value in every step of every chain - every pass leaves one bin; column 1: zeros
    # of both signs, infinities, subnormals, neighbours in the last bit
    walks = [np.column_stack([np.full(n, -0.75), rng.choice(sp, n)]) for n in (1, 5, 64, 37)]
    e = special_engine(mhx, walks)
    got = ec.call(e, 64)
    check(mhx, got, hc.traces(e, 64))
    assert (got["out"][:, 0] == -0.75).all() and got["status"].tolist() == [0, 0]
    assert got["out"][ec.PCTS.index(0), 1] == -np.inf and got["out"][ec.PCTS.index(100), 1] == np.inf
    # zeros of both signs alone: every point is a zero
    zeros = [np.column_stack([rng.choice([0.0, -0.0], n), rng.choice([0.0, -0.0], n)]) for n in (3, 64, 10, 2)]
    for c, th in enumerate(zeros):
        e.set_history(c, -np.arange(1.0, len(th) + 1), th)
    got = ec.call(e, 64)
    check(mhx, got, hc.traces(e, 64))
    assert (got["out"] == 0.0).all()
    # a NaN in one chain, in column 1 only: it sorts last and marks that column alone
    walks[2][17, 1] = np.nan
    for c, th in enumerate(walks):
        e.set_history(c, -np.arange(1.0, len(th) + 1), th)
    for cols in ([0, 1], [1, 0], [1], [0]):
        got = ec.call(e, 64, cols)
        check(mhx, got, hc.traces(e, 64), cols)
        assert got["status"].tolist() == [int(p == 1) for p in cols]
        if 1 in cols:
            column = got["out"][:, cols.index(1)]
            assert np.isnan(column[ec.PCTS.index(100)]) and not np.isnan(np.delete(column, ec.PCTS.index(100))).any()
    # the chain that holds it left out: no mark
    assert ec.call(e, 64, None, [1, 1, 0, 1])["status"].tolist() == [0, 0]
    e.close()


def test_a_subset_of_the_columns_in_another_order(mhx, d3):
    full = ec.call(d3, 1000)
    for cols in ([2, 0], [1], [1, 2, 0], [0, 1, 2]):
        part = ec.call(d3, 1000, cols)
        assert part["out"].shape == (len(ec.PCTS), len(cols))
        for j, p in enumerate(cols):
            assert ec.same(part["out"][:, j], full["out"][:, p]), (cols, p)
        assert part["n_pooled"] == full["n_pooled"] and np.array_equal(part["n_used"], full["n_used"])


def test_include_equals_an_engine_of_those_chains(mhx, d3):
    n = d3.n_chains
    windows = windows_of(d3, 2048)
    masks = [[c % 3 != 1 for c in range(n)], [c == 8 for c in range(n)], [c >= 9 for c in range(n)], [True] * n]
    for mask in masks:
        got = ec.call(d3, 1000, None, mask)
        check(mhx, got, windows_of(d3, 1000), None, mask)
        assert all((u == 0) == (not m) for u, m in zip(got["n_used"], mask))
        # ... and an engine that holds only those chains' walks
        kept = [c for c in range(n) if mask[c]]
        e = hc.line_engine(mhx, len(kept), d=3, used=(0, 2), history_capacity=2048)
        e.init_chains([-1.0, 0.5, 2.0])
        for i, c in enumerate(kept):
            e.set_history(i, -np.arange(1.0, len(windows[c]) + 1), windows[c])
        alone = ec.call(e, 1000)
        e.close()
        assert ec.same(alone["out"], got["out"]) and alone["n_pooled"] == got["n_pooled"]
        assert np.array_equal(alone["n_used"], got["n_used"][kept])
    with pytest.raises(mhx.MhxError) as err:
        ec.call(d3, 1000, None, [False] * n)
    assert err.value.code == mhx.capi.EINVAL
    with pytest.raises(ValueError):
        ec.call(d3, 1000, None, [True] * (n - 1))


def test_keys_in_lds_and_keys_from_memory_give_the_same_bits(mhx, tmp_path_factory):
    """every case a second time in a child process with MHX_ENSEMBLE_NO_LDS=1; and a call whose
    columns cannot fit LDS by themselves (3 chains, d = 63, 2048 steps, all columns) against the
    yardstick"""
    here, child = ec.lds_results(mhx), ec.no_lds_results(tmp_path_factory)
    assert set(here) == set(child) and len(here) == len(ec.TAKES) + 4
    for name in here:
        assert sorted(here[name]) == sorted(child[name]) == ["n_pooled", "n_used", "out", "status"]
        for k in here[name]:
            assert ec.same(here[name][k], child[name][k]) and here[name][k].dtype == child[name][k].dtype, (name, k)
    e = ec.wide_engine(mhx)
    windows = hc.traces(e, 2048)
    e.close()
    assert all(th.shape == (2048, 63) for th in windows)
    for results in (here, child):
        check(mhx, {k: (int(v) if k == "n_pooled" else v) for k, v in results["wide"].items()}, windows)
        check(mhx, {k: (int(v) if k == "n_pooled" else v) for k, v in results["wide_few"].items()}, windows,
              [62, 0, 31])


def test_a_real_walk_on_a_group_and_on_one_engine(mhx):
    s = pb.two_peak(n=2500, seed=4)
    n = 49
    th0 = pb.perturbed(s.theta_star, n, 0.01, seed=6)
    e = s.engine(mhx, n, seed=10)
    g = mhx.Group(n, s.d, s.K, devices=[0, 0], seed=10)
    s.apply(g)
    for obj in (e, g):
        obj.init_chains(th0)
        obj.adaptive_begin(30000, 10.0, 1)
        obj.adaptive_advance(1500)
    assert g.ranges == [(0, 25), (25, 24)]
    mask = [c % 5 != 0 and not 20 <= c < 30 for c in range(n)]      # chains of both engines' ranges
    assert any(mask[:25]) and any(mask[25:]) and not all(mask[:25]) and not all(mask[25:])
    for take in (1, 200, 1024):
        windows = hc.traces(e, take)
        for cols, include in ((None, None), ([7, 0, 3], mask)):
            single, whole = ec.call(e, take, cols, include), ec.call(g, take, cols, include)
            for k in ("out", "n_used", "status"):
                assert ec.same(whole[k], single[k]), (take, k)
            assert whole["n_pooled"] == single["n_pooled"]
            check(mhx, single, windows, cols, include)
    assert len(np.unique(single["out"])) == single["out"].size      # a posterior, not a constant
    e.close()
    g.close()


def test_more_chains_than_the_chip_holds_at_once(mhx):
    """3000 workgroups on a short ring; the yardstick's windows come from ONE mhx_get_derived call
    whose expressions are the parameters themselves"""
    n = 3000
    e = hc.line_engine(mhx, n, seed=3, history_capacity=8)
    e.init_chains(np.array([-1.0, 2.0]) + 1e-3 * np.arange(n)[:, None])
    e.many_steps(40, np.diag([0.05, 0.05]))
    ring = e.history_capacity()
    r = e.derived(["a", "b"], ["a", "b"], [0, 1], ring, values=True)
    windows = [r["values"][c, :, :r["n_used"][c]].T for c in range(n)]
    assert len({len(th) for th in windows}) == 1 and len(windows[0]) >= 8
    mask = (np.arange(n) % 7 != 3)
    for include in (None, mask):
        got = ec.call(e, ring, None, include)
        check(mhx, got, windows, None, include)
    short = ec.call(e, 3, [1])
    check(mhx, short, [th[:3] for th in windows], [1])
    assert e.summary_timing() > 0.0
    e.close()


def test_arguments_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    n, d = 3, 2
    e = hc.line_engine(mhx, n, history_capacity=64)
    _a, cols = capi.as_i32([1, 0])
    _b, num = capi.as_i32([50, 5])
    _c, den = capi.as_i32([1, 2])
    out = np.full((2, 2), -7.0)
    used, status = np.full(n, -7, dtype=np.int32), np.full(2, -7, dtype=np.int32)
    pooled = C.c_int64(-7)
    outs = [out.ctypes.data_as(capi.f64p), C.byref(pooled), used.ctypes.data_as(capi.i32p),
            status.ctypes.data_as(capi.i32p)]

    def call(take=10, cols_=cols, n_cols=2, include=None, num_=num, den_=den, n_pct=2, outs_=outs):
        return lib.mhx_get_ensemble_percentiles(e._h, take, cols_, n_cols, include, num_, den_, n_pct, *outs_)

    def untouched():
        return (out == -7.0).all() and (used == -7).all() and (status == -7).all() and pooled.value == -7

    assert call() == capi.ESTATE and untouched()          # before mhx_init_chains
    e.init_chains([-1.0, 2.0])
    ring = e.history_capacity()
    mask = np.zeros(n, dtype=np.uint8)
    bad = [dict(take=0), dict(take=ring + 1), dict(n_cols=0), dict(n_cols=d + 1), dict(cols_=None),
           dict(cols_=capi.as_i32([1, 1])[1]), dict(cols_=capi.as_i32([0, d])[1]), dict(cols_=capi.as_i32([-1, 0])[1]),
           dict(n_pct=-1), dict(n_pct=17), dict(num_=None), dict(den_=None), dict(num_=capi.as_i32([50, 201])[1]),
           dict(num_=capi.as_i32([-1, 5])[1]), dict(den_=capi.as_i32([1, 0])[1]),
           dict(include=mask.ctypes.data_as(capi.u8p))]
    for kw in bad:
        assert call(**kw) == capi.EINVAL and lib.mhx_last_error() and untouched(), sorted(kw)
    assert lib.mhx_get_ensemble_percentiles(None, 10, cols, 2, None, num, den, 2, *outs) == capi.EINVAL
    assert lib.mhx_group_get_ensemble_percentiles(None, 10, cols, 2, None, num, den, 2, *outs) == capi.EINVAL
    assert untouched()
    assert call(outs_=[None] * 4) == capi.OK              # every output may be NULL
    for k in range(4):                                    # ... and each one alone
        assert call(outs_=[o if j != k else None for j, o in enumerate(outs)]) == capi.OK
    out[:], used[:], status[:], pooled.value = -7.0, -7, -7, -7
    assert call(n_pct=0, num_=None, den_=None) == capi.OK     # no percentile: only the counts
    assert (out == -7.0).all() and used.tolist() == [1, 1, 1] and status.tolist() == [0, 0] and pooled.value == 3
    # a chain in MHX_CHAIN_FP_TRAP is served from the history it has; cols = [1, 0]
    e.close()
    e = hc.line_engine(mhx, n, history_capacity=64)
    e.init_chains([[-1.0, 2.0], [1e308, 1e308], [0.5, 1.5]])
    assert e.chain_status()[0][1] == capi.CHAIN_FP_TRAP
    e.set_history(2, [-1.0, -2.0], [[3.0, 5.0], [1.0, 6.0]])
    mask[:] = [1, 0, 1]
    assert call(include=mask.ctypes.data_as(capi.u8p)) == capi.OK
    assert used.tolist() == [1, 0, 2] and pooled.value == 3 and status.tolist() == [0, 0]
    assert out.tolist() == [[5.0, 1.0], [3.5, 0.0]]       # the median; the 2.5 % point: (e[0] + e[1]) / 2
    assert call() == capi.OK and pooled.value == 4 and used.tolist() == [1, 1, 2]
    assert out[0].tolist() == [5.5, 2.0]                  # of (2, 5, 6, 1e308) and (-1, 1, 3, 1e308)
    e.close()
    g = mhx.Group(4, 2, 1, devices=[0, 0])
    assert lib.mhx_group_get_ensemble_percentiles(g._h, 10, cols, 2, None, num, den, 2, *outs) == capi.ESTATE
    g.close()


SELECTORS = [":median-params", ":95cr", ":iqr", ":stddev-normal", (":percentile", 84.1), (":percentile", 0),
             (":percentile", 100)]


def test_the_walker_level(mhx, d3):
    e = d3
    w, keys = as_walker(mhx, e)
    take = 1000
    mask = [c % 2 == 0 for c in range(e.n_chains)]
    for include in (None, mask):
        r = e.ensemble_percentiles(take, [50, 2.5, 97.5, 25, 75, 84.1, 0, 100], None, include)["out"]
        want = {":median-params": lambda j: r[0, j], ":95cr": lambda j: [r[1, j], r[2, j]],
                ":iqr": lambda j: r[4, j] - r[3, j], ":stddev-normal": lambda j: r[5, j] - r[0, j],
                (":percentile", 84.1): lambda j: r[5, j], (":percentile", 0): lambda j: r[6, j],
                (":percentile", 100): lambda j: r[7, j]}
        for get in SELECTORS:
            got = mhx.walker_set_ensemble_get(w, get, take, None, include)
            assert list(got) == keys
            for j, k in enumerate(keys):
                assert got[k] == want[get](j), (get, k)
                assert isinstance(got[k], list if get == ":95cr" else float)
    # keys pick and order the columns; the default is the median of 1000 steps of every chain
    some = mhx.walker_set_ensemble_get(w, ":95cr", take, [":p2", "p0"])
    assert list(some) == ["p2", "p0"] and some["p0"] == mhx.walker_set_ensemble_get(w, ":95cr", take)["p0"]
    assert mhx.walker_set_ensemble_get(w) == mhx.walker_set_ensemble_get(w, ":median-params", 1000)
    for bad in (":mean", ":median", ":percentile", (":percentile", 101), (":95cr", 3), ":steps"):
        with pytest.raises(ValueError):
            mhx.walker_set_ensemble_get(w, bad)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # nothing reaches past the ring
        mhx.walker_set_ensemble_get(w, ":iqr", 2048)


def test_a_window_past_the_ring_warns_once(mhx):
    e = hc.line_engine(mhx, 4, seed=2, history_capacity=64)
    e.init_chains([-1.0, 2.0])
    ring = e.history_capacity()
    e.many_steps(ring + 36, np.diag([0.05, 0.05]))
    w, keys = as_walker(mhx, e)
    with pytest.warns(mhx.walker.HistoryTruncated) as seen:
        got = mhx.walker_set_ensemble_get(w, ":median-params", ring + 30)
    assert len(seen) == 1
    pool = ec.pooled(hc.traces(e, ring))
    assert [got[k] for k in keys] == ec.yardstick(mhx, pool, [50])[0].tolist()
    e.close()
