"""Autocorrelation time, effective sample size and the half moments of split R-hat of every chain
on the device (mhx_get_autocorr, Engine.autocorr, walker_set_autocorr, walker_set_rhat).  The
yardstick is tests/autocorr_cases.py's serial implementation of the definitions on the chain's own
trace, e.trace(c, take); every comparison is on the float bits (any NaN equal to any NaN) and
covers ALL chains and columns of its engine, acf up to n_lags, what the device does not write
keeping the caller's fill."""
import warnings

import numpy as np
import pytest

import autocorr_cases as ac
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


_windows = {}


def windows_of(e, take):
    """hc.traces(e, take), read once per engine and take"""
    key = (id(e), take)
    if key not in _windows:
        _windows[key] = hc.traces(e, take)
    return _windows[key]


def as_walker(mhx, e):
    keys = ["p%d" % j for j in range(e.d)]
    return mhx.Walker(e, None, keys, None, None, None, None), keys


@pytest.mark.parametrize("take,max_lag", ac.D2_SHAPES)
def test_crafted_walks_every_chain_column_and_output(d2, take, max_lag):
    """300 chains, d = 2, ring 2048, walks of 1 to 2048 steps: windows of one step (no lag, no
    halves), two, three (a middle step in neither half), and lags on either side of a block of 64"""
    e = d2
    got = ac.engine_autocorr(e, take, [0, 1], max_lag)
    want = ac.want_autocorr(windows_of(e, take), [0, 1], max_lag)
    assert ac.same(got, want) is None
    assert np.array_equal(got["n_lags"], np.minimum(max_lag, got["n_used"] - 1))
    assert (got["status"] & ac.NONFINITE == 0).all()
    one = got["n_used"] == 1
    assert one.any() and (got["status"][one] == ac.CONSTANT | ac.OPEN).all()
    assert np.isnan(got["half_mean"][one]).all() and np.isnan(got["acf"][one]).all()
    if take == 2:       # two steps: the same twice, or a single P_0 that is positive
        two = got["n_used"] == 2
        assert two.sum() > 250 and set(np.unique(got["status"][two])) == {ac.CONSTANT, ac.OPEN}
    if take >= 1000 and max_lag >= 63:
        assert set(np.unique(got["status"])) == {0, 2, 4, 6}


def test_wide_vector_some_columns_out_of_order(d33):
    e = d33
    for take in (57, 2048):
        got = ac.engine_autocorr(e, take, hc.COLS33, 64)
        assert ac.same(got, ac.want_autocorr(windows_of(e, take), hc.COLS33, 64)) is None, take
    # every column of the long windows: 33 x 2048 doubles are beyond a workgroup's LDS
    cols = list(range(33))
    got = ac.engine_autocorr(e, 2048, cols, 64)
    assert ac.same(got, ac.want_autocorr(windows_of(e, 2048), cols, 64)) is None


def test_values_that_are_not_finite(mhx):
    e = ac.nonfinite_engine(mhx)
    for cols in ([0, 1], [1, 0]):
        got = ac.engine_autocorr(e, 40, cols, 20)
        want = ac.want_autocorr(hc.traces(e, 40), cols, 20)
        marked = ac.NONFINITE_HIT[:, cols]
        assert ac.same(got, want, unspecified=marked) is None
        assert np.array_equal((got["status"] & ac.NONFINITE) != 0, marked)    # exactly the hit columns
        assert (got["status"][~marked] == 0).all() and np.isfinite(got["tau"][~marked]).all()
    e.close()


def test_a_ring_that_has_wrapped(mhx):
    e = ac.wrapped_engine(mhx)
    for take in (1000, 1024):
        windows = hc.traces(e, take)
        assert all(len(th) == take for th in windows)
        got = ac.engine_autocorr(e, take, [1, 0], 255)
        assert ac.same(got, ac.want_autocorr(windows, [1, 0], 255)) is None, take
        assert (got["n_used"] == take).all() and (got["n_lags"] == 255).all()
        assert np.isfinite(got["tau"]).all() and (got["tau"] > 1.0).all()
    e.close()


def test_reading_the_window_from_memory_gives_the_bits_of_lds(mhx, tmp_path_factory):
    """every case above a second time, in a child process with MHX_AUTOCORR_NO_LDS=1: the same bits.
    The walk of the wrapped rings is the child's own, so its results also face the yardstick on the
    child's own steps: slot arithmetic over a ring that has wrapped, read from memory."""
    here, child = ac.lds_results(mhx), ac.no_lds_results(tmp_path_factory)
    assert set(here) == set(child) and len(here) == len(ac.D2_SHAPES) + 2 + 2 + 2 + 1
    steps = child["wrapped_windows"]["theta"]
    assert steps.shape == (8, 1024, 2)
    for take in (1000, 1024):
        want = ac.want_autocorr([th[:take] for th in steps], [1, 0], 255)
        assert ac.same(child["wrapped_%d" % take], want) is None, take
    assert np.array_equal(steps, here["wrapped_windows"]["theta"])    # the walk is the same in both
    for name in here:
        if name == "wrapped_windows":
            continue
        marked = ac.NONFINITE_HIT[:, [int(name[-2]), int(name[-1])]] if name.startswith("nonfinite") else None
        assert ac.same(child[name], here[name], unspecified=marked) is None, name
        assert np.isfinite(here[name]["tau"]).any() or name == "d2_1_255"


def test_chains_beyond_one_portion(mhx):
    """d = 33, all columns, 1024 lags: a chain's pieces are 33 x 1024 doubles of rho and 33 x 52 + 8
    bytes of the rest, 272060 bytes, so 246 chains fill the 64 MiB of a portion and 300 chains are
    worked through in two (tests/test_autocorr_stage_plan.py has the carver's own answer)."""
    rng = np.random.default_rng(246)
    d, max_lag, n, ring = 33, 1023, 300, 64
    per_chain = 8 * d * (max_lag + 1) + d * (8 + 8 + 16 + 16 + 4) + 8
    per_portion = ((1 << 26) - 8 * 256) // per_chain
    assert per_chain == 272060 and per_portion == 246 and -(-n // per_portion) == 2
    answer = ac.carver_answers(["%d %d" % (d, max_lag)])      # carve_autocorr's own portion
    assert answer is not None, "a C++ compiler is needed to ask csrc/mhx_stage.hpp"
    assert -(-n // int(answer[0].split()[0])) == 2 and int(answer[0].split()[0]) == per_portion
    e = hc.line_engine(mhx, n, d=d, used=range(0, 32, 4), history_capacity=ring)
    e.init_chains(np.linspace(-1.0, 2.0, d))
    for c in range(n):
        e.set_history(c, *hc.crafted_walk(rng, 1 + c % ring, d, c % 3))
    cols = list(range(d))
    got = ac.engine_autocorr(e, ring, cols, max_lag)
    want = ac.want_autocorr(hc.traces(e, ring), cols, max_lag)
    for c in (0, 1, 244, 245, 246, 247, 298, 299):      # first, last, either side of the boundary
        assert all(ac.same_bits(got[k][c], want[k][c]) for k in want), c
    assert ac.same(got, want) is None
    assert np.array_equal(got["n_used"], 1 + np.arange(n) % ring)
    e.close()


def test_arguments_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    n, d, max_lag = 3, 2, 5
    e = hc.line_engine(mhx, n, history_capacity=64)
    _c, cols = capi.as_i32([1, 0])
    f64 = {k: np.full(shape, -7.0) for k, shape in (("tau", (n, 2)), ("ess", (n, 2)), ("acf", (n, 2, max_lag + 1)),
                                                    ("half_mean", (n, 2, 2)), ("half_var", (n, 2, 2)))}
    i32 = {k: np.full(shape, -7, dtype=np.int32) for k, shape in (("n_lags", n), ("n_used", n), ("status", (n, 2)))}
    outs = [a.ctypes.data_as(capi.f64p) for a in f64.values()] + [a.ctypes.data_as(capi.i32p) for a in i32.values()]

    def call(take=10, cols_=cols, n_cols=2, max_lag_=max_lag, outs_=outs):
        rc = lib.mhx_get_autocorr(e._h, take, cols_, n_cols, max_lag_, *outs_)
        return rc, lib.mhx_last_error().decode()

    assert call()[0] == capi.ESTATE                       # before mhx_init_chains
    e.init_chains([-1.0, 2.0])
    ring = e.history_capacity()

    def refused(**kw):
        rc, msg = call(**kw)
        assert rc == capi.EINVAL and msg, kw
        assert call()[0] == capi.OK                       # the engine works as before
        assert (i32["n_used"] == 1).all()
        return msg

    refused(take=0)
    refused(take=ring + 1)
    refused(max_lag_=0)
    refused(max_lag_=capi.MAX_AUTOCORR_LAG + 1)
    _d, twice = capi.as_i32([1, 1])
    refused(cols_=twice)
    _e, beyond = capi.as_i32([0, d])
    refused(cols_=beyond)
    _f, negative = capi.as_i32([-1, 0])
    refused(cols_=negative)
    refused(n_cols=0)
    refused(n_cols=d + 1)
    assert lib.mhx_get_autocorr(None, 10, cols, 2, max_lag, *outs) == capi.EINVAL
    assert lib.mhx_group_get_autocorr(None, 10, cols, 2, max_lag, *outs) == capi.EINVAL
    assert call(outs_=[None] * 8)[0] == capi.OK           # every output may be NULL
    for k in range(8):                                    # ... and each one alone
        assert call(outs_=[o if j != k else None for j, o in enumerate(outs)])[0] == capi.OK
    assert call(max_lag_=capi.MAX_AUTOCORR_LAG, outs_=[None] * 8)[0] == capi.OK
    # the one step every chain has: nothing to correlate, no halves; the fill stays where the
    # device writes nothing
    assert call()[0] == capi.OK
    assert (i32["n_used"] == 1).all() and (i32["n_lags"] == 0).all() and (i32["status"] == 6).all()
    assert np.isnan(f64["tau"]).all() and np.isnan(f64["ess"]).all() and np.isnan(f64["acf"][:, :, 0]).all()
    assert (f64["acf"][:, :, 1:] == -7.0).all() and (f64["half_mean"] == -7.0).all() and (f64["half_var"] == -7.0).all()
    # four steps in chain 1: three lags, halves of two; two in chain 2: rho_1 = -1/2 exactly, tau =
    # 0, ess = +inf, halves of one step (a variance of 0/0); chain 0 keeps its fill
    e.set_history(1, [-1.0, -2.0, -3.0, -4.0], [[1.0, 8.0], [2.0, 8.0], [4.0, 8.0], [8.0, 8.0]])
    e.set_history(2, [-1.0, -2.0], [[3.0, 5.0], [1.0, 5.0]])
    assert call()[0] == capi.OK
    assert i32["n_used"].tolist() == [1, 4, 2] and i32["n_lags"].tolist() == [0, 3, 1]
    assert i32["status"].tolist() == [[6, 6], [2, 0], [2, 4]]           # cols = [1, 0]: column 1 never moved
    assert f64["half_mean"][1].tolist() == [[8.0, 8.0], [1.5, 6.0]] and f64["half_var"][1].tolist() == [[0.0, 0.0], [0.5, 8.0]]
    assert f64["half_mean"][2].tolist() == [[5.0, 5.0], [3.0, 1.0]] and np.isnan(f64["half_var"][2]).all()
    assert f64["acf"][2, 1, :2].tolist() == [1.0, -0.5] and f64["tau"][2, 1] == 0.0 and f64["ess"][2, 1] == np.inf
    assert np.isnan(f64["tau"][2, 0]) and (f64["acf"][2, :, 2:] == -7.0).all()
    assert (f64["half_mean"][0] == -7.0).all() and (f64["acf"][0, :, 1:] == -7.0).all()
    assert (f64["acf"][1, :, 4:] == -7.0).all() and f64["acf"][1, 1, 0] == 1.0 and np.isnan(f64["acf"][1, 0, :4]).all()
    want = ac.scalar_autocorr([1.0, 2.0, 4.0, 8.0], max_lag)
    assert ac.same_bits(f64["acf"][1, 1, :4], want[0]) and f64["tau"][1, 1] == want[1] and f64["ess"][1, 1] == want[2]
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
        single, whole = ac.engine_autocorr(e, take, [2, 0], 70), ac.engine_autocorr(g, take, [2, 0], 70)
        assert ac.same(whole, single) is None, take
        assert ac.same(single, ac.want_autocorr(hc.traces(e, take), [2, 0], 70)) is None, take
    # the chains differ: their order matters
    assert len({single["tau"][c].tobytes() for c in range(n)}) > n // 2
    e.close()
    g.close()


def test_the_python_surface(mhx, d2):
    e = d2
    w, keys = as_walker(mhx, e)
    take, max_lag = 57, 30
    r = e.autocorr(take, [0, 1], max_lag, acf=True)
    assert "acf" not in e.autocorr(take, [0, 1], max_lag)
    whole = mhx.walker_set_autocorr(w, None, take, max_lag, acf=True)
    assert len(whole) == e.n_chains
    for c in range(e.n_chains):
        assert list(whole[c]) == keys
        for j, k in enumerate(keys):
            entry = whole[c][k]
            assert sorted(entry) == ["acf", "ess", "status", "tau"]
            assert ac.same_bits(np.array([entry["tau"], entry["ess"]]), np.array([r["tau"][c, j], r["ess"][c, j]]))
            assert entry["status"] == r["status"][c, j]
            assert ac.same_bits(entry["acf"], r["acf"][c, j, :r["n_lags"][c] + 1])
    for c in (0, 7, 299):
        one = mhx.walker_autocorr(w, "p1", take, max_lag, chain=c)
        assert sorted(one) == ["ess", "status", "tau"]
        assert ac.same_bits(np.array([one["tau"], one["ess"]]), np.array([r["tau"][c, 1], r["ess"][c, 1]]))
    assert list(mhx.walker_set_autocorr(w, ["p1"], take, max_lag)[5]) == ["p1"]
    # the crafted walks differ in length: their windows of 57 steps are not comparable ...
    with pytest.raises(ValueError, match="chain"):
        mhx.walker_set_rhat(w, None, take)
    # ... the newest 4 steps of the walks that have them are
    want = ac.want_autocorr(windows_of(e, take), [0, 1], 1)
    long_enough = np.flatnonzero(want["n_used"] == take)
    assert len(long_enough) > 200
    rhat = mhx.split_rhat(want["half_mean"][long_enough], want["half_var"][long_enough], want["n_used"][long_enough])
    assert rhat.shape == (2,) and np.isfinite(rhat).all()
    assert ac.same_bits(rhat, mhx.split_rhat(r["half_mean"][long_enough], r["half_var"][long_enough],
                                             r["n_used"][long_enough]))


def test_a_real_short_walk(mhx):
    """16 chains of the line fit, 600 steps each from nearby starts: walker_set_rhat is split_rhat
    of the yardstick's half moments, every tau and every rhat is finite"""
    e = hc.line_engine(mhx, 16, seed=11)
    e.init_chains(np.array([-1.0, 2.0]) + 0.01 * np.arange(16)[:, None])
    e.many_steps(600, np.diag([0.05, 0.05]))
    w, keys = as_walker(mhx, e)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # nothing reaches past the ring
        whole = mhx.walker_set_autocorr(w, None, 500, 255)
        rhat = mhx.walker_set_rhat(w, None, 500)
    assert all(np.isfinite(whole[c][k]["tau"]) and whole[c][k]["tau"] > 1.0 for c in range(16) for k in keys)
    want = ac.want_autocorr(hc.traces(e, 500), [0, 1], 1)
    assert (want["n_used"] == 500).all()
    yard = mhx.split_rhat(want["half_mean"], want["half_var"], want["n_used"])
    assert list(rhat) == keys and ac.same_bits(np.array([rhat[k] for k in keys]), yard)
    assert np.isfinite(yard).all() and (yard > 0.9).all()
    print("tau", [round(whole[0][k]["tau"], 2) for k in keys], "rhat", yard)
    # a window longer than the ring warns as walker_set_get does
    e.many_steps(600, np.diag([0.05, 0.05]))
    with pytest.warns(mhx.walker.HistoryTruncated):
        mhx.walker_set_rhat(w, None, 2000)
    e.close()
