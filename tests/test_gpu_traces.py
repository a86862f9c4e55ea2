"""Every chain's steps, filtered and thinned on the device (mhx_get_traces, Engine.traces,
Group.traces, walker_set_get's list selectors, walker_set_trace, walker_set_catepillar; walker-get
mcmc-fitting.lisp:490-510 and 540, thin 149-157).  The yardstick is tests/traces_cases.py: each
chain's own e.trace(c, take) and numpy / plain Python; every comparison is bit for bit and covers
ALL chains of its engine."""
import warnings

import numpy as np
import pytest

import histo_cases as hc
import problems as pb
import traces_cases as tc

pytestmark = pytest.mark.gpu
PROB = tc.PROB


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


@pytest.fixture(scope="module")
def d2(mhx):
    e = hc.crafted_d2(mhx)
    yield e
    e.close()


def check(e, y, take, cols, filt, stride, start, envelope, max_out=None):
    got = e.traces(take, cols, filter=filt, stride=stride, start=start, max_out=max_out, envelope=envelope)
    want = y.want(take, cols, filt, stride, start, max_out, envelope)
    assert tc.differences(got, want) == [], (take, cols, filt, stride, start, envelope, max_out)
    assert tc.rows_beyond_are_zero(got)
    return got


STRIDES = ((1, 0), (2, 0), (2, 1), (3, 2), (64, 0), (65, 64), (2048, 0), (2048, 2047))


@pytest.mark.parametrize("take", (1, 2, 64, 65, 1000, 2048))
def test_crafted_walks_every_filter_stride_and_column_list(mhx, d2, take):
    """300 chains, d = 2, walks of 1 to 2048 steps: all three filters, strides from 1 to the ring
    with first and last starts, three column lists, with and without the envelope, max_out = all
    the rows there can be.  The inputs exercise the rules, which is asserted."""
    e, y = d2, tc.Yardstick(d2)
    length = e.state()["length"]
    seen = {"dropped": 0, "partial": 0, "empty": 0}
    for filt in tc.FILTERS:
        for stride, start in STRIDES:
            for cols in ([PROB, 0, 1], [1], [PROB]):
                for envelope in (False, True):
                    r = check(e, y, take, cols, filt, stride, start, envelope)
                    assert r["values"].shape == (300, mhx.trace_rows(take, stride, start) or 1, len(cols))
            y._buckets.clear()
            assert np.array_equal(r["n_used"], np.minimum(length, take))
            one = r["n_used"] == 1
            assert one.any()
            if filt == "unique":
                seen["dropped"] += int((r["n_kept"] < r["n_used"]).sum())
                assert (r["n_kept"][one] == 1).all() and (r["n_kept"] >= 1).all()
            elif filt == "forward":
                assert (r["n_kept"][one] == 0).all() and (r["n_kept"] < r["n_used"]).all()
            else:
                assert np.array_equal(r["n_kept"], r["n_used"])
            seen["partial"] += int(((r["n_kept"] > start) & ((r["n_kept"] - start) % stride != 0)).sum())
            seen["empty"] += int((r["n_out"] == 0).sum())
            assert ((r["n_out"] == 0) == (r["n_kept"] <= start)).all()
    assert seen["empty"] > 0                          # start >= n_kept somewhere
    if take > 1:
        assert seen["dropped"] > 0 and seen["partial"] > 0


def test_max_out_below_the_row_count(mhx, d2):
    e, y = d2, tc.Yardstick(d2)
    for filt in tc.FILTERS:
        full = e.traces(2048, [PROB, 0, 1], filter=filt, envelope=True)
        assert full["n_out"].max() > 7
        r = check(e, y, 2048, [PROB, 0, 1], filt, 1, 0, True, max_out=7)
        assert r["values"].shape == (300, 7, 3)
        assert np.array_equal(r["n_out"], np.minimum(full["n_out"], 7)) and (r["n_out"] == 7).any()
        assert np.array_equal(r["n_kept"], full["n_kept"]) and np.array_equal(r["n_used"], full["n_used"])
        for k in ("values", "lo", "hi"):
            assert np.array_equal(r[k].view(np.uint64), full[k][:, :7].view(np.uint64)), (filt, k)


def test_wide_vector_columns_out_of_order_and_twice(mhx):
    e = hc.crafted_d33(mhx)
    y = tc.Yardstick(e)
    for take in (57, 2048):
        for stride, start in ((1, 0), (5, 0), (5, 3)):
            for filt in tc.FILTERS:
                r = check(e, y, take, [32, PROB, 0, 7, 7], filt, stride, start, True)
                assert np.array_equal(r["values"][:, :, 3].view(np.uint64), r["values"][:, :, 4].view(np.uint64))
    e.close()


def nan_with_payload(payload):
    return np.array([0x7FF8000000000000 | payload], dtype=np.uint64).view(np.float64)[0]


def test_values_that_are_not_finite(mhx):
    """4 chains of 40 steps.  With stride 4 and start 0 under :steps, bucket r is steps 4r .. 4r+3:
    chain 1's column 0 has a NaN first in bucket 2 (it stays), a NaN inside bucket 3 (ignored),
    -0.0 before +0.0 in buckets 4 and 6 and the reverse in 5 and 7 (the earlier zero stays, as lo
    among positive and as hi among negative values), and both infinities.  Chain 2's prob has a
    NaN repeated with the same bits (one step, not two, is unique), a NaN next to a NaN of another
    payload (both unique), -0.0 next to +0.0 (unique by bits, not forward) and both infinities."""
    rng = np.random.default_rng(40)
    e = hc.line_engine(mhx, 4, history_capacity=64)
    e.init_chains([-1.0, 2.0])
    prob = [rng.normal(-5.0, 1.0, 40) for _ in range(4)]
    walks = [rng.normal(0.0, 2.0, (40, 2)) for _ in range(4)]
    a, b = nan_with_payload(1), nan_with_payload(2)
    col = walks[1][:, 0]
    col[8], col[13] = a, b
    col[16:20] = -0.0, 0.0, 1.0, 2.0
    col[20:24] = 0.0, -0.0, 1.0, 2.0
    col[24:28] = -0.0, 0.0, -1.0, -2.0
    col[28:32] = 0.0, -0.0, -1.0, -2.0
    col[33], col[38] = np.inf, -np.inf
    walks[3][5, 1], walks[3][6, 1] = -np.inf, a
    p = prob[2]
    p[5], p[6] = a, a
    p[10], p[11] = a, b
    p[20], p[21] = -0.0, 0.0
    p[30], p[31], p[39] = np.inf, -np.inf, b
    prob[3][0], prob[3][1] = b, np.inf
    for c in range(4):
        e.set_history(c, prob[c], walks[c])
    y = tc.Yardstick(e)
    for filt in tc.FILTERS:
        for stride, start in ((1, 0), (4, 0), (4, 3), (7, 2), (40, 0)):
            r = check(e, y, 40, [PROB, 0, 1], filt, stride, start, True)
            if filt == "steps" and (stride, start) == (4, 0):
                lo, hi, first = r["lo"][1, :, 1], r["hi"][1, :, 1], r["values"][1, :, 1]
                bits = lambda v: np.asarray(v).view(np.uint64)
                assert bits(lo[2]) == bits(hi[2]) == bits(a)                       # a first NaN stays
                assert lo[3] == col[12:16][[0, 2, 3]].min() and hi[3] == col[12:16][[0, 2, 3]].max()
                assert lo[4] == 0 and np.signbit(lo[4]) and lo[5] == 0 and not np.signbit(lo[5])
                assert hi[6] == 0 and np.signbit(hi[6]) and hi[7] == 0 and not np.signbit(hi[7])
                assert hi[8] == np.inf and lo[9] == -np.inf
                assert np.array_equal(bits(first), bits(col[0::4]))
            if (stride, start) == (1, 0):
                for k in ("lo", "hi"):
                    assert np.array_equal(r[k].view(np.uint64), r["values"].view(np.uint64))
                kept = set(np.flatnonzero(np.isin(np.arange(40), y.kept(40, filt)[2])).tolist())
                if filt == "unique":
                    assert 5 not in kept and 6 in kept and {10, 11, 20, 21, 39} <= kept
                if filt == "forward":       # a NaN on either side keeps the step; -0.0 <= +0.0
                    assert {5, 6, 10, 11, 30} <= kept and 20 not in kept and 39 not in kept
    e.close()


def test_the_ring_as_the_walk_leaves_it(mhx):
    """a ring that has wrapped, then one whose walk :burn-walks has cut below what the ring holds,
    then a chain restored from more steps than the ring's capacity.  (mhx_set_history keeps the
    newest history_capacity steps and sets walker-length to that number, so n_used equals
    min(take, length) there too: the wrapped ring is what puts the window across the ring's end.)"""
    e = hc.line_engine(mhx, 8, seed=5)
    e.init_chains(np.array([-1.0, 2.0]) + 0.01 * np.arange(8)[:, None])
    assert e.history_capacity() == 1024
    e.many_steps(1500, np.diag([0.05, 0.05]))
    assert (e.state()["length"] > 1024).all()

    def sweep(takes, used):
        y = tc.Yardstick(e)
        for take in takes:
            for filt in tc.FILTERS:
                for stride, start in ((1, 0), (16, 5)):
                    r = check(e, y, take, [PROB, 0, 1], filt, stride, start, True)
                    assert r["n_used"].tolist() == used(take)
        return r

    sweep((1000, 1024), lambda take: [take] * 8)
    e.modify("burn-walks", 900)      # walker_modify's :burn-walks
    left = e.state()["length"]
    assert (left == 601).all()
    sweep((1000, 1024), lambda take: [601] * 8)
    rng = np.random.default_rng(1500)
    e.set_history(3, *hc.crafted_walk(rng, 1500, 2, 0))
    assert e.state()["age"][3] == 1500 and e.state()["length"][3] == 1024
    sweep((1000, 1024), lambda take: [601] * 3 + [take] + [601] * 4)
    e.close()


def test_chains_beyond_one_portion(mhx):
    """d = 33, all 34 columns, envelope, ring 2048, take = max_out = 2048: a chain's pieces are
    three arrays of 2048 x 34 doubles, three counts and 2048 kept indices, 1679372 bytes, so 39
    chains fill the 64 MiB of a portion (the column list, 136 bytes, is carved once) and 100
    chains are worked through in three."""
    rng = np.random.default_rng(39)
    d, n, ring = 33, 100, 2048
    per_chain = 3 * 8 * ring * (d + 1) + 3 * 4 + 4 * ring
    assert per_chain == 1679372 and ((1 << 26) - 4 * (d + 1) - 8 * 256) // per_chain == 39
    e = hc.line_engine(mhx, n, d=d, used=range(0, 32, 4), history_capacity=ring)
    e.init_chains(np.linspace(-1.0, 2.0, d))
    lengths = [ring, 1, 700] + list(rng.integers(1, 60, n - 3))
    lengths[38:41] = [ring, 900, ring]
    lengths[77:79] = [ring, ring]
    hc.inject(e, rng, lengths)
    cols = [PROB] + list(range(d))
    y = tc.Yardstick(e)
    for filt in ("unique", "steps"):
        got = e.traces(ring, cols, filter=filt, max_out=ring, envelope=True)
        want = y.want(ring, cols, filt, 1, 0, ring, True)
        for c in (0, 1, 38, 39, 40, 77, 78, 79, 99):      # first, last, either side of both boundaries
            assert tc.differences({k: v[c] for k, v in got.items()}, {k: v[c] for k, v in want.items()}) == [], c
        assert tc.differences(got, want) == [] and tc.rows_beyond_are_zero(got)
    assert np.array_equal(got["n_used"], lengths)
    e.close()


def test_arguments_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    n, d = 3, 2
    e = hc.line_engine(mhx, n)
    _c, cols = capi.as_i32([PROB, 1, 1])
    arrays = [np.full((n, 4, 3), -7.0) for _ in range(3)] + [np.full(n, -7, dtype=np.int32) for _ in range(3)]
    outs = [a.ctypes.data_as(capi.f64p) for a in arrays[:3]] + [a.ctypes.data_as(capi.i32p) for a in arrays[3:]]

    def call(take=10, filt=capi.TRACE_STEPS, stride=1, start=0, cols_=cols, n_cols=3, max_out=4, outs_=outs):
        rc = lib.mhx_get_traces(e._h, take, filt, stride, start, cols_, n_cols, max_out, *outs_)
        return rc, lib.mhx_last_error().decode()

    assert call()[0] == capi.ESTATE                       # before mhx_init_chains
    e.init_chains([-1.0, 2.0])
    ring = e.history_capacity()

    def refused(word, **kw):
        rc, msg = call(**kw)
        assert rc == capi.EINVAL and word in msg, (kw, msg)
        assert call()[0] == capi.OK                       # the engine works as before
        assert (arrays[5] == 1).all()
        return msg

    refused("take", take=0)
    refused("take", take=ring + 1)
    refused("filter", filt=-1)
    refused("filter", filt=3)
    refused("stride", stride=0)
    refused("stride", stride=ring + 1)
    refused("start", start=-1)
    refused("start", stride=3, start=3)
    refused("n_cols", n_cols=0)
    refused("cols is NULL", cols_=None)
    _d, below = capi.as_i32([PROB, -2, 0])
    refused("cols[1]", cols_=below)
    _e, beyond = capi.as_i32([0, 1, d])
    refused("cols[2]", cols_=beyond)
    refused("max_out", max_out=0)
    refused("max_out", max_out=ring + 1)
    assert call(stride=ring, start=ring - 1, max_out=ring, outs_=[None] * 6)[0] == capi.OK
    for k in range(6):                                    # every output may be NULL, each alone too
        assert call(outs_=[None if j == k else o for j, o in enumerate(outs)])[0] == capi.OK
        assert call(outs_=[o if j == k else None for j, o in enumerate(outs)])[0] == capi.OK
    assert lib.mhx_group_get_traces(None, 10, 0, 1, 0, cols, 3, 4, *outs) == capi.EINVAL
    # the one step every chain has: prob, then theta[1] = 2 twice; rows 1 .. 3 are zero
    assert call()[0] == capi.OK
    values, lo, hi, n_out, n_kept, n_used = arrays
    assert (n_out == 1).all() and (n_kept == 1).all() and (n_used == 1).all()
    assert (values[:, 0, 1:] == 2.0).all() and np.array_equal(values[:, 0, 0], e.state()["logpost"])
    assert np.array_equal(lo, values) and np.array_equal(hi, values) and not values[:, 1:].any()
    e.close()


def test_group_equals_a_single_engine(mhx):
    rng = np.random.default_rng(49)
    n, d = 49, 3
    e = hc.line_engine(mhx, n, d=d, used=(0, 2), history_capacity=256)
    g = mhx.Group(n, d, 1, devices=[0, 0, 0], history_capacity=256)
    g.set_function(0, mhx.capi.MODEL_POLY, (), [0, 2])
    g.set_dataset(0, hc.LF_X, hc.LF_Y, np.full(5, 0.2))
    for obj in (e, g):
        obj.init_chains([-1.0, 0.5, 2.0])
    assert g.ranges == [(0, 17), (17, 16), (33, 16)]
    walks = [hc.crafted_walk(rng, int(rng.integers(1, 257)), d, c % 3) for c in range(n)]
    for part, (first, count) in zip([e] + g.engines, [(0, n)] + g.ranges):
        for c in range(count):
            part.set_history(c, *walks[first + c])
    y = tc.Yardstick(e)
    for take in (1, 100, 256):
        for filt in tc.FILTERS:
            for stride, start in ((1, 0), (7, 3)):
                single = check(e, y, take, [2, PROB, 0], filt, stride, start, True)
                whole = g.traces(take, [2, PROB, 0], filter=filt, stride=stride, start=start, envelope=True)
                assert tc.differences(whole, single) == [], (take, filt, stride)
    e.close()
    g.close()


KEYS = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]
SELECTORS = (":steps", ":params", ":param", ":log-liklihoods", ":unique-steps", ":forward-steps")


def plain(v):
    """a walker_get result as plain data: WalkerSteps become (prob, params)"""
    if isinstance(v, list):
        return [plain(x) for x in v]
    return (v.prob, v.params) if hasattr(v, "prob") else v


@pytest.fixture(scope="module")
def walked(mhx):
    s = pb.two_peak(n=700, seed=12)
    x, y, sig, _ = s.data[0]
    idx, lo, hi = s.bounds[0]
    params = []
    for k, v in zip(KEYS, s.theta_star):
        params += [":" + k, float(v)]
    w = mhx.walker_create(
        function=mhx.models.gauss_peaks(KEYS[:2], [tuple(KEYS[2:5]), tuple(KEYS[5:8])]),
        data=[x, y], params=params, data_error=sig,
        log_prior=mhx.prior_bounds({KEYS[i]: (lo[i], hi[i]) for i in idx}),
        n_chains=11, theta0=pb.perturbed(s.theta_star, 11, 0.01, seed=5), seed=41)
    mhx.walker_adaptive_steps(w, 3000)
    yield w
    w.engine.close()


def test_walker_set_get_is_walker_get_of_every_chain(mhx, walked):
    w = walked
    e = w.engine
    ring = e.history_capacity()
    length = e.state()["length"]
    assert (length > ring).any()
    for get in SELECTORS:
        for take in (None, 5, 1000, 5000):
            past = take is None or take > ring
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                got = mhx.walker_set_get(w, get, take, param=":mu1")
            assert len([x for x in caught if issubclass(x.category, mhx.walker.HistoryTruncated)]) == int(past)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = [mhx.walker_get(w, get, take, param=":mu1", chain=c) for c in range(e.n_chains)]
            assert plain(got) == plain(want), (get, take)
            assert len(got) == 11
            if get not in (":unique-steps", ":forward-steps"):
                held = np.minimum(length if take is None else np.minimum(take, length), ring)
                assert [len(v) for v in got] == held.tolist()


def test_walker_set_get_reads_no_trace_per_chain(mhx, walked, monkeypatch):
    w = walked
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = {get: plain(mhx.walker_set_get(w, get, 300, param=":w2")) for get in SELECTORS}

    def no_trace(self, chain, take):
        raise AssertionError("walker_set_get read the trace of chain %d" % chain)

    monkeypatch.setattr(mhx.Engine, "trace", no_trace)
    for get in SELECTORS:
        assert plain(mhx.walker_set_get(w, get, 300, param=":w2")) == want[get]
    with pytest.raises(KeyError):       # as walker_get: the first step's plist has no such key
        mhx.walker_set_get(w, ":param", 300, param=":nope")


def test_walker_set_trace_and_catepillar(mhx, walked):
    w = walked
    e = w.engine
    y = tc.Yardstick(e)
    keys = list(w.param_keys)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = mhx.walker_set_trace(w, [":mu1"], take=700, thin=3, start=1, which=":unique-steps", envelope=True)
        cat = mhx.walker_set_catepillar(w, take=1000, points=50)
        every = mhx.walker_set_catepillar(w, take=200)
    want = y.want(700, [PROB, keys.index("mu1")], "unique", 3, 1, None, True)
    for k in ("n_out", "n_kept", "n_used"):
        assert np.array_equal(r[k], want[k])
    bits = lambda v: np.ascontiguousarray(v).view(np.uint64)
    for name, side in (("values", "values"), ("lo", "lo"), ("hi", "hi")):
        assert list(r[name]) == ["mu1"] and np.array_equal(bits(r[name]["mu1"]), bits(want[side][:, :, 1]))
    assert np.array_equal(bits(r["prob"]), bits(want["values"][:, :, 0]))
    assert np.array_equal(bits(r["prob_lo"]), bits(want["lo"][:, :, 0]))
    assert (r["n_kept"] < r["n_used"]).any()
    # 1000 steps on 50 points: buckets of 20
    assert cat["stride"] == 20 and list(cat["params"]) == keys
    want = y.want(1000, [PROB] + list(range(8)), "steps", 20, 0, None, True)
    assert np.array_equal(cat["n_out"], want["n_out"]) and (cat["n_out"] == 50).all()
    for name, side in (("first", "values"), ("lo", "lo"), ("hi", "hi")):
        assert np.array_equal(bits(cat["log_liklihoods"][name]), bits(want[side][:, :, 0]))
        for j, k in enumerate(keys):
            assert np.array_equal(bits(cat["params"][k][name]), bits(want[side][:, :, 1 + j]))
    assert (cat["params"]["mu1"]["lo"] < cat["params"]["mu1"]["hi"]).any()
    want = y.want(200, [PROB, 0, 1], "steps", 1, 0, None, False)
    assert every["stride"] == 1 and list(every["params"]["b0"]) == ["first"]
    assert np.array_equal(bits(every["params"]["b1"]["first"]), bits(want["values"][:, :, 2]))
    assert np.array_equal(bits(every["log_liklihoods"]["first"]), bits(want["values"][:, :, 0]))
