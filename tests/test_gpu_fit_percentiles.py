"""mhx_get_fit_percentiles: the pointwise posterior of the fit curve of every chain, on the device.

The yardstick is the device's own e.trace + e.eval_function and numpy on the host:
  percentiles  a stable sort per column (numpy puts a NaN last, whatever its sign) and
               mhx_percentile_rank; compared bit for bit, except where the picked element is a
               zero (-0 and +0 are one number: either may be returned) - there by value - and where
               it is a NaN (any NaN)
  moments      the definition's Welford recurrence written with separate numpy operations (numpy
               fuses nothing), compared bit for bit; a chain with a value that is not finite, whose
               moments are "whatever IEEE gives", up to the NaN's payload
Every test fails on a library without the symbol."""
import ctypes as C

import numpy as np
import pytest

import problems as pb

pytestmark = pytest.mark.gpu

LF_X, LF_Y = [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0]
TWO_PEAK = ("(lambda (x &key b0 b1 a1 mu1 w1 a2 mu2 w2 &allow-other-keys)"
            " (+ (+ b0 (* b1 x))"
            "    (* a1 (exp (- (expt (/ (- x mu1) w1) 2))))"
            "    (* a2 (exp (- (expt (/ (- x mu2) w2) 2))))))")
KEYS8 = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]
PCTS = [(0, 1), (5, 2), (50, 1), (841, 10), (195, 2), (100, 1)]     # 0, 2.5, 50, 84.1, 97.5, 100
B = 1 << 26                                                          # kStageBudget (mhx_stage.hpp)


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


# ---- the yardstick -----------------------------------------------------------------------------
def rank(mhx, n, num, den):
    pos, between = C.c_int64(0), C.c_int32(0)
    mhx.capi.check(mhx.capi.lib().mhx_percentile_rank(int(n), int(num), int(den), C.byref(pos), C.byref(between)))
    return pos.value, bool(between.value)


def welford(vals, stops):
    """{n: (mean, M2)} after the n newest rows of vals [len, m], for every n in stops: the
    definition's recurrence, one numpy operation per IEEE operation"""
    m = vals.shape[1]
    mean, m2, out = np.zeros(m), np.zeros(m), {}
    if 0 in stops:
        out[0] = (mean.copy(), m2.copy())
    with np.errstate(all="ignore"):
        for s in range(max(stops)):
            v = vals[s]
            qk = 1.0 / float(s + 1)
            delta = v - mean
            mean = mean + delta * qk
            m2 = m2 + delta * (v - mean)
            if s + 1 in stops:
                out[s + 1] = (mean, m2)
    return out


def host_percentiles(mhx, vals, pcts):
    """[len(pcts), m] nth-percentile of the columns of vals [n, m]"""
    n = vals.shape[0]
    e = np.sort(vals, axis=0, kind="stable")
    out = np.empty((len(pcts), vals.shape[1]))
    with np.errstate(all="ignore"):
        for q, (num, den) in enumerate(pcts):
            pos, between = rank(mhx, n, num, den)
            out[q] = (e[pos] + e[pos + 1]) / 2.0 if between else e[pos]
    return out


def same(got, want, what):
    """bit for bit; a zero by value; a NaN for a NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    ok = (got.view(np.uint64) == want.view(np.uint64)) | ((want == 0.0) & (got == 0.0)) | \
        (np.isnan(want) & np.isnan(got))
    assert ok.all(), (what, np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])


def bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes(), what


class Yardstick:
    """the values of every chain's whole ring at xs, evaluated once and shared by the takes"""

    def __init__(self, mhx, e, fn, xs, chains=None, takes=()):
        self.mhx, self.e, self.takes = mhx, e, tuple(takes)
        ring = e.history_capacity()
        self.chains = list(range(e.n_chains) if chains is None else chains)
        self.lengths = e.state()["length"]
        th = [e.trace(c, ring)[1] for c in self.chains]
        held = [len(t) for t in th]
        every = e.eval_function(fn, np.concatenate(th), xs) if sum(held) else np.zeros((0, 0))
        ends = np.cumsum([0] + held)
        self.vals = {c: every[ends[i]:ends[i + 1]] for i, c in enumerate(self.chains)}
        self.moments = {}

    def window(self, c, take):
        return min(int(take), int(self.lengths[c]), len(self.vals[c]))

    def check(self, take, got, pcts=PCTS, what=""):
        pct, mean, sd, used, status = got
        capi = self.mhx.capi
        for c in self.chains:
            n, v = self.window(c, take), self.vals[c]
            assert used[c] == n, (what, take, c, used[c], n)
            finite = bool(np.isfinite(v[:n]).all())
            want_status = (0 if finite else capi.FITPCT_NONFINITE) | (capi.FITPCT_ONE_STEP if n == 1 else 0) | \
                (capi.FITPCT_EMPTY if n == 0 else 0)
            assert status[c] == want_status, (what, take, c, status[c], want_status)
            if n == 0:
                continue
            if (c, n) not in self.moments:      # (one pass serves every take: the recurrence's prefixes)
                stops = {n} | {self.window(c, t) for t in self.takes}
                self.moments.update({(c, k): mm for k, mm in welford(v, stops - {0}).items()})
            m1, m2 = self.moments[c, n]
            with np.errstate(all="ignore"):
                want_sd = np.sqrt(m2 / float(n - 1))
            if finite:
                bits(mean[c], m1, (what, "mean", take, c))
                if n == 1:
                    assert np.isnan(sd[c]).all(), (what, take, c)
                else:
                    bits(sd[c], want_sd, (what, "stddev", take, c))
            else:
                same(mean[c], m1, (what, "mean", take, c))
                same(sd[c], want_sd, (what, "stddev", take, c))
            same(pct[c], host_percentiles(self.mhx, v[:n], pcts), (what, "pct", take, c))


def line_engine(mhx, n_chains, **kw):
    e = mhx.Engine(n_chains, 2, 1, **kw)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    e.set_dataset(0, LF_X, LF_Y, np.full(5, 0.2))
    return e


def crafted(rng, n, d, centre, spread):
    """a Metropolis-like walk, newest first: runs of repeated steps"""
    prob, theta = np.empty(n), np.empty((n, d))
    p, th = 0.0, centre.copy()
    for i in range(n):
        if i == 0 or rng.random() < 0.4:
            p = rng.normal(-50.0, 3.0)
            th = centre * (1.0 + spread * rng.standard_normal(d))
        prob[i], theta[i] = p, th
    return prob[::-1].copy(), theta[::-1].copy()


LINE = np.array([-1.0, 2.0])


def crafted_line_engine(mhx, lengths, seed=1, ring=1024):
    rng = np.random.default_rng(seed)
    e = line_engine(mhx, len(lengths), history_capacity=ring)
    e.init_chains(LINE)
    for c, n in enumerate(lengths):
        e.set_history(c, *crafted(rng, n, 2, LINE, 0.3))
    return e


# ---- 1. crafted line histories -----------------------------------------------------------------
def test_crafted_line_histories(mhx):
    lengths = [1, 2, 3, 9, 64, 65, 150, 151, 1000, 1023, 1024, 300]
    e = crafted_line_engine(mhx, lengths)
    blk = mhx.capi.FITPCT_BLOCK
    for m in (1, 63, 64, 65, blk - 1, blk, blk + 1, 1000):
        xs = np.linspace(-4.0, 10.0, m) if m > 1 else np.array([2.5])
        takes = (1, 2, 3, 64, 65, 1000, 1024)
        y = Yardstick(mhx, e, 0, xs, takes=takes)
        for take in takes:
            got = e.fit_percentiles(0, take, xs, PCTS)
            assert got[0].shape == (len(lengths), len(PCTS), m) and got[1].shape == (len(lengths), m)
            y.check(take, got, what="m %d" % m)
            pct, _, sd, used, status = got
            assert list(used) == [min(take, n) for n in lengths]
            for c, n in enumerate(lengths):     # the ONE_STEP bit and its NaN standard deviation
                assert bool(status[c] & mhx.capi.FITPCT_ONE_STEP) == (min(take, n) == 1)
                assert np.isnan(sd[c]).all() == (min(take, n) == 1)
            assert (pct[:, 0] <= pct[:, 2]).all() and (pct[:, 2] <= pct[:, 5]).all()
    # the dataset's own x
    own = e.fit_percentiles(0, 150)
    assert own[0].shape == (len(lengths), 3, 5)
    for a, b in zip(own, e.fit_percentiles(0, 150, np.array(LF_X))):
        bits(a, b, "own x")
    e.close()


# ---- 2. ties and specials ----------------------------------------------------------------------
def ties_engine(mhx, bad):
    """chain 0: ten steps whose values tie in runs; chain 1: +0 and -0; chain 2: a NaN parameter
    and a step that overflows (bad) or a plain walk; chain 3: a plain walk"""
    e = line_engine(mhx, 4, history_capacity=64)
    e.init_chains(LINE)
    b0 = np.array([3.0, 1.0, 2.0, 3.0, 1.0, 5.0, 3.0, 2.0, 1.0, 3.0])      # sorted: 1 1 1 2 2 3 3 3 3 5
    e.set_history(0, -np.arange(10.0), np.column_stack([b0, np.zeros(10)]))
    z = np.array([[0.0, 0.0], [-0.0, -0.0], [1.0, 0.0], [-1.0, -0.0], [0.0, 0.0], [-0.0, -0.0]])
    e.set_history(1, -np.arange(6.0), z)
    rng = np.random.default_rng(5)
    pr, th = crafted(rng, 40, 2, LINE, 0.3)
    if bad:
        th[7] = [np.nan, 1.0]
        th[21] = [1e308, 1e308]          # b + m x overflows for x > 0
        th[22] = [-1e308, -1e308]
    e.set_history(2, pr, th)
    e.set_history(3, *crafted(rng, 33, 2, LINE, 0.3))
    return e


def test_ties_and_specials(mhx):
    xs = np.linspace(1.0, 9.5, 70)
    e, plain = ties_engine(mhx, True), ties_engine(mhx, False)
    y = Yardstick(mhx, e, 0, xs)
    # ranks at and across the runs of chain 0 (n = 10): pos = k exactly, and k + 1/2 (between)
    at = [(100 * k, 9) for k in range(10)]
    across = [((2 * k + 1) * 50, 9) for k in range(9)]
    for k in range(10):
        assert rank(mhx, 10, *at[k]) == (k, False)
    for k in range(9):
        assert rank(mhx, 10, *across[k]) == (k, True)
    for pcts in (at, across, PCTS):
        for take in (10, 64, 6, 5):
            got = e.fit_percentiles(0, take, xs, pcts)
            y.check(take, got, pcts, what="ties")
            other = plain.fit_percentiles(0, take, xs, pcts)
            # the bad chain is flagged alone, and nobody else's bits know of it
            assert [int(s) & 1 for s in got[4]] == [0, 0, 1 if take > 7 else 0, 0], take
            for c in (0, 1, 3):
                for a, b in zip(got, other):
                    bits(a[c], b[c], ("beside the bad chain", take, c))
    got = e.fit_percentiles(0, 10, xs, at + across[:4])
    sorted0 = [1, 1, 1, 2, 2, 3, 3, 3, 3, 5]
    for k in range(10):
        assert (got[0][0, k] == sorted0[k]).all()
    for k in range(4):
        assert (got[0][0, 10 + k] == (sorted0[k] + sorted0[k + 1]) / 2.0).all()
    # chain 1 holds both zeros and they are one number: the percentiles are zeros wherever the
    # sorted column has them (-1 < 0 0 0 0 < 1), of either sign
    col = e.eval_function(0, e.trace(1, 64)[1], xs)
    assert (col == 0.0).sum() == 4 * len(xs)
    print("zeros of chain 1: %d negative, %d positive" % (np.signbit(col[col == 0.0]).sum(),
                                                         (~np.signbit(col[col == 0.0])).sum()))
    z = e.fit_percentiles(0, 6, xs, [(20, 1), (40, 1), (50, 1), (60, 1), (80, 1)])[0][1]
    assert (z == 0.0).all()
    # NaN last: the greatest element of the bad chain's window is its NaN, the least its -inf
    top = e.fit_percentiles(0, 40, xs, [(0, 1), (100, 1), (50, 1)])[0][2]
    assert np.isnan(top[1]).all() and np.isneginf(top[0]).all() and np.isfinite(top[2]).all()
    e.close()
    plain.close()


# ---- 3. both selection paths -------------------------------------------------------------------
def test_keys_in_lds_and_keys_from_the_stage_give_the_same_bits(mhx, monkeypatch):
    lengths = [1, 2, 9, 65, 300, 1000, 1024]
    xs = np.linspace(-4.0, 10.0, 131)
    takes = (1, 3, 65, 1000, 1024)
    # the keys from LDS or from the stage; a column's percentiles in shared passes or one by one;
    # the staged values with a step's points or a point's steps side by side
    knobs = ("MHX_FITPCT_NO_LDS", "MHX_FITPCT_SELECT_SINGLY", "MHX_FITPCT_STEP_FASTEST")
    runs = {}
    for on in ((), (0,), (1,), (0, 1), (2,), (0, 2), (0, 1, 2)):
        for k, name in enumerate(knobs):                     # (read when the problem is finalised)
            monkeypatch.setenv(name, "1" if k in on else "0")
        e = crafted_line_engine(mhx, lengths, seed=3)
        runs[on] = [e.fit_percentiles(0, take, xs, PCTS + [(100, 3), (200, 3), (1, 7)]) for take in takes]
        if on in ((0,), (0, 1, 2)):
            y = Yardstick(mhx, e, 0, xs, takes=takes)
            for take, got in zip(takes, runs[on]):
                y.check(take, got, PCTS + [(100, 3), (200, 3), (1, 7)], what="knobs %r" % (on,))
        e.close()
    for on, other in runs.items():
        for a, b in zip(runs[()], other):
            for u, v in zip(a, b):
                bits(u, v, ("the default against knobs", on))


def test_a_window_too_long_for_lds_takes_the_memory_path_by_itself(mhx):
    ring = 32768
    rng = np.random.default_rng(8)
    e = mhx.Engine(2, 3, 1, history_capacity=ring)
    e.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1, 2])
    e.set_dataset(0, LF_X, LF_Y, np.full(5, 0.2))
    centre = np.array([-1.0, 2.0, 0.1])
    e.init_chains(centre)
    for c, n in enumerate((ring, 20001)):
        e.set_history(c, *crafted(rng, n, 3, centre, 0.3))
    assert e.history_capacity() == ring
    xs = np.linspace(-4.0, 10.0, 65)
    y = Yardstick(mhx, e, 0, xs)
    y.check(ring, e.fit_percentiles(0, ring, xs, PCTS), what="ring 32768")
    e.close()


# ---- 4. every kernel home ----------------------------------------------------------------------
def two_peak_engine(mhx, seed=2):
    s = pb.two_peak(n=2000, seed=5)
    rng = np.random.default_rng(seed)
    lengths = [5, 150, 700, 1024, 3000, 1]
    e = s.engine(mhx, len(lengths), history_capacity=1024)
    e.init_chains(s.theta_star)
    for c, n in enumerate(lengths):
        e.set_history(c, *crafted(rng, n, 8, s.theta_star, 0.02))
    return e


def check_takes(mhx, e, fn, xs, takes, what):
    y = Yardstick(mhx, e, fn, xs, takes=takes)
    for take in takes:
        y.check(take, e.fit_percentiles(fn, take, xs, PCTS), what=what)


def test_the_two_peak_kernel_and_the_generic_one(mhx, monkeypatch):
    xs = mhx.fit_linspace(0.0, 1.0)
    e = two_peak_engine(mhx)
    assert "gauss22_normal" in e.kernel_name()
    check_takes(mhx, e, 0, xs, (1, 150, 1000, 1024), "two-peak")
    aot = e.fit_percentiles(0, 1000, xs, PCTS)
    e.close()
    monkeypatch.setenv("MHX_FORCE_GENERIC", "1")
    g = two_peak_engine(mhx)
    assert "generic" in g.kernel_name()
    check_takes(mhx, g, 0, xs, (3, 1000), "generic")
    assert list(g.fit_percentiles(0, 1000, xs, PCTS)[3]) == list(aot[3])
    g.close()


def test_an_expression_model_as_written(mhx):
    s = pb.two_peak(n=1200, seed=8)
    x, y, sig, _ = s.data[0]
    params = []
    for k, v in zip(KEYS8, s.theta_star):
        params += [":" + k, float(v)]
    w = mhx.walker_create(function=mhx.models.lisp(TWO_PEAK, as_written=True), data=[x, y], params=params,
                          data_error=sig, n_chains=4, history_capacity=1024)
    e = w.engine
    assert "rtc[expr" in e.kernel_name()
    rng = np.random.default_rng(4)
    for c, n in enumerate((1, 77, 400, 1024)):
        e.set_history(c, *crafted(rng, n, 8, s.theta_star, 0.02))
    check_takes(mhx, e, 0, mhx.fit_linspace(x.min(), x.max(), 333), (1, 100, 1024), "expression")
    check_takes(mhx, e, 0, None, (400,), "expression, own x")
    e.close()


def test_an_expression_of_two_columns_of_x(mhx):
    rng = np.random.default_rng(5)
    n = 900
    X = np.column_stack([rng.uniform(-1, 2, n), rng.uniform(0, 3, n)])
    e = mhx.Engine(3, 2, 1, history_capacity=1024)
    e.set_function_expr(0, "b0 + b1*xcol0*xcol1", ["b0", "b1"], [0, 1])
    e.set_dataset(0, X, np.zeros(n), np.full(n, 0.1))
    e.init_chains(LINE)
    for c, k in enumerate((2, 65, 600)):
        e.set_history(c, *crafted(rng, k, 2, LINE, 0.3))
    Xo = np.column_stack([rng.uniform(-2, 3, 333), rng.uniform(-1, 4, 333)])
    check_takes(mhx, e, 0, Xo.T, (1, 64, 1000), "two columns, other x")
    own = e.fit_percentiles(0, 600, None, PCTS)
    assert own[0].shape == (3, len(PCTS), n)
    for a, b in zip(own, e.fit_percentiles(0, 600, X.T, PCTS)):
        bits(a, b, "two columns, own x")
    Yardstick(mhx, e, 0, X.T).check(600, own, what="two columns, own x")
    with pytest.raises(mhx.MhxError) as err:      # n_cols is not the function's
        e.fit_percentiles(0, 600, X[:, 0], PCTS)
    assert err.value.code == mhx.capi.EINVAL
    e.close()


def test_a_dataset_per_walker_gives_the_bits_of_shared_data(mhx):
    C11, n = 11, 334
    s = pb.two_peak(n=n, seed=6)
    x, y, sig, _ = s.data[0]
    rng = np.random.default_rng(9)
    walks = [crafted(rng, int(k), 8, s.theta_star, 0.02) for k in [1, 2, 40] + list(rng.integers(3, 1024, C11 - 3))]
    shared = s.engine(mhx, C11, history_capacity=1024)
    planes = mhx.Engine(C11, s.d, 1, history_capacity=1024)
    planes.set_function(0, pb.GAUSS, (2, 2), list(range(8)))
    planes.set_dataset_planes(0, x, y[None, :] + 0.01 * rng.standard_normal((C11, n)), sig, mhx.capi.SIGMA_SHARED)
    planes.set_bounds(0, *s.bounds[0])
    for e in (shared, planes):
        e.init_chains(s.theta_star)
        for c, (pr, th) in enumerate(walks):
            e.set_history(c, pr, th)
    assert "planes" in planes.kernel_name()
    xs = mhx.fit_linspace(x.min(), x.max(), 500)
    for take, pts in ((1, xs), (150, xs), (1000, xs), (1000, None)):
        a, b = planes.fit_percentiles(0, take, pts, PCTS), shared.fit_percentiles(0, take, pts, PCTS)
        for u, v in zip(a, b):
            bits(u, v, ("planes against shared", take))
    Yardstick(mhx, planes, 0, xs, chains=(0, 2, 5)).check(1000, planes.fit_percentiles(0, 1000, xs, PCTS),
                                                         what="planes")
    shared.close()
    planes.close()


# ---- 5. a real walk ----------------------------------------------------------------------------
def test_a_real_walk(mhx):
    s = pb.two_peak(n=2000, seed=6)
    C_ = 256
    e = s.engine(mhx, C_, seed=3, history_capacity=2048)
    e.init_chains(pb.perturbed(s.theta_star, C_, 0.01, seed=9))
    e.adaptive_begin(30000, 10.0, 1)
    e.adaptive_advance(3200)
    assert int(e.state()["length"].min()) >= 3000      # the ring (2048) has wrapped
    xs = mhx.fit_linspace(0.0, 1.0)
    for take in (150, 1000):
        got = e.fit_percentiles(0, take, xs)
        print("fit_percentiles 256 chains take %d m 1000: kernels %.3f ms" % (take, e.summary_timing()))
        pct, mean, sd, used, status = got
        assert (status == 0).all() and (used == take).all()
        assert (pct[:, 0] <= pct[:, 1]).all() and (pct[:, 1] <= pct[:, 2]).all()
        assert (sd >= 0).all()
        Yardstick(mhx, e, 0, xs, chains=(0, 100, 255)).check(take, got, [(5, 2), (50, 1), (195, 2)], what="real walk")
    e.close()


# ---- 6. portions -------------------------------------------------------------------------------
def test_chunks_of_points_give_the_bits_of_the_callers_own_slices(mhx):
    """3 chains at take 1024 and 25 000 points: one chain's chunk is the whole blocks that keep
    8 * 1024 bytes a point below 64 MiB - 8064 points - so the call is worked through in four
    chunks of points for each of three portions of one chain"""
    e = crafted_line_engine(mhx, [1024, 700, 1], seed=6)
    m = 25000
    xs = np.linspace(-4.0, 10.0, m)
    whole = e.fit_percentiles(0, 1024, xs, PCTS)
    cuts = [0, 1, 7000, 8064, 8065, 20000, m]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = e.fit_percentiles(0, 1024, xs[lo:hi], PCTS)
        bits(part[0], whole[0][:, :, lo:hi], ("pct", lo))
        bits(part[1], whole[1][:, lo:hi], ("mean", lo))
        bits(part[2], whole[2][:, lo:hi], ("stddev", lo))
        assert list(part[3]) == list(whole[3]) == [1024, 700, 1] and list(part[4]) == list(whole[4]) == [0, 0, 2]
    Yardstick(mhx, e, 0, xs[8000:8200]).check(1024, e.fit_percentiles(0, 1024, xs[8000:8200], PCTS), what="slice")
    e.close()


def test_more_chains_than_one_portion_holds(mhx):
    """The chains of a portion are what the carve gives: of the 64 MiB budget the pieces that do
    not grow with the chains (x0, x1: 16 m bytes) and a piece's alignment each (8 pieces of 256
    bytes) are set aside, and a chain takes 8 (status, n_used) + 8 m take (values) +
    8 m (n_pct + 2) (percentiles, mean, stddev) bytes.  At m = 5, take = 1024 and six percentiles
    that is 1625 chains; three more make a second portion."""
    m, take = 5, 1024
    per = (B - 16 * m - 8 * 256) // (8 + 8 * m * take + 8 * m * (len(PCTS) + 2))
    assert per == 1625
    n = per + 3
    rng = np.random.default_rng(12)
    e = line_engine(mhx, n, history_capacity=1024)
    e.init_chains(LINE)
    lengths = rng.integers(1, 30, n)
    lengths[[0, per - 1, per, n - 1]] = [1024, 1000, 1024, 517]
    for c in range(n):
        e.set_history(c, *crafted(rng, int(lengths[c]), 2, LINE, 0.3))
    got = e.fit_percentiles(0, take, None, PCTS)
    assert list(got[3]) == list(lengths)
    Yardstick(mhx, e, 0, np.array(LF_X), chains=[0, 1, 2, per - 2, per - 1, per, per + 1, n - 1]).check(
        take, got, what="two portions of chains")
    e.close()


# ---- 7. a group --------------------------------------------------------------------------------
def test_a_group_gives_the_bits_of_one_engine(mhx):
    s = pb.two_peak(n=1500, seed=4)
    n = 11
    rng = np.random.default_rng(7)
    walks = [crafted(rng, int(k), 8, s.theta_star, 0.02) for k in rng.integers(1, 600, n)]
    e = s.engine(mhx, n, history_capacity=512)
    g = mhx.Group(n, s.d, s.K, devices=[0, 0], history_capacity=512)
    s.apply(g)
    e.init_chains(s.theta_star)
    g.init_chains(s.theta_star)
    for c, (pr, th) in enumerate(walks):
        e.set_history(c, pr, th)
        i = 0 if c < g.ranges[1][0] else 1
        g.engines[i].set_history(c - g.ranges[i][0], pr, th)
    xs = mhx.fit_linspace(0.0, 1.0, 700)
    for take in (1, 150, 512):
        whole, single_ = g.fit_percentiles(0, take, xs, PCTS), e.fit_percentiles(0, take, xs, PCTS)
        parts = [x.fit_percentiles(0, take, xs, PCTS) for x in g.engines]
        for k in range(5):
            bits(whole[k], single_[k], (take, k))
            bits(whole[k], np.concatenate([p[k] for p in parts]), (take, k))
    e.close()
    g.close()


# ---- 8. through the ABI ------------------------------------------------------------------------
def test_edges_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = line_engine(mhx, 2, history_capacity=64)
    m = 7
    xs = np.linspace(0.0, 1.0, m)
    xp = xs.ctypes.data_as(capi.f64p)
    num, nump = capi.as_i32([5, 50, 195])
    den, denp = capi.as_i32([2, 1, 2])
    mark = 7.25
    out = {"pct": np.full((2, 3, m), mark), "mean": np.full((2, m), mark), "sd": np.full((2, m), mark),
           "used": np.full(2, 77, dtype=np.int32), "st": np.full(2, 77, dtype=np.int32)}

    def ptrs(skip=None):
        return [None if k == skip else out[k].ctypes.data_as(capi.f64p if out[k].dtype == np.float64 else capi.i32p)
                for k in ("pct", "mean", "sd", "used", "st")]

    def call(h=None, fn=0, take=5, x=xp, n_cols=1, pts=m, nu=nump, de=denp, n_pct=3, skip=None):
        return lib.mhx_get_fit_percentiles(e._h if h is None else h, fn, take, x, n_cols, pts, nu, de, n_pct,
                                           *ptrs(skip))

    def untouched():
        return all((out[k] == (mark if out[k].dtype == np.float64 else 77)).all() for k in out)

    assert call() == capi.ESTATE and untouched()                 # before mhx_init_chains
    e.init_chains(LINE)
    cap = e.history_capacity()
    for take in (0, -1, cap + 1):
        assert call(take=take) == capi.EINVAL
    for fn in (-1, 1):
        assert call(fn=fn) == capi.EINVAL
    assert call(pts=0) == capi.EINVAL and call(pts=-3) == capi.EINVAL
    assert call(n_cols=2) == capi.EINVAL and call(n_cols=0) == capi.EINVAL
    assert call(n_pct=-1) == capi.EINVAL and call(n_pct=17) == capi.EINVAL
    assert call(nu=None) == capi.EINVAL and call(de=None) == capi.EINVAL
    bad_num, bad_nump = capi.as_i32([5, 201, 195])               # 201/2 per cent
    assert call(nu=bad_nump) == capi.EINVAL
    bad_den, bad_denp = capi.as_i32([2, 0, 2])
    assert call(de=bad_denp) == capi.EINVAL
    assert call(x=None, pts=4) == capi.EINVAL                     # the dataset's own x has 5 points
    assert lib.mhx_get_fit_percentiles(None, 0, 5, xp, 1, m, nump, denp, 3, *ptrs()) == capi.EINVAL
    assert untouched()
    # the outputs, all and every one NULL in turn
    assert call() == capi.OK and not untouched()
    full = {k: v.copy() for k, v in out.items()}
    assert list(full["used"]) == [1, 1] and list(full["st"]) == [capi.FITPCT_ONE_STEP] * 2
    assert np.isnan(full["sd"]).all()
    for skip in out:
        for k in out:
            out[k][...] = mark if out[k].dtype == np.float64 else 77
        assert call(skip=skip) == capi.OK
        for k in out:
            if k == skip:
                assert (out[k] == (mark if out[k].dtype == np.float64 else 77)).all()
            else:
                assert np.array_equal(out[k].view(np.uint8), full[k].view(np.uint8)), (skip, k)
    assert lib.mhx_get_fit_percentiles(e._h, 0, 5, xp, 1, m, nump, denp, 3, None, None, None, None, None) == capi.OK
    # n_pct = 0: the moments only, the percentile lists may be NULL
    for k in out:
        out[k][...] = mark if out[k].dtype == np.float64 else 77
    assert call(nu=None, de=None, n_pct=0) == capi.OK
    assert (out["pct"] == mark).all() and np.array_equal(out["mean"], full["mean"]) and list(out["used"]) == [1, 1]
    assert call(x=None, pts=5, skip="pct") == capi.OK              # the dataset's own x
    assert e.summary_timing() >= 0.0
    e.close()


def test_a_take_whose_values_cannot_be_staged_is_refused_by_name(mhx):
    """one chain's smallest chunk - 128 points - at take 65536 is 64 MiB of values: refused, and the
    message names the greatest take that fits, by the carve's own accounting"""
    capi, lib = mhx.capi, mhx.capi.lib()
    e = line_engine(mhx, 1, history_capacity=65536)
    e.init_chains(LINE)
    assert e.history_capacity() == 65536
    blk = capi.FITPCT_BLOCK
    xs = np.linspace(0.0, 1.0, blk + 5)
    out = np.full((1, 3, blk + 5), 7.25)
    with pytest.raises(mhx.MhxError) as err:
        e.fit_percentiles(0, 65536, xs)
    fits = max(t for t in range(65000, 65537)
               if 8 + 16 * blk + 8 * blk * t + 8 * blk * (3 + 2) + 8 * 256 <= B)
    assert err.value.code == capi.EUNSUPPORTED and str(fits) in str(err.value), str(err.value)
    num, nump = capi.as_i32([5, 50, 195])
    den, denp = capi.as_i32([2, 1, 2])
    assert lib.mhx_get_fit_percentiles(e._h, 0, 65536, xs.ctypes.data_as(capi.f64p), 1, blk + 5, nump, denp, 3,
                                       out.ctypes.data_as(capi.f64p), None, None, None, None) == capi.EUNSUPPORTED
    assert (out == 7.25).all()
    # the greatest take that fits is served, and so is the whole ring at fewer points than a block
    assert e.fit_percentiles(0, fits, xs)[3][0] == 1
    assert e.fit_percentiles(0, 65536, xs[:blk - 1])[3][0] == 1
    e.close()


# ---- 9. the mirror -----------------------------------------------------------------------------
def test_the_mirrors_credible_bands(mhx):
    s = pb.two_peak(n=600, seed=12)
    x, y, sig, _ = s.data[0]
    params = []
    for k, v in zip(KEYS8, s.theta_star):
        params += [":" + k, float(v)]
    w = mhx.walker_create(function=mhx.models.gauss_peaks(["b0", "b1"], [["a1", "mu1", "w1"], ["a2", "mu2", "w2"]]),
                          data=[x, y], params=params, data_error=sig, n_chains=5, seed=2,
                          history_capacity=2048)
    mhx.walker_adaptive_steps(w, 1500)
    e = w.engine
    for band, pts, lo_hi in ((":95cr", 1000, (2.5, 97.5)), (":iqr", 200, (25, 75)),
                             ((":percentile", 10, 90), 77, (10, 90))):
        every = mhx.walker_set_get_fit_credible(w, take=1000, points=pts, band=band)
        assert len(every) == 5
        x_fit = mhx.fit_linspace(x.min(), x.max(), pts)
        pct, mean, sd, _, _ = e.fit_percentiles(0, 1000, x_fit, [lo_hi[0], 50, lo_hi[1]])
        for c in range(5):
            one = mhx.walker_get_fit_credible(w, take=1000, points=pts, band=band, chain=c)
            assert one == every[c]
            xf, hi, lo, med, mu, sdev = one
            assert xf == list(x_fit) and hi == list(pct[c, 2]) and lo == list(pct[c, 0])
            assert med == list(pct[c, 1]) and mu == list(mean[c]) and sdev == list(sd[c])
            assert (np.array(lo) <= np.array(med)).all() and (np.array(med) <= np.array(hi)).all()
    assert mhx.walker_get_fit_credible(w)[1] == mhx.walker_get_fit_credible(w, band=":95cr", take=1000, points=1000)[1]
    with pytest.raises(ValueError):
        mhx.walker_get_fit_credible(w, band=":nonsense")
    with pytest.raises(ValueError):
        mhx.walker_get_fit_credible(w, band=(":percentile", 90, 10))
    e.close()
    # a window that holds a value that is not finite
    xl = np.linspace(0.0, 1.0, 50)
    wl = mhx.walker_create(function=mhx.models.poly("b", "m"), data=[xl, 1.0 + 2.0 * xl],
                           params=[":b", 1.0, ":m", 2.0], data_error=0.1, n_chains=3, history_capacity=64)
    rng = np.random.default_rng(3)
    for c in range(3):
        pr, th = crafted(rng, 30, 2, np.array([1.0, 2.0]), 0.1)
        if c == 1:
            th[4] = [1e308, 1e308]
        wl.engine.set_history(c, pr, th)
    assert len(mhx.walker_get_fit_credible(wl, take=30, chain=0)) == 6
    with pytest.raises(FloatingPointError):
        mhx.walker_get_fit_credible(wl, take=30, chain=1)
    with pytest.raises(FloatingPointError):
        mhx.walker_set_get_fit_credible(wl, take=30)
    assert len(mhx.walker_get_fit_credible(wl, take=3, chain=1)) == 6      # (the bad step is the fifth newest)
    wl.engine.close()
