"""walker-set-get (mcmc-fitting.lisp:1029-1030): the summarising selectors of walker-get for
EVERY chain in one launch (mhx_get_percentiles / _covariances / _proposal_factors / _window_best
and their mhx_group_get_* forms) against the per-chain route and the Python mirror's own
functions.  Every comparison is exact (np.array_equal / ==) and covers all chains of its
engine: each result is a selection of stored values, the IEEE mean of two of them, or the same
IEEE operations in the same order as the yardstick."""
import os
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

import problems as pb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCTS = [50, 2.5, 97.5, 25, 75, 84.1, 0, 100]
LENGTHS = [1, 2, 3, 9, 10, 64, 65, 1023, 1024, 2047, 2048]
LF_X, LF_Y = [-4.0, -1.0, 2.0, 5.0, 10.0], [0.0, 2.0, 5.0, 9.0, 13.0]


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def line_engine(mhx, n_chains, d=2, used=(0, 1), **kw):
    """the five-point line fit over the parameters `used` of a vector of d (the histories of
    these tests are injected: the model does not matter)"""
    e = mhx.Engine(n_chains, d, 1, **kw)
    e.set_function(0, mhx.capi.MODEL_POLY, (), list(used))
    e.set_dataset(0, LF_X, LF_Y, np.full(5, 0.2))
    return e


def crafted_walk(rng, n, d, kind):
    """a walk of n steps, NEWEST FIRST (prob [n], theta [n][d]), built oldest first:
    0 a Metropolis-like walk: runs of repeated steps (unique < length), negative values
    1 the same over a handful of parameter values that recur under different probs (ties in the
      sort), some of them neighbours in the last bit
    2 strictly increasing probs (every step but the oldest is a forward step)
    3 strictly decreasing probs (no forward step: the l-matrix is L_CAUGHT)
    4 decreasing but for one rise (one forward step: L_EMPTY)
    5 like 0 with one parameter that never moves (a zero pivot in the Cholesky)"""
    prob, theta = np.empty(n), np.empty((n, d))
    base = np.array([1.0, -2.5, 1e-3, -1e5, 0.0, 7.0, -0.125])
    pool = np.concatenate([base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf)])
    p, th = rng.normal(-50.0, 3.0), rng.normal(0.0, 2.0, d)
    for i in range(n):
        if kind in (0, 1, 5):
            if i == 0 or rng.random() < 0.4:
                p = rng.normal(-50.0, 3.0)
                th = rng.choice(pool, d) if kind == 1 else th + rng.normal(0.0, 0.3, d)
                if kind == 5:
                    th[d - 1] = 4.25
        else:
            up = kind == 2 or (kind == 4 and i == n // 2)
            p = p + rng.uniform(0.1, 1.0) * (1.0 if up else -1.0)
            th = th + rng.normal(0.0, 0.3, d)
        prob[i], theta[i] = p, th
    return prob[::-1].copy(), theta[::-1].copy()


def inject(e, rng, lengths):
    walks = []
    for c, n in enumerate(lengths):
        pr, th = crafted_walk(rng, int(n), e.d, c % 6)
        e.set_history(c, pr, th)
        walks.append((pr, th))
    return walks


def percentile(mirror, n, col):
    return mirror._percentile(n, col)


def reduce_best(prob):
    """index of walker_get's :most-likely-step over newest-first probs (M:503-505)"""
    best = 0
    for s in range(1, len(prob)):
        best = best if prob[best] > prob[s] else s
    return best


def check_crafted(mhx, e, walks, takes, n_checked=None):
    """every selector of engine e at every take against the mirror and the per-chain route, for
    the chains whose walks are given: all of them, unless n_checked says how many"""
    from lisp_mcmc_amd import walker as mirror
    capi = mhx.capi
    seen = set()
    n, d = e.n_chains, e.d
    for take in takes:
        pct, used = e.percentiles(take, PCTS)
        cov, n_unique, cst = e.covariances(take)
        st, L, nf = e.proposal_factors(take)
        bp, bth = e.window_best(take)
        for c, (pr, th) in enumerate(walks):
            t = min(take, len(pr))
            assert used[c] == t, (take, c)
            want = np.array([[percentile(mirror, q, th[:t, j]) for j in range(d)] for q in PCTS])
            assert np.array_equal(pct[c], want), (take, c)
            bits = pr[:t].view(np.uint64)
            keep = [i for i in range(t) if i + 1 >= t or bits[i] != bits[i + 1]]
            assert n_unique[c] == len(keep), (take, c)
            wcov = mirror.lplist_covariance(th[keep])
            assert np.array_equal(cov[c], wcov), (take, c)
            assert cst[c] == (capi.L_OK if np.isfinite(wcov).all() else capi.L_CAUGHT), (take, c)
            s1, L1, nf1 = e.proposal_factor(c, take)
            assert (st[c], nf[c]) == (s1, nf1), (take, c)
            assert np.array_equal(L[c], L1), (take, c)
            seen.add(int(s1))
            b = reduce_best(pr[:t])
            assert bp[c] == pr[b] and np.array_equal(bth[c], th[b]), (take, c)
        assert len(walks) == (n if n_checked is None else n_checked)
    return seen


def test_crafted_histories_every_selector_every_chain_d2(mhx):
    rng = np.random.default_rng(2024)
    e = line_engine(mhx, 300, history_capacity=2048)
    e.init_chains([-1.0, 2.0])
    assert e.history_capacity() == 2048
    lengths = LENGTHS * 6 + list(rng.integers(1, 2049, 300 - 6 * len(LENGTHS)))
    walks = inject(e, rng, lengths)
    assert any(len(set(pr.tolist())) < len(pr) for pr, _ in walks)  # repeated probs occur
    seen = check_crafted(mhx, e, walks, (1, 2, 57, 1000, 2048))
    capi = mhx.capi
    assert {capi.L_OK, capi.L_CAUGHT, capi.L_EMPTY} <= seen, seen
    e.close()


def test_crafted_histories_every_selector_every_chain_d33(mhx):
    rng = np.random.default_rng(33)
    e = line_engine(mhx, 40, d=33, used=range(0, 32, 4), history_capacity=2048)
    e.init_chains(np.linspace(-1.0, 2.0, 33))
    lengths = LENGTHS + list(rng.integers(1, 2049, 40 - len(LENGTHS)))
    walks = inject(e, rng, lengths)
    seen = check_crafted(mhx, e, walks, (1, 2, 57, 1000, 2048))
    capi = mhx.capi
    assert {capi.L_OK, capi.L_CAUGHT, capi.L_EMPTY} <= seen, seen
    e.close()


def test_chains_beyond_one_portion_of_the_stage_buffer(mhx):
    """d = 33 at take 8: a chain of the factor call takes 2 x 33 x 33 doubles, two ints and 8
    ints of scratch, 17464 bytes, so 3842 chains fill the 64 MiB of a portion - an engine of 4000
    chains works through two, and so does either engine of a group of 8000.  (history_capacity 8
    is asked for; the ring is never shorter than the adaptation windows, 1024 steps.)  Chain c
    carries walk c % 40; chains 0-39 are checked against the mirror, every other chain must give
    its walk's results to the bit, and the group what the single engine gives."""
    rng = np.random.default_rng(4000)
    d, ring, period, n = 33, 8, 40, 4000
    per_chain = 2 * d * d * 8 + 2 * 4 + ring * 4
    assert per_chain == 17464 and ((1 << 26) - 5 * 256) // per_chain == 3842 < n
    walks = [crafted_walk(rng, 1 + k % ring, d, k % 6) for k in range(period)]
    assert {len(pr) for pr, _ in walks} == set(range(1, ring + 1))
    e = line_engine(mhx, n, d=d, used=range(0, 32, 4), history_capacity=ring)
    g = mhx.Group(2 * n, d, 1, devices=[0, 0], history_capacity=ring)
    g.set_function(0, mhx.capi.MODEL_POLY, (), list(range(0, 32, 4)))
    g.set_dataset(0, LF_X, LF_Y, np.full(5, 0.2))
    assert g.ranges == [(0, n), (n, n)]
    for obj in (e, g):
        obj.init_chains(np.linspace(-1.0, 2.0, d))
    for part, (first, count) in zip([e] + g.engines, [(0, n)] + g.ranges):
        for c in range(count):
            part.set_history(c, *walks[(first + c) % period])
    check_crafted(mhx, e, walks, (ring,), n_checked=period)
    calls = (lambda o: o.percentiles(ring, PCTS), lambda o: o.covariances(ring),
             lambda o: o.proposal_factors(ring), lambda o: o.window_best(ring))
    for which, call in enumerate(calls):
        single, whole = call(e), call(g)
        for k in range(len(single)):
            a, b = np.asarray(single[k]), np.asarray(whole[k])
            assert a.shape[0] == n and b.shape[0] == 2 * n, (which, k)
            # every chain is its walk's chain among the first 40 (2n is a multiple of the period)
            assert a.tobytes() == a[np.arange(n) % period].tobytes(), (which, k)
            assert b.tobytes() == b[np.arange(2 * n) % period].tobytes(), (which, k)
            assert b[:n].tobytes() == a.tobytes(), (which, k)
    e.close()
    g.close()


def outcome(fn):
    """the value of fn(), or the condition it raises, with the warnings it gave"""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        try:
            val = ("value", fn())
        except Exception as ex:  # compared, not swallowed
            val = ("raised", type(ex), str(ex))
    return val, [w for w in rec]


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    if hasattr(a, "prob") and hasattr(a, "params"):
        return type(a) is type(b) and a.prob == b.prob and same(a.params, b.params)
    return type(a) is type(b) and a == b


def test_a_real_walk_through_a_wrapped_ring(mhx):
    """4096 chains of config 2's problem at a small N, default ring of 1024, 3000 iterations:
    walker_set_get equals walker_get(..., chain=c) for EVERY chain.  Every chain's trace is read
    once and the mirror's own functions applied to it; every 64th chain goes through walker_get
    itself."""
    from lisp_mcmc_amd import walker as mirror
    from lisp_mcmc_amd.walker import HistoryTruncated
    s = pb.two_peak(n=700, seed=12)
    keys = ["b0", "b1", "a1", "mu1", "w1", "a2", "mu2", "w2"]
    x, y, sig, _ = s.data[0]
    idx, lo, hi = s.bounds[0]
    n = 4096
    params = []
    for k, v in zip(keys, s.theta_star):
        params += [":" + k, float(v)]
    w = mhx.walker_create(
        function=mhx.models.gauss_peaks(keys[:2], [tuple(keys[2:5]), tuple(keys[5:8])]),
        data=[x, y], params=params, data_error=sig,
        log_prior=mhx.prior_bounds({keys[i]: (lo[i], hi[i]) for i in idx}),
        n_chains=n, theta0=pb.perturbed(s.theta_star, n, 0.01, seed=5), seed=41)
    mhx.walker_adaptive_steps(w, 3000)
    e = w.engine
    ring = e.history_capacity()
    assert ring == 1024
    cap = e.state()["length"]
    assert (cap > ring).any()  # (rings have wrapped)
    traces = [e.trace(c, ring) for c in range(n)]
    selectors = (":median-params", ":stddev-params", ":covariance-matrix", ":l-matrix",
                 ":most-likely-step", ":acceptance")
    for take in (None, 500, 1000):
        tc = cap.copy() if take is None else np.minimum(take, cap)   # walker_get's window
        past = tc > ring
        for get in selectors:
            got, warned = outcome(lambda: mhx.walker_set_get(w, get=get, take=take))
            trunc = [x_ for x_ in warned if issubclass(x_.category, HistoryTruncated)]
            device_only = get in (":stddev-params", ":l-matrix", ":acceptance")
            if past.any() and device_only:
                # a window longer than the ring: walker_get hands it to the device, which
                # refuses it - so the set raises what the first such chain raises
                first = int(np.argmax(past))
                one, _ = outcome(lambda: mhx.walker_get(w, get=get, take=take, chain=first))
                assert one[0] == "raised" and one[1] is mhx.MhxError
                assert got == one, (get, got)
                continue
            assert got[0] == "value", (get, take, got)
            vals = got[1]
            assert len(vals) == n
            assert len(trunc) == (1 if past.any() else 0), (get, take)
            for c in range(n):
                t = int(min(tc[c], ring))
                pr, th = traces[c][0][:t], traces[c][1][:t]
                assert len(pr) == t
                bits = pr.view(np.uint64)
                keep = [i for i in range(t) if i + 1 >= t or bits[i] != bits[i + 1]]
                if get == ":median-params":
                    want = {k: mirror._percentile(50, th[:, j]) for j, k in enumerate(keys)}
                elif get == ":covariance-matrix":
                    want = mirror.lplist_covariance(th[keep])
                elif get == ":most-likely-step":
                    b = reduce_best(pr)
                    want = w._step(th[b], pr[b])
                elif get == ":acceptance":
                    want = Fraction(int(round(float(len(keep)) / float(t) * t)), t)
                else:
                    st, L, nf = e.proposal_factor(c, t)
                    assert st == mhx.capi.L_OK and nf > 10, c
                    want = L if get == ":l-matrix" else \
                        {k: float(L[j, j]) for j, k in enumerate(keys)}
                assert same(vals[c], want), (get, take, c)
                if c % 64 == 0:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        one = mhx.walker_get(w, get=get, take=take, chain=c)
                    assert same(vals[c], one), (get, take, c)
    # the struct-slot selector and a list-valued one, the lengths read once
    ml = mhx.walker_set_get(w, get=":most-likely-params")
    st = e.state()
    assert ml == [dict(zip(keys, st["best_theta"][c].tolist())) for c in range(n)]
    ll = mhx.walker_set_get(w, get=":log-liklihoods", take=5)
    assert ll == [traces[c][0][:5].tolist() for c in range(n)]
    e.close()


def test_a_window_too_large_for_lds(mhx):
    """64 chains, ring 32768, walks of 30000 steps, take 30000: the selection reads its columns
    from memory"""
    rng = np.random.default_rng(7)
    n, d, steps = 64, 3, 30000
    e = line_engine(mhx, n, d=d, used=(0, 2), history_capacity=32768)
    e.init_chains([-1.0, 0.5, 2.0])
    assert e.history_capacity() == 32768
    walks = []
    for c in range(n):
        th = rng.normal(0.0, 1.0, (steps, d))
        th[:, 1] = rng.integers(-5, 6, steps) * 0.25      # heavy ties
        th[rng.integers(0, steps, 50), 2] = -0.0
        pr = rng.normal(-10.0, 1.0, steps)
        e.set_history(c, pr, th)
        walks.append(th)
    pct, used = e.percentiles(steps, PCTS)
    assert (used == steps).all()
    for c in range(n):
        srt = np.sort(walks[c], axis=0)
        for qi, q in enumerate(PCTS):
            pos = Fraction(q).limit_denominator(1000) * (steps - 1) / 100
            lo = pos.numerator // pos.denominator
            want = srt[lo] if pos == lo else (srt[lo] + srt[lo + 1]) / 2
            assert np.array_equal(pct[c, qi], want), (c, q)
    # ... and a window of that ring that does fit LDS gives what the large path gives for it
    small, _ = e.percentiles(1000, [50, 97.5])
    for c in range(n):
        srt = np.sort(walks[c][:1000], axis=0)
        assert np.array_equal(small[c, 0], (srt[499] + srt[500]) / 2)
    e.close()


def test_group_equals_its_engines_and_a_single_engine(mhx):
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
    for take in (1, 200, 1024):
        calls = (lambda o: o.percentiles(take, PCTS), lambda o: o.covariances(take),
                 lambda o: o.proposal_factors(take), lambda o: o.window_best(take))
        for call in calls:
            whole, parts, single = call(g), [call(x) for x in g.engines], call(e)
            for k in range(len(whole)):
                assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts])), (take, k)
                assert np.array_equal(whole[k], single[k]), (take, k)
    e.close()
    g.close()


def test_edges_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    e = line_engine(mhx, 3)
    d, n = 2, 3
    num, nump = capi.as_i32([50, 5])
    den, denp = capi.as_i32([1, 2])
    out = np.full((n, 2, d), 777.0)
    used = np.full(n, -7, dtype=np.int32)
    outp, usedp = out.ctypes.data_as(capi.f64p), used.ctypes.data_as(capi.i32p)
    cov = np.zeros((n, d, d))
    covp = cov.ctypes.data_as(capi.f64p)
    i1, i2 = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    i1p, i2p = i1.ctypes.data_as(capi.i32p), i2.ctypes.data_as(capi.i32p)
    pr, th = np.zeros(n), np.zeros((n, d))
    prp, thp = pr.ctypes.data_as(capi.f64p), th.ctypes.data_as(capi.f64p)

    def all_four(take):
        return [lib.mhx_get_percentiles(e._h, take, nump, denp, 2, outp, usedp),
                lib.mhx_get_covariances(e._h, take, covp, i1p, i2p),
                lib.mhx_get_proposal_factors(e._h, take, covp, i1p, i2p),
                lib.mhx_get_window_best(e._h, take, prp, thp)]

    assert all_four(10) == [capi.ESTATE] * 4              # before mhx_init_chains
    e.init_chains([[-1.0, 2.0], [1e308, 1e308], [0.5, 1.5]])
    status, _ = e.chain_status()
    assert status[1] == capi.CHAIN_FP_TRAP
    ring = e.history_capacity()
    assert all_four(0) == [capi.EINVAL] * 4
    assert all_four(ring + 1) == [capi.EINVAL] * 4
    assert lib.mhx_get_percentiles(e._h, 10, nump, denp, capi_max(lib) + 1, outp, usedp) == capi.EINVAL
    bad, badp = capi.as_i32([101, 5])
    assert lib.mhx_get_percentiles(e._h, 10, badp, denp, 2, outp, usedp) == capi.EINVAL
    assert (out == 777.0).all() and (used == -7).all()      # nothing was written so far
    # n_pct = 0: fine, nothing written
    assert lib.mhx_get_percentiles(e._h, 10, None, None, 0, outp, usedp) == capi.OK
    assert (out == 777.0).all() and (used == -7).all()
    # NULL outputs
    assert lib.mhx_get_percentiles(e._h, 10, nump, denp, 2, None, None) == capi.OK
    assert lib.mhx_get_covariances(e._h, 10, None, None, None) == capi.OK
    assert lib.mhx_get_proposal_factors(e._h, 10, None, None, None) == capi.OK
    assert lib.mhx_get_window_best(e._h, 10, None, None) == capi.OK
    # a frozen chain is summarised from the history it has: its one step
    assert all_four(ring) == [capi.OK] * 4
    state = e.state()
    assert np.array_equal(used, np.minimum(state["length"], ring)) and (used == 1).all()
    for c in range(n):
        assert np.array_equal(out[c], np.array([state["theta"][c]] * 2)), c
        assert np.array_equal(th[c], state["theta"][c]), c
    g = mhx.Group(4, 2, 1, devices=[0, 0])
    assert lib.mhx_group_get_window_best(g._h, 10, None, None) == capi.ESTATE
    assert lib.mhx_group_get_percentiles(None, 10, nump, denp, 2, None, None) == capi.EINVAL
    g.close()
    e.close()


def capi_max(lib):
    """MHX_MAX_PERCENTILES of include/mhx.h"""
    import re
    src = open(os.path.join(ROOT, "include", "mhx.h")).read()
    return int(re.search(r"#define\s+MHX_MAX_PERCENTILES\s+(\d+)", src).group(1))


def test_c_example_prints_the_percentiles_of_the_first_walkers(tmp_path):
    exe = str(tmp_path / "walker_set")
    lib = os.path.join(ROOT, "lisp-mcmc_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "walker_set.c"), "-L", lib, "-lmhx",
                           "-Wl,-rpath," + lib, "-lm", "-o", exe])
    out = subprocess.run([exe, "1", "64"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("  walker ")]
    assert len(rows) == 3 * 8, out.stdout          # 3 walkers x 8 parameters
    for r in rows:
        # "  walker <c> <name> median <m> 95cr [<lo>, <hi>] over <n> steps"
        assert r[3] == "median" and r[5] == "95cr" and r[8] == "over", r
        med, lo, hi = float(r[4]), float(r[6].strip("[,")), float(r[7].strip("],"))
        assert lo <= med <= hi, r
        assert int(r[9]) >= 1000, r
