"""The host side of the autocorrelation read-out, no device: lisp_mcmc_amd.autocorr against the
yardstick of tests/autocorr_cases.py (bit for bit), the status bits, the estimator on AR(1)
sequences of known autocorrelation time, and mhx_split_rhat through ctypes against its formula."""
import numpy as np
import pytest

import autocorr_cases as ac
import histo_cases as hc


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def crafted_columns(lengths, seed=1361):
    """the parameter columns, newest first, of histo_cases.crafted_d2's recipe"""
    rng = np.random.default_rng(seed)
    for c, n in enumerate(lengths):
        _prob, theta = hc.crafted_walk(rng, int(n), 2, c % 3)
        for p in range(2):
            yield c, p, theta[:, p]


def test_the_yardstick_is_the_definitions_one_operation_at_a_time():
    """column_autocorr (a matrix of products accumulated along s) against plain Python floats"""
    for c, p, x in crafted_columns([1, 2, 3, 9, 64, 65] * 3, seed=5):
        for max_lag in (1, 2, 63, 64):
            a, b = ac.column_autocorr(x, max_lag), ac.scalar_autocorr(x, max_lag)
            assert ac.same_bits(a[0], b[0]) and ac.same_bits(np.array(a[1:3]), np.array(b[1:3])), (c, p, max_lag)
            assert a[3] == b[3]


def test_autocorr_equals_the_yardstick_bit_for_bit(mhx):
    lengths = [1, 2, 3, 9, 64, 65, 2048]
    statuses = set()
    for c, p, x in crafted_columns(lengths * 3):          # kinds 0, 1, 2 at every length
        for max_lag in (1, 2, 63, 64, 1023):
            rho, tau, ess, status = mhx.autocorr(x, max_lag)
            want = ac.column_autocorr(x, max_lag)
            assert len(rho) == min(max_lag, len(x) - 1) + 1
            assert ac.same_bits(rho, want[0]), (c, p, max_lag)
            assert ac.same_bits(np.array([tau, ess]), np.array(want[1:3])), (c, p, max_lag, tau, want[1])
            assert status == want[3], (c, p, max_lag)
            statuses.add(status)
    assert statuses == {0, 2, 4, 6}
    # a two-step window: rho_1 = -1/2, P_0 = 1/2, tau = 0, ess = +inf, nothing clamped
    rho, tau, ess, status = mhx.autocorr([3.0, 1.0], 5)
    assert rho.tolist() == [1.0, -0.5] and tau == 0.0 and ess == np.inf and status == ac.OPEN
    # one step: no P_j at all, 0/0
    rho, tau, ess, status = mhx.autocorr([3.0], 5)
    assert np.isnan(rho).all() and np.isnan(tau) and np.isnan(ess) and status == ac.CONSTANT | ac.OPEN
    assert mhx.autocorr([1.0, np.inf, 2.0], 2)[3] & ac.NONFINITE
    for bad in (0, 1024):
        with pytest.raises(ValueError):
            mhx.autocorr([1.0, 2.0], bad)


def test_every_status_occurs_on_the_crafted_walks(mhx):
    """histo_cases.crafted_d2's 300 walks, whole, at max_lag 255"""
    rng = np.random.default_rng(1361)
    lengths = hc.LENGTHS * 6 + list(rng.integers(1, 2049, 300 - 6 * len(hc.LENGTHS)))
    counts = {}
    for c, n in enumerate(lengths):
        _prob, theta = hc.crafted_walk(rng, int(n), 2, c % 3)
        for p in range(2):
            status = ac.column_autocorr(theta[:, p], 255)[3]
            counts[status] = counts.get(status, 0) + 1
            if n <= 65:
                assert mhx.autocorr(theta[:, p], 255)[3] == status
    assert counts == {0: 389, 2: 13, 4: 186, 6: 12}


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ar1_sequences_have_the_known_autocorrelation_time(mhx, phi):
    """64 AR(1) sequences of 2048 steps: tau = (1 + phi) / (1 - phi); Geyer's estimate over 255
    lags has a median within 15 % of it and never runs out of lags"""
    rng = np.random.default_rng(7)
    taus = []
    for _ in range(64):
        e = rng.normal(size=2048)
        x = np.empty(2048)
        x[0] = e[0] / np.sqrt(1 - phi * phi)
        for s in range(1, 2048):
            x[s] = phi * x[s - 1] + e[s]
        rho, tau, ess, status = ac.column_autocorr(x, 255)
        assert not status & ac.OPEN and status == 0
        assert ess == 2048 / tau
        taus.append(tau)
    got = mhx.autocorr(x, 255)
    assert ac.same_bits(got[0], rho) and got[1:] == (tau, ess, status)
    exact = (1 + phi) / (1 - phi)
    print("phi %.1f: median tau %.3f against %.3f" % (phi, np.median(taus), exact))
    assert abs(np.median(taus) - exact) <= 0.15 * exact


# ---- mhx_split_rhat: host only

def rhat_formula(half_mean, half_var, h):
    """the header's formula in numpy, every sum serial from its first term"""
    n, nc, _ = half_mean.shape
    out = np.zeros(nc)
    with np.errstate(all="ignore"):
        for k in range(nc):
            mu, var = half_mean[:, k, :].reshape(-1), half_var[:, k, :].reshape(-1)   # chain 0 half 0, half 1, ...
            m = len(mu)
            w = ac.serial(var) / m
            mean = ac.serial(mu) / m
            b_over_h = ac.serial((mu - mean) * (mu - mean)) / (m - 1)
            out[k] = np.sqrt((np.float64(h - 1) / np.float64(h) * w + b_over_h) / w)
    return out


def call_rhat(mhx, half_mean, half_var, n_used, n_chains=None, n_cols=None, want_out=True):
    capi, lib = mhx.capi, mhx.capi.lib()
    hm, hv = np.ascontiguousarray(half_mean, dtype=np.float64), np.ascontiguousarray(half_var, dtype=np.float64)
    nu = np.ascontiguousarray(n_used, dtype=np.int32)
    out = np.full(hm.shape[1], -7.0)
    rc = lib.mhx_split_rhat(hm.ctypes.data_as(capi.f64p), hv.ctypes.data_as(capi.f64p),
                            nu.ctypes.data_as(capi.i32p), hm.shape[0] if n_chains is None else n_chains,
                            hm.shape[1] if n_cols is None else n_cols,
                            out.ctypes.data_as(capi.f64p) if want_out else None)
    return rc, out, lib.mhx_last_error().decode()


def test_split_rhat_is_its_formula_bit_for_bit(mhx):
    rng = np.random.default_rng(11)
    for n in (1, 2, 300):
        for nc in (1, 33):
            for n_used in (4, 5, 1000, 2047):
                hm = rng.normal(1.0, 0.3, (n, nc, 2))
                hv = rng.gamma(2.0, 0.5, (n, nc, 2))
                rc, got, _ = call_rhat(mhx, hm, hv, np.full(n, n_used))
                assert rc == mhx.capi.OK
                assert ac.same_bits(got, rhat_formula(hm, hv, n_used // 2)), (n, nc, n_used)
                assert ac.same_bits(mhx.split_rhat(hm, hv, np.full(n, n_used)), got)


def test_split_rhat_on_chains_that_agree_and_on_one_that_does_not(mhx):
    rng = np.random.default_rng(12)
    n, t = 8, 400
    walks = rng.normal(0.0, 1.0, (n, t))
    moments = [[ac.half_moments(w)] for w in walks]                       # [n][1] of (means, variances)
    hm = np.array([[m[0] for m in row] for row in moments])
    hv = np.array([[m[1] for m in row] for row in moments])
    assert hm.shape == (n, 1, 2)
    # the same sequence in every half: B = 0, rhat = sqrt((h - 1) / h), a little below 1
    rc, got, _ = call_rhat(mhx, np.full((n, 1, 2), 0.25), np.full((n, 1, 2), 2.0), np.full(n, t))
    assert rc == mhx.capi.OK and got[0] == np.sqrt(np.float64(199) / np.float64(200)) < 1.0
    rc, agree, _ = call_rhat(mhx, hm, hv, np.full(n, t))
    assert rc == mhx.capi.OK and 0.99 < agree[0] < 1.02
    hm[3] += 3.0                                                          # one chain sits elsewhere
    rc, apart, _ = call_rhat(mhx, hm, hv, np.full(n, t))
    assert rc == mhx.capi.OK and apart[0] > 1.3
    # W = 0 follows IEEE: no spread within, some between -> +inf; none at all -> 0/0
    zero = np.zeros((n, 1, 2))
    rc, got, _ = call_rhat(mhx, hm, zero, np.full(n, t))
    assert rc == mhx.capi.OK and got[0] == np.inf
    rc, got, _ = call_rhat(mhx, zero, zero, np.full(n, t))
    assert rc == mhx.capi.OK and np.isnan(got[0])


def test_split_rhat_refuses_windows_that_are_not_comparable(mhx):
    capi = mhx.capi
    hm, hv = np.ones((5, 2, 2)), np.ones((5, 2, 2))
    rc, out, msg = call_rhat(mhx, hm, hv, [10, 10, 10, 8, 6])
    assert rc == capi.EINVAL and "chain 3" in msg and (out == -7.0).all()
    assert call_rhat(mhx, hm, hv, [10, 11, 10, 11, 10])[0] == capi.OK      # the same halves of 5
    for short in (0, 1, 2, 3):
        rc, out, msg = call_rhat(mhx, hm, hv, [short] * 5)
        assert rc == capi.EINVAL and "chain 0" in msg and (out == -7.0).all()
    assert call_rhat(mhx, hm, hv, [4] * 5)[0] == capi.OK
    rc, _, msg = call_rhat(mhx, hm, hv, [10] * 5, n_chains=0)
    assert rc == capi.EINVAL and msg
    assert call_rhat(mhx, hm, hv, [10] * 5, want_out=False)[0] == capi.OK  # NULL rhat
    assert call_rhat(mhx, hm, hv, [10, 10, 10, 8, 6], want_out=False)[0] == capi.EINVAL
    with pytest.raises(ValueError, match="chain 3"):
        mhx.split_rhat(hm, hv, [10, 10, 10, 8, 6])
