"""CPU checks around mhx_get_heldout: the constants and signatures of the binding, kfold_folds,
the exactness of the K-fold layer's power-of-two scaling of sigma, and the numpy yardstick's own
additions to tests/waic_cases.py (tests/heldout_cases.py: the value moments, the mask, the
block-ordered total) on hand cases.  No device is touched."""
import math

import numpy as np
import pytest

import heldout_cases as hc
import waic_cases as wc


@pytest.fixture(scope="module")
def mirror():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def test_constants_and_signatures(mirror):
    capi = mirror.capi
    assert (capi.HELDOUT_NONFINITE, capi.HELDOUT_NO_POINTS) == (hc.NONFINITE, hc.NO_POINTS) == (1, 2)
    assert capi.HELDOUT_BLOCK == hc.BLOCK == wc.BLOCK == capi.WAIC_BLOCK
    for name in ("mhx_get_heldout", "mhx_group_get_heldout"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
    one, grp = capi.SIGNATURES["mhx_get_heldout"], capi.SIGNATURES["mhx_group_get_heldout"]
    assert one == grp and len(one[1]) == 18
    # (handle, fn, take, xcols, n_cols, m, y, y_per_chain, sigma, sigma_kind, use, use_per_chain, then the outputs)
    assert one[1][3] is capi.f64p and one[1][6] is capi.f64p and one[1][8] is capi.f64p and one[1][10] is capi.u8p
    assert [one[1][k] for k in (12, 13, 14, 15, 16, 17)] == [capi.f64p, capi.i32p, capi.f64p, capi.f64p,
                                                              capi.i32p, capi.i32p]
    for name in ("walker_set_score_data", "walker_score_data", "kfold_folds", "walker_set_kfold_create",
                 "walker_set_kfold"):
        assert name in mirror.__all__ and callable(getattr(mirror, name))
    assert callable(mirror.Engine.heldout) and callable(mirror.Group.heldout)
    assert (hc.SIGMA_NONE, hc.SIGMA_SHARED, hc.SIGMA_PER_CHAIN, hc.SIGMA_PER_POINT) == \
        (capi.SIGMA_NONE, capi.SIGMA_SHARED, capi.SIGMA_PER_CHAIN, capi.SIGMA_PER_POINT)


@pytest.mark.parametrize("n", [1, 7, 10, 11])
@pytest.mark.parametrize("K", [1, 2, 3, 10])
def test_kfold_folds(mirror, n, K):
    for scheme in (":interleaved", ":blocks"):
        if K > n:
            with pytest.raises(ValueError):
                mirror.kfold_folds(n, K, scheme)
            continue
        f = mirror.kfold_folds(n, K, scheme)
        assert f.shape == (n,) and f.dtype == np.int32
        sizes = np.bincount(f, minlength=K)
        assert sizes.size == K and sizes.sum() == n and sizes.min() >= 1       # every point in exactly one fold
        assert sizes.max() - sizes.min() <= 1
        if scheme == ":interleaved":
            assert list(f) == [i % K for i in range(n)]
        else:
            assert list(f) == sorted(f)                                         # contiguous runs, in fold order
            assert list(sizes) == sorted(sizes, reverse=True)                   # the longer ones first
            assert list(sizes) == [n // K + (1 if k < n % K else 0) for k in range(K)]
    with pytest.raises(ValueError):
        mirror.kfold_folds(n, K, ":random")
    with pytest.raises(ValueError):
        mirror.kfold_folds(n, 0)


def test_the_power_of_two_scaling_of_sigma_is_exact(mirror):
    """1 / (s 2^400) == (1 / s) 2^-400 and y / (s 2^400) likewise, bit for bit: a held-out point's
    residual is its own times 2^-400, its square 2^-800 of it, and adding that to a sum of training
    terms changes no bit"""
    from lisp_mcmc_amd import walker
    scale = walker.KFOLD_SIGMA_SCALE
    assert scale == 2.0 ** 400 and math.frexp(scale)[0] == 0.5
    rng = np.random.default_rng(400)
    s = np.concatenate([rng.uniform(1e-3, 1e3, 4000), 10.0 ** rng.uniform(-30, 30, 4000)])
    y = rng.normal(0.0, 100.0, s.size)
    v = rng.normal(0.0, 100.0, s.size)
    w, wk = 1.0 / s, 1.0 / (s * scale)
    assert wc.same_bits(wk, w * 2.0 ** -400)
    assert wc.same_bits(y * wk, (y * w) * 2.0 ** -400)
    r, rk = y * w - v * w, y * wk - v * wk
    assert wc.same_bits(rk, r * 2.0 ** -400)
    q = (0.5 * rk) * rk
    assert (q <= np.abs((0.5 * r) * r) * 2.0 ** -799).all()
    # a residual of up to a million sigma: its held-out square is below 2^-760 and vanishes even
    # against a sum of training terms as small as 1e-200
    keep = np.abs(r) < 1e6
    assert keep.sum() > 4000 and (q[keep] < 2.0 ** -760).all()
    total = np.float64(1e-200)
    assert ((total + q[keep]) == total).all() and ((-total - q[keep]) == -total).all()
    # the constant moves by -400 log 2 per held-out point, in one rounding of the logarithm
    c, ck = wc.normal_constants(s[:50]), wc.normal_constants(s[:50] * scale)
    assert np.allclose(ck - c, -400.0 * math.log(2.0), rtol=0, atol=1e-12 * 400)


def test_the_block_ordered_total_on_hand_cases():
    assert hc.block_sum([1.5]) == 1.5 and hc.block_sum(np.zeros(0)) == 0.0
    # 64 lanes hold one point each: the butterfly adds pairs 32 apart first
    v = np.zeros(64)
    v[0], v[32], v[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert hc.block_sum(v) == (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0          # (each addend is lost on its own)
    v[32], v[33] = 0.0, 2.0 ** -53
    assert hc.block_sum(v) == 1.0 + 2.0 ** -52                                 # lanes 1 and 33 meet first
    # a lane adds its own points serially before any lane meets another, blocks go serially after that
    v = np.zeros(600)
    v[0], v[64], v[128], v[256], v[512] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53
    assert hc.block_sum(v) == 1.0
    v[0] = 0.0
    assert hc.block_sum(v) == 4 * 2.0 ** -53
    rng = np.random.default_rng(1)
    for m in (63, 256, 257, 1000):
        pw = rng.normal(-3.0, 2.0, m)
        assert abs(hc.block_sum(pw) - math.fsum(pw)) <= m * 2.0 ** -53 * math.fsum(np.abs(pw))


def test_the_yardstick_masks_and_moments():
    rng = np.random.default_rng(2)
    v = rng.normal(1.0, 0.3, (40, 9))
    y, sig = rng.normal(1.0, 0.5, 9), rng.uniform(0.2, 0.6, 9)
    ell = wc.terms(wc.NORMAL, v, y, sig)
    full = hc.yardstick(ell, v)
    assert full["status"] == 0 and full["n_scored"] == 9
    assert wc.same_bits(full["acc"][:, :2], np.column_stack(wc.accumulate(ell)[:2]))
    assert np.allclose(full["acc"][:, 2], v.mean(axis=0), rtol=1e-14)
    assert np.allclose(full["acc"][:, 3], v.var(axis=0, ddof=0) * 40, rtol=1e-12)
    use = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], dtype=np.uint8)
    some = hc.yardstick(ell, v, use)
    assert some["n_scored"] == 5 and some["status"] == 0
    assert (some["acc"][use == 0] == 0.0).all() and (some["pw_lpd"][use == 0] == 0.0).all()
    assert wc.same_bits(some["acc"][use == 1], full["acc"][use == 1])
    v2 = v.copy()
    v2[3, 1] = np.inf                           # not finite where the chain does not look
    assert hc.yardstick(wc.terms(wc.NORMAL, v2, y, sig), v2, use)["status"] == 0
    assert hc.yardstick(wc.terms(wc.NORMAL, v2, y, sig), v2)["status"] == hc.NONFINITE
    none = hc.yardstick(ell, v, np.zeros(9))
    assert none["status"] == hc.NO_POINTS and none["n_scored"] == 0 and hc.block_sum(none["pw_lpd"]) == 0.0
