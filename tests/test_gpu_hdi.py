"""Highest-density intervals and quantile ladders of every chain on the device (mhx_get_hdi,
mhx_get_derived_hdi and their group forms; Engine.hdi, walker_set_hdi, walker_set_quantiles).  The
histories are injected; the yardstick is tests/hdi_cases.py's numpy statement of the definition on
the very steps that were injected.  Every comparison is on the float bits and covers ALL chains,
columns and outputs of its engine - but lo, hi and pos of a column that is not finite, which the
definition leaves unspecified."""
import ctypes as C
import warnings

import numpy as np
import pytest

import autocorr_cases as ac
import hdi_cases as hd
import histo_cases as hc
from test_gpu_walker_set_get import crafted_walk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def as_walker(mhx, e):
    keys = ["p%d" % j for j in range(e.d)]
    return mhx.Walker(e, None, keys, None, None, None, None), keys


@pytest.mark.parametrize("take", hd.TAKES)
def test_crafted_histories_every_chain_column_and_output_d2(mhx, take):
    """300 chains, d = 2, ring 2048, walks of 1 to 2048 steps of kinds 0-5: windows of one step,
    two, and on either side of a power of two; spans from 0 (a mass of a thousandth of a per cent)
    to the whole window; ladders shorter and longer than the window"""
    walks = hd.d2_walks()
    for ladder in hd.LADDERS:
        got = hd.lds_results(mhx)["d2_%d_%d" % (take, ladder)]
        want = hd.want_hdi(hd.windows_of(walks, take), [0, 1], hd.MASSES, ladder)
        assert hd.same(got, want) is None, ladder
        assert (got["status"] == 0).all() and got["ladder"].shape == (300, 2, ladder)
    assert np.array_equal(got["n_used"], [min(take, len(pr)) for pr, _ in walks])
    assert (got["pos"][:, 5] == 0).all() and np.array_equal(got["lo"][:, 5], got["hi"][:, 5])     # g = 0
    if take >= 57:      # the inputs hold ties of least width and winners away from j = 0 (spans above 0)
        tied, away = want["ties"][:, :5] > 1, want["pos"][:, :5] > 0
        assert tied.any() and away.any() and (tied & away).any()


def test_crafted_histories_wide_vector_columns_out_of_order_d33(mhx):
    walks = hd.d33_walks()
    for take in hd.TAKES:
        got = hd.lds_results(mhx)["d33_%d" % take]
        want = hd.want_hdi(hd.windows_of(walks, take), hd.COLS33, hd.MASSES, 101)
        assert hd.same(got, want) is None, take
    assert len(walks) == 40 and got["lo"].shape == (40, 6, 3)
    got = hd.lds_results(mhx)["d33_all_57"]
    assert hd.same(got, hd.want_hdi(hd.windows_of(walks, 57), list(range(33)), hd.MASSES, 2)) is None


def test_a_ring_that_has_wrapped(mhx):
    e = ac.wrapped_engine(mhx)
    for take in (1000, 1024):
        windows = hc.traces(e, take)
        assert all(len(th) == take for th in windows)
        got = e.hdi(take, hd.MASSES, [1, 0], 101)
        assert hd.same(got, hd.want_hdi(windows, [1, 0], hd.MASSES, 101)) is None, take
        assert (got["n_used"] == take).all() and (got["hi"] >= got["lo"]).all()
    e.close()


def test_windows_that_cannot_fit_lds(mhx):
    """take 8192 at three columns is 196 608 bytes of keys, above a CU's 160 KiB whatever the
    layout: the memory path without its switch.  Windows of two chunks of keys, one step short of
    them, an odd length, one step more than a chunk, exactly a chunk, and one step.  Then one column
    of a ring of 32768 steps: merges whose passes cross several chunks."""
    rng = np.random.default_rng(8192)
    lengths = [8192, 8191, 5000, 4097, 4096, 1]
    walks = [crafted_walk(rng, n, 3, c % 6) for c, n in enumerate(lengths)]
    e = hc.line_engine(mhx, 6, d=3, used=(0, 1), history_capacity=8192)
    e.init_chains([-1.0, 2.0, 0.5])
    assert e.history_capacity() == 8192
    for c, (pr, th) in enumerate(walks):
        e.set_history(c, pr, th)
    for take, cols in ((8192, [0, 1, 2]), (8192, [2, 0, 1]), (5000, [0, 1, 2])):
        got = e.hdi(take, hd.MASSES, cols, 4096)
        assert hd.same(got, hd.want_hdi(hd.windows_of(walks, take), cols, hd.MASSES, 4096)) is None, (take, cols)
        assert got["n_used"].tolist() == [min(n, take) for n in lengths]
    e.close()
    # (values to a quarter: long runs of equal keys)
    long_walks = [(rng.normal(-5.0, 1.0, n), np.round(rng.normal(0.0, 50.0, (n, 2)) * 4) / 4) for n in (32768, 20000)]
    e = hc.line_engine(mhx, 2, history_capacity=32768)
    e.init_chains([-1.0, 2.0])
    for c, (pr, th) in enumerate(long_walks):
        e.set_history(c, pr, th)
    got = e.hdi(32768, hd.MASSES, [1], 4096)
    assert hd.same(got, hd.want_hdi(hd.windows_of(long_walks, 32768), [1], hd.MASSES, 4096)) is None
    assert got["n_used"].tolist() == [32768, 20000]
    e.close()


def test_sorting_in_memory_gives_the_bits_of_lds(mhx, tmp_path_factory):
    """the crafted d = 2 and d = 33 cases a second time, in a child process with MHX_HDI_NO_LDS=1:
    the same bytes, output by output"""
    here, child = hd.lds_results(mhx), hd.no_lds_results(tmp_path_factory)
    assert set(here) == set(child) and len(here) == len(hd.TAKES) * (len(hd.LADDERS) + 1) + 1
    for name in here:
        assert sorted(child[name]) == sorted(here[name])
        for k in here[name]:
            assert child[name][k].tobytes() == here[name][k].tobytes(), (name, k)


def beyond_one_portion(mhx, d, ring, take, cols, ladder, key_pitch, theta0):
    """the smallest chain count that needs two portions, by carve_hdi's own answer; chain c carries
    walk c % 40; a group of twice the chains on the same device equals the single engine"""
    rng = np.random.default_rng(4000)
    period, nc = 40, len(cols)
    per_chain = sum(hd.carve_need(nc, 1, ladder, take, 0, key_pitch))
    per_portion = hd.portion(nc, 1, ladder, take, 0, key_pitch)
    assert per_portion == ((1 << 26) - 8 * 256) // per_chain
    n = per_portion + 1
    n += -n % period                                    # (a whole number of periods: 2n is one too)
    assert -(-n // per_portion) == 2
    walks = [crafted_walk(rng, 1 + k % 8, d, k % 6) for k in range(period)]
    e = hc.line_engine(mhx, n, d=d, used=(0, 1), history_capacity=ring)
    g = mhx.Group(2 * n, d, 1, devices=[0, 0], history_capacity=ring)
    g.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    g.set_dataset(0, hc.LF_X, hc.LF_Y, np.full(5, 0.2))
    assert g.ranges == [(0, n), (n, n)]
    for obj in (e, g):
        obj.init_chains(theta0)
    for part, (first, count) in zip([e] + g.engines, [(0, n)] + g.ranges):
        for c in range(count):
            part.set_history(c, *walks[(first + c) % period])
    single, whole = e.hdi(take, [(50, 1)], cols, ladder), g.hdi(take, [(50, 1)], cols, ladder)
    want = hd.want_hdi(hd.windows_of(walks, take), cols, [(50, 1)], ladder)
    assert hd.same({k: v[:period] for k, v in single.items()}, want) is None
    for k in single:
        a, b = single[k], whole[k]
        assert a.shape[0] == n and b.shape[0] == 2 * n, k
        assert a.tobytes() == a[np.arange(n) % period].tobytes(), k          # either side of the boundary
        assert b.tobytes() == b[np.arange(2 * n) % period].tobytes(), k
        assert b[:n].tobytes() == a.tobytes(), k
    e.close()
    g.close()
    return n, per_portion


def test_chains_beyond_one_portion_sorted_in_lds(mhx):
    """two columns with ladders of 4096 ranks: 65 588 bytes a chain, 1023 chains a portion"""
    n, per_portion = beyond_one_portion(mhx, 2, 8, 8, [1, 0], 4096, 0, [-1.0, 2.0])
    assert per_portion == 1023 and n == 1040


def test_chains_beyond_one_portion_sorted_in_memory(mhx):
    """three columns of a window of 8192 steps: 196 608 bytes of keys a chain, 341 chains a portion"""
    n, per_portion = beyond_one_portion(mhx, 3, 8192, 8192, [2, 0, 1], 0, 8192, [-1.0, 2.0, 0.5])
    assert per_portion == 341 and n == 360


def test_values_that_are_not_finite(mhx):
    walks = hd.nonfinite_walks()
    e = hc.line_engine(mhx, 5, d=3, used=(0, 1), history_capacity=64)
    e.init_chains([-1.0, 2.0, 0.5])
    for c, (pr, th) in enumerate(walks):
        e.set_history(c, pr, th)
    for cols in ([0, 1, 2], [2, 0], [1]):
        got = e.hdi(40, hd.MASSES, cols, 40)
        want = hd.want_hdi(hd.windows_of(walks, 40), cols, hd.MASSES, 40)
        marked = hd.NONFINITE_HIT[:, cols]
        assert np.array_equal(got["status"] != 0, marked) and set(np.unique(got["status"])) <= {0, mhx.capi.HDI_NONFINITE}
        assert hd.same(got, want) is None, cols         # the other columns' bits, and every ladder
        # what is unspecified still lies in range and in the window
        g = np.array([hd.span(40, *m) for m in hd.MASSES])
        assert (got["pos"] >= 0).all() and (got["pos"] + g[None, :, None] <= 39).all()
    lad = hd.bits(e.hdi(40, [], [0, 2], 40))["ladder"]
    assert (lad[1, 0, 39] == hd.NAN_BITS) and np.isfinite(lad[1, 0, :39].view(np.float64)).all()    # the NaN last
    assert lad[4, 0, 39] == hd.NAN_BITS and lad[4, 0, 38].view(np.float64) == np.inf    # a NaN of either sign
    assert lad[4, 1, 0].view(np.float64) == -np.inf and lad[3, 1, 39].view(np.float64) == np.inf
    e.close()


def test_derived_quantities(mhx):
    """two expressions over a crafted history, one of them with prob, against the yardstick on
    mhx_get_derived's own values; the same through a group"""
    rng = np.random.default_rng(107)
    lengths = [1, 2, 9, 300, 1024, 700, 57]
    e = hc.line_engine(mhx, len(lengths), history_capacity=1024)
    g = mhx.Group(len(lengths), 2, 1, devices=[0, 0], history_capacity=1024)
    g.set_function(0, mhx.capi.MODEL_POLY, (), [0, 1])
    g.set_dataset(0, hc.LF_X, hc.LF_Y, np.full(5, 0.2))
    for obj in (e, g):
        obj.init_chains([-1.0, 2.0])
    walks = [crafted_walk(rng, n, 2, c % 6) for c, n in enumerate(lengths)]
    for part, (first, count) in zip([e] + g.engines, [(0, len(lengths))] + g.ranges):
        for c in range(count):
            part.set_history(c, *walks[first + c])
    exprs, names, index = ["a * b * sqrt(3.14159265358979323846)", "prob + abs(b)", "1 / (a - a)"], ["a", "b"], [0, 1]
    for take in (1, 57, 1000):
        r = e.derived(exprs, names, index, take, values=True)
        windows = [r["values"][c][:, :r["n_used"][c]] for c in range(len(lengths))]
        want = hd.want_hdi(windows, None, hd.MASSES, 101)
        got = e.derived_hdi(exprs, names, index, take, hd.MASSES, 101)
        assert hd.same(got, want) is None, take
        assert np.array_equal(got["status"], r["status"]) and np.array_equal(got["n_used"], r["n_used"])
        assert (got["status"][:, :2] == 0).all() and (got["status"][:, 2] == 1).all()     # 1 / 0 is not finite
        whole = g.derived_hdi(exprs, names, index, take, hd.MASSES, 101)
        assert all(whole[k].tobytes() == got[k].tobytes() for k in ("ladder", "n_used", "status")), take
        assert hd.same(whole, want) is None, take
    # an unknown identifier is refused as mhx_get_derived refuses it
    with pytest.raises(mhx.MhxError) as there:
        e.derived(["a + nosuch"], names, index, 10)
    with pytest.raises(mhx.MhxError) as here:
        e.derived_hdi(["a + nosuch"], names, index, 10, [95])
    assert here.value.code == there.value.code == mhx.capi.EINVAL and "'nosuch'" in str(here.value)
    e.close()
    g.close()


def test_arguments_through_the_abi(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    n, d, nm, L = 3, 2, 2, 5
    e = hc.line_engine(mhx, n, history_capacity=64)
    _c, cols = capi.as_i32([1, 0])
    _n, num = capi.as_i32([95, 1365])
    _d, den = capi.as_i32([1, 20])
    f64 = {k: np.full(shape, -7.0) for k, shape in (("lo", (n, nm, 2)), ("hi", (n, nm, 2)), ("ladder", (n, 2, L)))}
    i32 = {k: np.full(shape, -7, dtype=np.int32) for k, shape in (("pos", (n, nm, 2)), ("n_used", n), ("status", (n, 2)))}
    outs = [f64["lo"].ctypes.data_as(capi.f64p), f64["hi"].ctypes.data_as(capi.f64p),
            i32["pos"].ctypes.data_as(capi.i32p), f64["ladder"].ctypes.data_as(capi.f64p),
            i32["n_used"].ctypes.data_as(capi.i32p), i32["status"].ctypes.data_as(capi.i32p)]

    def call(take=10, cols_=cols, n_cols=2, num_=num, den_=den, n_mass=nm, ladder=L, outs_=outs, h=None,
             fn=lib.mhx_get_hdi):
        rc = fn(e._h if h is None else h, take, cols_, n_cols, num_, den_, n_mass, ladder, *outs_)
        return rc, lib.mhx_last_error().decode()

    def untouched():
        return all((a == -7).all() for a in list(f64.values()) + list(i32.values()))

    assert call()[0] == capi.ESTATE and untouched()       # before mhx_init_chains
    e.init_chains([-1.0, 2.0])
    ring = e.history_capacity()

    def refused(**kw):
        rc, msg = call(**kw)
        assert rc == capi.EINVAL and msg and untouched(), kw
        return msg

    refused(take=0)
    refused(take=ring + 1)
    refused(n_cols=0)
    refused(n_cols=d + 1)
    refused(cols_=None)
    for bad in ([1, 1], [0, d], [-1, 0]):
        refused(cols_=capi.as_i32(bad)[1])
    refused(n_mass=-1)
    refused(n_mass=capi.MAX_HDI_MASSES + 1)
    refused(num_=None)
    refused(den_=None)
    for bad_num, bad_den in (([0, 95], [1, 1]), ([95, 101], [1, 1]), ([95, 95], [1, 0]), ([95, 95], [1, 10 ** 6 + 1]),
                             ([-5, 95], [1, 1]), ([95, 2001], [1, 20])):
        refused(num_=capi.as_i32(bad_num)[1], den_=capi.as_i32(bad_den)[1])
    for bad in (1, -1, capi.MAX_HDI_LADDER + 1):
        refused(ladder=bad)
    assert lib.mhx_get_hdi(None, 10, cols, 2, num, den, nm, L, *outs) == capi.EINVAL
    assert lib.mhx_group_get_hdi(None, 10, cols, 2, num, den, nm, L, *outs) == capi.EINVAL and untouched()
    assert call(outs_=[None] * 6)[0] == capi.OK           # every output may be NULL
    for k in range(6):                                    # ... and each one alone
        assert call(outs_=[o if j != k else None for j, o in enumerate(outs)])[0] == capi.OK
    # the one step every chain has: every interval and every rank is that step
    assert call()[0] == capi.OK
    assert (i32["n_used"] == 1).all() and (i32["pos"] == 0).all() and (i32["status"] == 0).all()
    for a in (f64["lo"], f64["hi"]):
        assert (a[:, :, 0] == 2.0).all() and (a[:, :, 1] == -1.0).all()          # cols = [1, 0]
    assert (f64["ladder"][:, 0] == 2.0).all() and (f64["ladder"][:, 1] == -1.0).all()
    # no mass, a ladder alone; the greatest ladder and the greatest count of masses
    lad = np.full((n, 2, 2), -7.0)
    assert call(n_mass=0, num_=None, den_=None, ladder=2,
                outs_=[None, None, None, lad.ctypes.data_as(capi.f64p), None, None])[0] == capi.OK
    assert (lad[:, 0] == 2.0).all() and (lad[:, 1] == -1.0).all()
    assert call(n_mass=0, ladder=0, outs_=[None] * 6)[0] == capi.OK
    assert call(ladder=capi.MAX_HDI_LADDER, outs_=[None] * 6)[0] == capi.OK
    eight = capi.as_i32([95] * 8)[1], capi.as_i32([1] * 8)[1]
    assert call(num_=eight[0], den_=eight[1], n_mass=8, outs_=[None] * 6)[0] == capi.OK
    # a history of four steps: the spans of 95 and 68.25 per cent are 3 and 2
    e.set_history(1, [-1.0, -2.0, -3.0, -4.0], [[1.0, 8.0], [2.5, 8.0], [2.0, 8.0], [4.0, 8.0]])
    assert call()[0] == capi.OK and i32["n_used"].tolist() == [1, 4, 1]
    assert f64["lo"][1, :, 1].tolist() == [1.0, 1.0] and f64["hi"][1, :, 1].tolist() == [4.0, 2.5]
    assert i32["pos"][1].tolist() == [[0, 0], [0, 0]] and f64["ladder"][1, 1].tolist() == [1.0, 1.0, 2.0, 2.5, 4.0]
    e.close()
    # the derived form and the group forms refuse alike
    g = mhx.Group(4, 2, 1, devices=[0, 0])
    assert call(h=g._h, fn=lib.mhx_group_get_hdi)[0] == capi.ESTATE
    ex, nmz, idx = (C.c_char_p * 1)(b"a"), (C.c_char_p * 2)(b"a", b"b"), capi.as_i32([0, 1])[1]
    for fn, h in ((lib.mhx_get_derived_hdi, None), (lib.mhx_group_get_derived_hdi, None)):
        assert fn(h, ex, 1, nmz, idx, 2, 10, num, den, nm, L, *[None] * 6) == capi.EINVAL
    assert lib.mhx_group_get_derived_hdi(g._h, ex, 1, nmz, idx, 2, 10, num, den, nm, L, *[None] * 6) == capi.ESTATE
    g.close()
    e = hc.line_engine(mhx, n, history_capacity=64)
    assert lib.mhx_get_derived_hdi(e._h, ex, 1, nmz, idx, 2, 10, num, den, nm, L, *[None] * 6) == capi.ESTATE
    e.init_chains([-1.0, 2.0])
    for kw in (dict(n_expr=0), dict(n_expr=17), dict(take=0), dict(take=ring + 1), dict(n_mass=9), dict(ladder=1)):
        a = dict(n_expr=1, take=10, n_mass=nm, ladder=L)
        a.update(kw)
        assert lib.mhx_get_derived_hdi(e._h, ex, a["n_expr"], nmz, idx, 2, a["take"], num, den, a["n_mass"],
                                       a["ladder"], *[None] * 6) == capi.EINVAL, kw
    assert lib.mhx_get_derived_hdi(e._h, ex, 1, nmz, idx, 2, 10, num, den, nm, L, *[None] * 6) == capi.OK
    e.close()


def test_the_python_surface(mhx):
    walks = hd.d2_walks()[:23]
    e = hd.engine_of(mhx, walks, history_capacity=2048)
    w, keys = as_walker(mhx, e)
    take = 1000
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # nothing reaches past the ring
        whole = mhx.walker_set_hdi(w, 95, None, take)
        quant = mhx.walker_set_quantiles(w, 101, None, take)
    want = hd.want_hdi(hd.windows_of(walks, take), [0, 1], [(95, 1), (1365, 20)], 101)
    assert len(whole) == len(quant) == e.n_chains
    for c in range(e.n_chains):
        assert list(whole[c]) == list(quant[c]) == keys
        for j, k in enumerate(keys):
            assert np.array(whole[c][k]).view(np.uint64).tolist() == [want["lo"][c, 0, j], want["hi"][c, 0, j]]
            assert np.array_equal(quant[c][k].view(np.uint64), want["ladder"][c, j])
    for c in (0, 7, 22):
        one = mhx.walker_hdi(w, (1365, 20), ["p1"], take, chain=c)
        assert list(one) == ["p1"]
        assert np.array(one["p1"]).view(np.uint64).tolist() == [want["lo"][c, 1, 1], want["hi"][c, 1, 1]]
    assert list(mhx.walker_set_quantiles(w, 2, ["p1"], take)[5]) == ["p1"]
    # the new selectors of walker_exp_get, against the yardstick on the expression's own values
    exp = "(* :p0 :p1 (sqrt pi))"
    values = mhx.walker_set_exp_get(w, exp, ":values", take)
    want = hd.want_hdi([v[None, :] for v in values], None, [(95, 1)], 11)
    intervals = mhx.walker_set_exp_get(w, exp, (":hdi", 95), take)
    ladders = mhx.walker_set_exp_get(w, exp, (":quantiles", 11), take)
    for c in range(e.n_chains):
        assert np.array(intervals[c]).view(np.uint64).tolist() == [want["lo"][c, 0, 0], want["hi"][c, 0, 0]]
        assert np.array_equal(ladders[c].view(np.uint64), want["ladder"][c, 0])
    assert mhx.walker_exp_get(w, exp, (":hdi", 95), take, chain=9) == intervals[9]
    assert np.array_equal(mhx.walker_exp_get(w, exp, (":quantiles", 11), take, chain=9), ladders[9])
    with pytest.raises(mhx.MhxError):                     # a mass of 0 per cent is refused by the library
        mhx.walker_set_exp_get(w, exp, (":hdi", 0), take)
    # Engine.hdi: masses as numbers, all columns by default, no ladder unless asked for
    r = e.hdi(take, [95, (1365, 20)])
    assert r["lo"].shape == (23, 2, 2) and r["ladder"].shape == (23, 2, 0)
    assert np.array_equal(r["lo"].view(np.uint64), hd.want_hdi(hd.windows_of(walks, take), [0, 1], [(95, 1), (1365, 20)])["lo"])
    # a window longer than the ring warns as walker_set_get does
    e.many_steps(2100, np.diag([0.05, 0.05]))
    with pytest.warns(mhx.walker.HistoryTruncated):
        mhx.walker_set_hdi(w, 95, None, 4000)
    e.close()
