"""CPU checks of the ensemble percentiles' host half: mhx_ensemble_pick against brute force, a
Python model of the whole eight-pass selection (order keys, mhx_ensemble_pick, the successor rule)
against walker._percentile on the sorted multiset, the ctypes prototypes, and the task bookkeeping
of csrc/mhx_ensemble.hpp through a small compiled program.  tests/test_gpu_ensemble.py holds the
device's side."""
import ctypes as C
import re

import numpy as np
import pytest

import ensemble_cases as ec
import histo_cases as hc


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def brute_pick(counts, rank):
    """the bin of `rank` by laying the bins out one element at a time"""
    digits = np.repeat(np.arange(len(counts)), counts)
    digit = int(digits[rank])
    return digit, rank - int(np.flatnonzero(digits == digit)[0]), int(counts[digit])


def boundary_ranks(counts):
    edges = np.cumsum(counts)
    total = int(edges[-1])
    ranks = {0, total - 1}
    for b in edges:
        ranks.update(r for r in (int(b) - 1, int(b)) if 0 <= r < total)
    return sorted(ranks)


PICK_COUNTS = {
    "dense": [3, 1, 4, 1, 5, 9, 2, 6],
    "empty_before_and_after": [0, 0, 0, 5, 0, 7, 1, 0, 0],
    "single_bin": [0] * 100 + [17] + [0] * 155,
    "one_element": [1],
    "ones": [1] * 256,
    "random": list(np.random.default_rng(7).integers(0, 50, 256)),
}


@pytest.mark.parametrize("name", sorted(PICK_COUNTS))
def test_pick_against_brute_force(mhx, name):
    counts = np.array(PICK_COUNTS[name], dtype=np.int64)
    total = int(counts.sum())
    ranks = range(total) if total <= 600 else boundary_ranks(counts)
    for rank in ranks:
        assert mhx.ensemble_pick(counts, rank) == brute_pick(counts, rank), rank
    for rank in boundary_ranks(counts):      # rank 0, the last, either side of every bin boundary
        assert mhx.ensemble_pick(counts, rank) == brute_pick(counts, rank), rank


def test_pick_counts_above_32_bits(mhx):
    big = 1 << 32
    counts = [0, 3 * big + 1, 0, 5, big, 0, 7 * big, 1]
    edges = np.cumsum([int(c) for c in counts], dtype=object)
    total = int(edges[-1])
    assert total > 11 * big
    for b in range(len(counts)):
        if counts[b] == 0:
            continue
        lo = int(edges[b]) - counts[b]
        for within in {0, counts[b] // 2, counts[b] - 1}:
            assert mhx.ensemble_pick(counts, lo + within) == (b, within, counts[b])
    assert mhx.ensemble_pick(counts, total - 1) == (7, 0, 1)
    assert mhx.ensemble_pick([(1 << 62) + 5, 9], (1 << 62) + 4) == (0, (1 << 62) + 4, (1 << 62) + 5)
    assert mhx.ensemble_pick([(1 << 62) + 5, 9], (1 << 62) + 5) == (1, 0, 9)
    with pytest.raises(ValueError):
        mhx.ensemble_pick(counts, total)


def test_pick_refuses_bad_arguments(mhx):
    capi, lib = mhx.capi, mhx.capi.lib()
    counts = np.array([2, 0, 3], dtype=np.uint64)
    cp = counts.ctypes.data_as(capi.u64p)
    digit, rb, bc = C.c_int32(-7), C.c_int64(-7), C.c_int64(-7)
    outs = (C.byref(digit), C.byref(rb), C.byref(bc))
    for n_bins, rank in ((3, -1), (3, 5), (3, 1 << 40), (0, 0), (-1, 0), (2, 2)):
        assert lib.mhx_ensemble_pick(cp, n_bins, rank, *outs) == capi.EINVAL, (n_bins, rank)
        assert lib.mhx_last_error()
        assert (digit.value, rb.value, bc.value) == (-7, -7, -7)      # untouched on error
    assert lib.mhx_ensemble_pick(None, 3, 0, *outs) == capi.EINVAL
    zeros = np.zeros(4, dtype=np.uint64)
    assert lib.mhx_ensemble_pick(zeros.ctypes.data_as(capi.u64p), 4, 0, *outs) == capi.EINVAL      # an empty pool
    assert lib.mhx_ensemble_pick(cp, 3, 4, None, None, None) == capi.OK                         # outputs may be NULL
    assert lib.mhx_ensemble_pick(cp, 3, 4, *outs) == capi.OK
    assert (digit.value, rb.value, bc.value) == (2, 2, 3)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="rank"):
            mhx.ensemble_pick(counts, bad)


def test_order_keys_sort_as_the_doubles_do():
    v = ec.special_values()
    keys = ec.order_keys(v)
    by_key, by_value = v[np.argsort(keys, kind="stable")], np.sort(v)
    assert np.array_equal(by_key, by_value)                 # (-0 == +0)
    assert all(ec.key_value(k) == x for k, x in zip(keys, v))
    assert all(np.signbit(ec.key_value(k)) == np.signbit(x) for k, x in zip(keys, v))
    nan = ec.order_keys(np.array([np.nan, -np.nan]))
    assert (nan == np.uint64(ec.ALL_ONES)).all() and keys.max() < nan[0]
    assert ec.order_keys(np.array([-0.0]))[0] + np.uint64(1) == ec.order_keys(np.array([0.0]))[0]


@pytest.mark.parametrize("name", sorted(ec.multisets()))
def test_the_eight_pass_model_equals_the_sorted_yardstick(mhx, name):
    values = ec.multisets()[name]
    log = []
    got = ec.model_select(mhx, values, ec.PCTS, log)
    want = ec.yardstick(mhx, values[:, None])[:, 0]
    assert ec.same(got, want), (got, want)
    if name == "equal":                                     # one value: every pass leaves one bin
        assert {occupied for _, occupied in log} == {1}
    if name == "nan_one":                                   # the NaN sorts last: the 100 % point alone
        assert np.isnan(got[ec.PCTS.index(100)]) and np.isfinite(np.delete(got, ec.PCTS.index(100))).all()
    if name == "two":                                       # between ranks of two distinct values
        assert got[ec.PCTS.index(50)] == 0.5 and got[ec.PCTS.index(0)] == -1.0


def test_the_header_and_the_bindings_agree(mhx):
    capi = mhx.capi
    lib = capi.lib()
    header = open(hc.ROOT + "/include/mhx.h").read()
    for name in ("mhx_get_ensemble_percentiles", "mhx_group_get_ensemble_percentiles", "mhx_ensemble_pick"):
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(capi.SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == capi.SIGNATURES[name][1]
    for name in ("ensemble_pick", "walker_set_ensemble_get"):
        assert name in mhx.__all__ and callable(getattr(mhx, name))
    assert callable(mhx.Engine.ensemble_percentiles) and callable(mhx.Group.ensemble_percentiles)
    lisp = open(hc.ROOT + "/lisp-mcmc_amd/lisp/package.lisp").read()
    assert "#:walker-set-ensemble-get" in lisp


def bookkeeping_cases():
    rng = np.random.default_rng(1008)
    sp = ec.special_values()
    cases = []
    for nc, n, pcts, chains in ((1, 1, ec.PCTS, 1), (1, 2, ec.PCTS, 2), (3, 257, ec.PCTS, 11), (2, 1000, [50], 4096),
                                (8, 300, [2.5, 50, 97.5], 65536), (5, 64, [], 3), (63, 40, list(range(0, 96, 6)), 7),
                                (4, 500, [0, 100, 50, 50], 300)):
        pool = rng.normal(0.0, 1.0, (n, nc))
        if nc > 1:
            pool[:, 1] = rng.choice(sp, n)                          # ties, zeros, last-bit neighbours
        if nc > 2:
            pool[:, 2] = np.round(pool[:, 2], 1)                    # long runs of equal values
            pool[rng.integers(0, n), 2] = np.nan
        cases.append((pool, pcts, chains))
    return cases


def test_the_bookkeeping_of_mhx_ensemble_hpp(mhx):
    cases = bookkeeping_cases()
    answers = ec.bookkeeping_answers(cases)
    if answers is None:
        pytest.skip("no g++ to compile against csrc/mhx_ensemble.hpp")
    align = lambda b: (b + 255) & ~255      # noqa: E731
    for (pool, pcts, chains), line in zip(cases, answers):
        n, nc = pool.shape
        m = re.fullmatch(r"tasks ([\d ]+) succ (\d+) pooled (\d+) values([ 0-9a-f]*) carve ([\d ]+)", line)
        assert m, line
        tasks = [int(t) for t in m.group(1).split()]
        assert int(m.group(3)) == n
        # pass 0 counts every column whole; later passes ask once per distinct (column, prefix)
        assert tasks[0] == nc and len(tasks) == (8 if pcts else 1)
        assert tasks[1:] == [ec.distinct_prefixes(pool, pcts, p) for p in range(1, len(tasks))]
        assert max(tasks) <= nc * max(1, len(pcts)) <= 1008
        assert int(m.group(2)) <= nc * len(pcts)
        bits = np.array([int(b, 16) for b in m.group(4).split()], dtype=np.uint64)
        got = bits.view(np.float64).reshape(len(pcts), nc)
        assert ec.same(got, ec.yardstick(mhx, pool, pcts).reshape(len(pcts), nc)), line
        carve = [int(v) for v in m.group(5).split()]
        max_tasks = nc * max(1, len(pcts))
        sizes = [max_tasks * 2048, max_tasks * 16, chains, chains * 4, nc * 4]
        offsets = [0]
        for s in sizes:
            offsets.append(offsets[-1] + align(s))
        assert carve == [max_tasks] + offsets + [1]
    # the greatest call: 1008 tasks of 2 KiB, and a set of 2^20 chains, stay far below the budget
    assert 1008 * 2048 + 1008 * 16 + 5 * (1 << 20) + 63 * 4 < (1 << 26) // 8
