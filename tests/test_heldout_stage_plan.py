"""CPU checks of the host-pure half of mhx_get_heldout (csrc/mhx_heldout.hpp), driven as
tests/test_hdi_stage_plan.py drives its header: a small program compiled against the header
(tests/heldout_cases.py has it) answers on the CPU.  The prepared ys, w and c are the bits of
tests/waic_cases.py's constants - what mhx_set_dataset forms - for every shape of y and sigma,
chunk by chunk and chain range by chain range; a refusal names the index in the caller's array; a
portion's carved bytes stay within the budget, its pieces lie in the engine's order without
reaching into each other, and by the planner's accounting one more chain would not fit.  The same
program is built once more with the address and undefined-behaviour sanitizers and asked again."""
import itertools

import numpy as np
import pytest

import heldout_cases as hc
import waic_cases as wc

B = 1 << 26
C_, M_ = 5, 37


@pytest.fixture(scope="module", autouse=True)
def built():
    yield
    hc.cleanup()


def data(seed=0):
    rng = np.random.default_rng(seed)
    y = rng.normal(2.0, 3.0, (C_, M_))
    return {"y": y, "counts": rng.poisson(6.0, (C_, M_)).astype(np.float64),
            hc.SIGMA_NONE: None, hc.SIGMA_SHARED: rng.uniform(0.1, 2.0, M_),
            hc.SIGMA_PER_CHAIN: rng.uniform(0.1, 2.0, C_), hc.SIGMA_PER_POINT: rng.uniform(0.1, 2.0, (C_, M_)),
            "use": (rng.random((C_, M_)) < 0.5).astype(np.uint8) * 7}


def expected(lik, d, kind, per_chain, c0, n, m0, mc, logfact_double=False):
    """(kinds, ys, w, c) [n, mc] each as mhx_set_dataset would form them, row by row"""
    rows = hc.sigma_rows(d[kind], kind, C_, M_)[c0:c0 + n, m0:m0 + mc]
    y = d["counts" if lik == wc.POISSON else "y"]
    ys_raw = (y[c0:c0 + n] if per_chain else np.repeat(y[:1], n, axis=0))[:, m0:m0 + mc]
    by_y = hc.PLANE if per_chain else hc.SHARED
    by_sigma = {hc.SIGMA_NONE: hc.ONE, hc.SIGMA_SHARED: hc.SHARED, hc.SIGMA_PER_CHAIN: hc.SCALAR,
                hc.SIGMA_PER_POINT: hc.PLANE}[kind]
    if lik == wc.POISSON:
        c = np.array([wc.poisson_constants(r, logfact_double) for r in ys_raw])
        return (by_y, hc.ONE, by_y), ys_raw, np.zeros_like(ys_raw), c
    if lik == wc.EXPR:
        return (by_y, by_sigma, hc.NONE), ys_raw, rows, None
    w = 1.0 / rows
    c = np.array([wc.normal_constants(r) for r in rows])
    ys_kind = hc.PLANE if per_chain or by_sigma in (hc.SCALAR, hc.PLANE) else hc.SHARED
    return (ys_kind, by_sigma, by_sigma), ys_raw * w, w, c


def spread(a, kind, n, mc):
    """an array of its kind as [n, mc]"""
    if kind == hc.ONE:
        return np.full((n, mc), a[0])
    if kind == hc.SHARED:
        return np.repeat(a[None, :], n, axis=0)
    if kind == hc.SCALAR:
        return np.repeat(a[:, None], mc, axis=1)
    return a.reshape(n, mc)


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_prepared_arrays_are_the_datasets_own_bits(sanitize):
    d = data()
    ranges = [(0, C_, 0, M_), (1, 3, 5, 20), (4, 1, 36, 1), (0, 1, 0, 1)]
    for lik, kind, per_chain, use_kind in itertools.product(
            (wc.NORMAL, wc.CUTOFF, wc.POISSON, wc.EXPR), range(4), (False, True), (0, 1, 2)):
        y = d["counts" if lik == wc.POISSON else "y"]
        use = None if use_kind == 0 else d["use"][0] if use_kind == 1 else d["use"]
        for c0, n, m0, mc in (ranges if not sanitize else ranges[1:3]):
            where = (lik, kind, per_chain, use_kind, c0, n, m0, mc)
            kinds, extra, ys, w, c, us = hc.ask_fill(lik, lik == wc.POISSON and kind % 2 == 1, y if per_chain else y[0],
                                                     d[kind], kind, use, C_, M_, c0, n, m0, mc, sanitize=sanitize)
            want_kinds, wys, ww, wcst = expected(lik, d, kind, per_chain, c0, n, m0, mc,
                                                 logfact_double=lik == wc.POISSON and kind % 2 == 1)
            assert tuple(kinds[:3]) == want_kinds and kinds[3] == (hc.NONE, hc.SHARED, hc.PLANE)[use_kind], where
            for got, k in ((ys, kinds[0]), (w, kinds[1]), (c, kinds[2]), (us, kinds[3])):
                assert got.size == hc.elems(k, n, mc), where
            assert extra == [mc if kinds[1] == hc.PLANE else 1 if kinds[1] == hc.SCALAR else 0,
                             int(kinds[1] in (hc.SHARED, hc.PLANE)),
                             mc if kinds[0] == hc.PLANE else 0, int(kinds[2] in (hc.SHARED, hc.PLANE))], where
            assert wc.same_bits(spread(ys, kinds[0], n, mc), wys), where
            assert wc.same_bits(spread(w, kinds[1], n, mc), ww), where
            if wcst is not None:
                assert wc.same_bits(spread(c, kinds[2], n, mc), wcst), where
            if use is not None:
                want_use = (use[c0:c0 + n] if use_kind == 2 else np.repeat(use[None, :], n, axis=0))[:, m0:m0 + mc] != 0
                assert np.array_equal(spread(us, kinds[3], n, mc) != 0, want_use), where
                assert set(us.tolist()) <= {0, 1}, where


def test_refusals_name_the_index_in_the_callers_array():
    d = data(1)
    ok = hc.ask_validate(wc.NORMAL, d["y"], d[hc.SIGMA_PER_POINT], hc.SIGMA_PER_POINT, C_, M_)
    assert ok == (0, "")
    for kind, index in ((hc.SIGMA_SHARED, 3), (hc.SIGMA_PER_CHAIN, 4), (hc.SIGMA_PER_POINT, 2 * M_ + 3)):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            s = np.array(d[kind], dtype=np.float64)
            s.reshape(-1)[index] = bad
            for lik in (wc.NORMAL, wc.CUTOFF):
                rc, msg = hc.ask_validate(lik, d["y"], s, kind, C_, M_)
                assert rc == -1 and msg.startswith("sigma[%d] = " % index) and "finite and > 0" in msg, (kind, bad, msg)
            # an expression likelihood's `error` is handed over untouched, and Poisson reads no sigma
            assert hc.ask_validate(wc.EXPR, d["y"], s, kind, C_, M_)[0] == 0
            assert hc.ask_validate(wc.POISSON, d["counts"], s, kind, C_, M_)[0] == 0
    for bad in (-1.0, 2.5, float("nan"), 2e9):
        y = d["counts"].copy()
        y[3, 7] = bad
        rc, msg = hc.ask_validate(wc.POISSON, y, None, hc.SIGMA_NONE, C_, M_)
        assert rc == -1 and msg.startswith("poisson count y[%d] = " % (3 * M_ + 7)), msg
        rc, msg = hc.ask_validate(wc.POISSON, y[3], None, hc.SIGMA_NONE, C_, M_)
        assert rc == -1 and msg.startswith("poisson count y[7] = "), msg
        assert hc.ask_validate(wc.NORMAL, y, None, hc.SIGMA_NONE, C_, M_)[0] == 0      # (a normal y is any number)


def test_portions_stay_within_the_budget_and_one_more_chain_would_not_fit():
    shapes = []
    for m, want, ys, w, c, use in itertools.product((1, 257, 1000, 1 << 17), (0, 1, 2, 3), (hc.SHARED, hc.PLANE),
                                                    (hc.ONE, hc.SHARED, hc.SCALAR, hc.PLANE),
                                                    (hc.NONE, hc.ONE, hc.PLANE), (hc.NONE, hc.SHARED, hc.PLANE)):
        for nb in ((m + 255) // 256, 4 * ((m + 255) // 256) + 1):      # (the call's blocks: this chunk's, or more)
            shapes.append((nb, want, ys, w, c, use, m))
    answers = hc.ask("".join("C %d %d %d %d %d %d %d\n" % s for s in shapes))
    assert len(answers) == len(shapes)
    for shape, line in zip(shapes, answers):
        nb, want, ys, w, c, use, m = shape
        fixed, per = hc.carve_need(nb, want, (ys, w, c, use), m)
        head, *carvings = line.split("|")
        P, fits = (int(t) for t in head.split())
        slack = 256 * len(per)
        assert fits == int(sum(fixed) + sum(per) + slack <= B) == 1, (shape, line)     # one chain always fits
        assert P == (B - sum(fixed) - slack) // sum(per) >= 1, (shape, line)
        assert sum(fixed) + (P + 1) * sum(per) + slack > B, (shape, line)               # one more would not
        for n, carving in zip((1, P), carvings):
            total, *off = (int(t) for t in carving.split())
            assert len(off) == len(per) == 14 and "PIECES" not in line, (shape, line)
            assert all(o % 256 == 0 for o in off) and off[0] == 0, (shape, n, off)
            for k in range(len(off)):
                end = off[k + 1] if k + 1 < len(off) else total
                assert off[k] + fixed[k] + n * per[k] <= end, (shape, n, k, off)
            assert total <= B, (shape, n, total)
    # the house shape with everything per chain and every output: 4096 chains go in portions
    fixed, per = hc.carve_need(4, 3, (hc.PLANE, hc.PLANE, hc.PLANE, hc.PLANE), 1000)
    line = hc.ask("C 4 3 4 4 4 4 1000\n")[0]
    # (65 068 bytes a chain - 65 a point and 68 of totals and block sums - beside 16 000 of x)
    assert sum(per) == 65068 and sum(fixed) == 16000
    assert int(line.split()[0]) == (B - 16000 - 256 * 14) // 65068 == 1031
