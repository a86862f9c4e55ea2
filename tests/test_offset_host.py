"""Peak models at x far from the origin, on the CPU: the oracle's mirror (the device's bit-for-bit
twin) against a high-precision evaluation of the reference's formulas, held to
1e-12 sum |term| + the ARGUMENT TERM (tests/offset_cases.py: the peak kernels form
t = fma(x, iw, c) with c = fl(-mu iw), whose rounding is a shift of mu by up to |mu| 2^-53; on a
grid the recurrence adds the grid's tolerated departure).  The same vectors go to the device in
tests/test_gpu_offset.py, which asks device == mirror.

Measured here (worst over the 12 vectors, mirror against mpmath at 120 bits, n = 300 / 6000):

    offset, span      |mirror - hp| / sum|term|    / (1e-12 sum|term| + argument term)
    (0, 1)            9.1e-16 / 1.0e-15            0.001
    (2000, 1)         4.6e-12 / 4.9e-12            0.20
    (2000, 1e-3)      4.5e-09 / 5.1e-09            0.20 / 0.26
    (-2000, 1)        4.8e-12 / 5.8e-12            0.20 / 0.24
    (1e5, 1)          3.3e-10 / 3.3e-10            0.30 / 0.32
    (1023.5, 1)       2.1e-12 / 3.2e-12            0.18 / 0.26

while the faithful oracle (plain double, the reference's (x - mu) / w) stays below 3e-15."""
import numpy as np
import pytest

import offset_cases as oc

FORMS = [("recurrence", True, True), ("direct", False, True), ("one grid or none", True, False)]


def mirror_errors(orc, s, th, ref, recurrence, window_grids):
    """|mirror - high precision| per vector, in the given form of the mirror"""
    E = oc.hp()
    op = s.oracle(orc)
    orc.mirror_set_recurrence(recurrence)
    orc.mirror_set_window_grids(window_grids)
    try:
        got = [op.logpost_mirror(t) for t in th]
    finally:
        orc.mirror_set_recurrence(True)
        orc.mirror_set_window_grids(True)
    assert np.isfinite(got).all()
    return np.array(got), np.array([float(abs(E.num(g) - r)) for g, r in zip(got, ref)])


@pytest.mark.parametrize("n", [300, 6000])
@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_mirror_within_the_argument_bound_of_high_precision(orc, off, span, n):
    s, th, ref, scale = oc.two_peak_case(off, span, n)
    E = oc.hp()
    hard = False
    for name, rec, wg in FORMS:
        _, err = mirror_errors(orc, s, th, ref, rec, wg)
        bound = np.array([oc.logpost_bound(s, t, rec) for t in th])
        ratio = err / (oc.REL * scale + bound)
        print("(%g, %g) n = %d, %s: worst |mirror - hp| / sum|term| = %.2e, / bound = %.3f (%s)"
              % (off, span, n, name, (err / scale).max(), ratio.max(), E.name))
        assert (ratio <= 1.0).all(), (off, span, n, name, ratio)
        hard = hard or bool((err > oc.REL * scale).any())
    # the inputs are the hard ones: away from the origin 1e-12 sum |term| alone does NOT hold
    assert hard == ((off, span) != (0.0, 1.0)), (off, span, n)
    # ... and the reference's formulas in plain double are not the problem
    op = s.oracle(orc)
    own = np.array([float(abs(E.num(op.logpost(t)) - r)) for t, r in zip(th, ref)])
    print("(%g, %g) n = %d: worst |oracle - hp| / sum|term| = %.2e" % (off, span, n, (own / scale).max()))
    assert (own <= oc.REL * scale).all(), (off, span, n, own / scale)
    # the scale the bound uses is the oracle's own
    assert np.allclose(scale, [op.abs_terms(t) for t in th], rtol=1e-9)


@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_wide_peaks_go_by_the_recurrence_and_keep_the_bound(orc, off, span):
    s, th, ref, scale = oc.two_peak_wide_case(off, span, 6000)
    rec, e_rec = mirror_errors(orc, s, th, ref, True, True)
    direct, e_dir = mirror_errors(orc, s, th, ref, False, True)
    assert (rec != direct).any()                      # the recurrence really ran
    for got, err, form in ((rec, e_rec, True), (direct, e_dir, False)):
        bound = np.array([oc.logpost_bound(s, t, form) for t in th])
        assert (err <= oc.REL * scale + bound).all(), (off, span, form, err / (oc.REL * scale + bound))
    assert (np.abs(rec - direct) <= 1e-13 * scale + np.array(
        [oc.logpost_bound(s, t, True) - oc.logpost_bound(s, t, False) for t in th])).all()


@pytest.mark.parametrize("off, span", oc.CASES, ids=oc.CASE_IDS)
def test_five_peak_poisson_mirror_within_the_argument_bound(orc, off, span):
    """config 3's kernel (run-time-masked peak loops, one seeding class, the Poisson term): the
    mirror of either form within the bound, the recurrence taken by the wide peaks, the faithful
    oracle within 1e-12 sum |term| alone"""
    s, th, ref, scale = oc.five_peak_case(off, span)
    E = oc.hp()
    rec, e_rec = mirror_errors(orc, s, th, ref, True, True)
    direct, e_dir = mirror_errors(orc, s, th, ref, False, True)
    assert (rec[6:] != direct[6:]).any() and np.array_equal(rec[:6], direct[:6])
    for err, form in ((e_rec, True), (e_dir, False)):
        bound = oc.REL * scale + np.array([oc.logpost_bound(s, t, form) for t in th])
        print("(%g, %g) five peaks, %s: worst |mirror - hp| / sum|term| = %.2e, / bound = %.3f"
              % (off, span, "recurrence" if form else "direct", (err / scale).max(), (err / bound).max()))
        assert (err <= bound).all(), (off, span, form, err / bound)
    assert bool((e_dir > oc.REL * scale).any()) == ((off, span) != (0.0, 1.0))
    op = s.oracle(orc)
    own = np.array([float(abs(E.num(op.logpost(t)) - r)) for t, r in zip(th, ref)])
    assert (own <= oc.REL * scale).all(), (off, span, own / scale)


def test_the_bound_has_no_room_for_a_lost_digit(orc):
    """what the issue asks of the bound: a kernel that loses another factor of ten fails it.  Ten
    times the mirror's own error is outside the bound in every offset case"""
    for off, span in oc.CASES[1:]:
        s, th, ref, scale = oc.two_peak_case(off, span, 300)
        _, err = mirror_errors(orc, s, th, ref, True, True)
        bound = np.array([oc.logpost_bound(s, t, True) for t in th])
        assert (10.0 * err > oc.REL * scale + bound).any(), (off, span)


def test_placing_keeps_what_it_says_it_keeps():
    import problems as pb
    base = pb.two_peak(n=300, seed=1300, bounds=False)
    s, th, _, _ = oc.two_peak_case(2000.0, 1e-3, 300)
    r = oc.roles(s)
    assert r == ["bg0", "bg1", "A", "mu", "w", "A", "mu", "w"]
    assert s.bounds == [None] and s.fns == base.fns
    assert np.array_equal(s.data[0][2], base.data[0][2])                 # sigmas
    keep = [j for j, g in enumerate(r) if g in ("A", "bg0")]
    assert np.array_equal(s.theta_star[keep], base.theta_star[keep])
    assert s.theta_star[1] == 0.0 and (th[:, 1] == 0.0).all()            # no slope, ever
    x = s.data[0][0]
    assert x[0] == 2000.0 and x[-1] == 2000.001 and oc.grid_step(x) != 0.0
    # centres moved by about 2 % of the SPAN, not of their value
    assert 0.0 < np.abs(th[:, 3] - s.theta_star[3]).max() < 0.1 * 1e-3
    # the noise is the origin problem's
    res0 = base.data[0][1] - pb.model_eval_np(pb.GAUSS, (2, 2), base.theta_star, base.data[0][0])
    res1 = s.data[0][1] - pb.model_eval_np(pb.GAUSS, (2, 2), s.theta_star, x)
    assert np.allclose(res0, res1, rtol=0, atol=1e-12)
    # every peaks problem of problems.py can be placed
    for p in (pb.poisson_peaks(n=50), pb.global_fit(n_each=20, n_sets=2)):
        q = oc.place(p, -2000.0, 1.0)
        assert all(b is None for b in q.bounds) and q.d == p.d
        assert all(-2000.0 <= d[0].min() and d[0].max() <= -1999.0 for d in q.data)


def test_high_precision_is_what_it_claims():
    E = oc.hp()
    # 2^-100 is visible next to 1: more than a double's 53 (and a long double's 64 when mpmath is there)
    tiny = E.num(2.0 ** -62)
    assert E.num(1) + tiny != E.num(1)
    v = oc.hp_values(1, (0, 1), [1.0, 2000.0, 0.5], [2000.25])[0]       # (exact inputs: u = 1/2)
    assert abs(float(v) - np.exp(-0.25)) < 1e-15
