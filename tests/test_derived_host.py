"""walker-with-exp (mcmc-fitting.lisp:1052-1064) on the host side of the Python mirror: the
translation of a keyword form into the C text and names mhx_get_derived takes, the two error
classes, and the parsing of walker_exp_get's `get`.  Needs no GPU."""
import pytest

from lisp_mcmc_amd import sexpr
from lisp_mcmc_amd import walker as mirror

PI = "3.14159265358979323846"


class FakeWalker:
    param_keys = ["a1", "mu1", "w1", "a2", "mu2", "w2"]


def test_keyword_forms_become_c_text_and_names():
    assert sexpr.keyword_exp_to_expr("(* :a1 :w1 (sqrt pi))") == (["a1", "w1"], "(a1 * w1 * sqrt(%s))" % PI)
    assert sexpr.keyword_exp_to_expr("(/ :a1 :a2)") == (["a1", "a2"], "(a1 / a2)")
    assert sexpr.keyword_exp_to_expr("(expt :w1 2)") == (["w1"], "ipow(w1, 2)")
    assert sexpr.keyword_exp_to_expr("'(+ :W1 :w1 prob)") == (["w1"], "(w1 + w1 + prob)")
    assert sexpr.keyword_exp_to_expr("(- :much-better-name 1d-3)") == (["much_better_name"],
                                                                       "(much_better_name - 1e-3)")


def test_names_and_places_follow_the_walkers_keys():
    names, index, text = mirror._exp_call(FakeWalker(), "(/ (* :a2 :w2) (* :a1 :w1))")
    assert names == ["a2", "w2", "a1", "w1"] and index == [3, 5, 0, 2]
    assert text == "((a2 * w2) / (a1 * w1))"


def test_a_keyword_that_is_no_parameter_is_a_key_error():
    with pytest.raises(KeyError, match=":nope"):
        mirror._exp_call(FakeWalker(), "(* :a1 :nope)")


def test_an_unsupported_operator_is_a_sexpr_error():
    with pytest.raises(sexpr.SexprError, match="gamma"):
        mirror._exp_call(FakeWalker(), "(gamma :a1)")
    with pytest.raises(sexpr.SexprError, match="whatever"):   # a free symbol has no value here
        mirror._exp_call(FakeWalker(), "(* :a1 whatever)")


def test_get_selectors():
    sel = mirror.exp_selector
    assert sel(":median") == ("median", (50,))
    assert sel("median") == ("median", (50,))
    assert sel(":95cr") == ("95cr", (2.5, 97.5))
    assert sel(":iqr") == ("iqr", (25, 75))
    assert sel(":stddev-normal") == ("stddev-normal", (50, 84.1))
    for g in (":most-likely", ":mean", ":stddev", ":values"):
        assert sel(g) == (g[1:], ())
    assert sel((":percentile", 84.1)) == ("percentile", (84.1,))
    for bad in (":mode", ":percentile", (":median", 3), (":percentile", 101), (":percentile",)):
        with pytest.raises(ValueError):
            sel(bad)
