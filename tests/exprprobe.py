"""One value of a run-time compiled expression, read out of the device exactly.

A function given as an expression over a ONE-point dataset (x = 0, y = 0, sigma = 1) whose
likelihood term is the expression `model` itself: mhx_logpost's parts[:, 0] is then f(row) for
every parameter row, bit for bit.  Pads are masked in the MHX_LIK_EXPR sweep, the accumulator
starts at 0.0 and the wave sum adds only +0.0, finish_lik<MHX_LIK_EXPR> returns the sum as it is
and k_logpost writes it unchanged (NaN and +-inf included).  Only the sign of a zero is lost
(0.0 + -0.0 is +0.0).  A function with an MHX_LIK_EXPR likelihood always stays an expression
(include/mhx.h), and with no bounds the prior part is exactly 0.

Write each argument as `a + x` so that the expression is evaluated per point inside the sweep,
as a real model is; a division `(a + x) / b` is the form whose reciprocal the compiler hoists.
Environment switches (MHX_EXPR_EXACT_DIV, MHX_EXPR_OCML_MATH, MHX_FAMILY_WPG ...) are the
caller's: the run-time compiled code is cached by its generated source, so each setting is its
own program.
"""
import numpy as np


def evaluate(mhx, body, names, rows):
    """f(row) for each row of `rows` ([n, len(names)]), f the expression `body` over `names`"""
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, len(names))
    e = mhx.Engine(1, len(names), 1)
    try:
        e.set_expr_recognition(False)
        e.set_function_expr(0, body, list(names), list(range(len(names))))
        e.set_dataset(0, [0.0], [0.0], [1.0], likelihood=mhx.capi.LIK_EXPR)
        e.set_likelihood_expr(0, "model")
        _, parts = e.logpost(rows, parts=True)
        assert "rtc[expr" in e.kernel_name(), e.kernel_name()
    finally:
        e.close()
    assert np.all(parts[:, 1] == 0.0)   # no bounds: the prior adds nothing
    return parts[:, 0].copy()


def select_chain(exprs, selector="s"):
    """`s < 0.5 ? e0 : s < 1.5 ? e1 : ... : e_last`: one program for many routines, row by row
    (only the selected value is returned, so each stays exact)"""
    out = exprs[-1]
    for i in range(len(exprs) - 2, -1, -1):
        out = "(%s < %d.5 ? (%s) : %s)" % (selector, i, exprs[i], out)
    return out
