"""The yardstick of mhx_get_candidate_scores: include/mhx.h's definition of the score and of the
ranking restated in plain Python.  The terms chi2_k are mhx_get_residuals' (resid_cases.yardstick,
or Engine.residuals called once per candidate); what is new here is their total and the order."""
import math

import numpy as np

KEEP_MAX = 16


def total(chi2_by_fn, bad=False):
    """one candidate's score from its chi2_k in ascending k: added serially to a sum that starts at
    0.0; exactly +inf where a value or residual of a selected function was not finite (`bad`) or
    the total is not finite"""
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for c in chi2_by_fn:
            s = s + np.float64(c)
    return float(s) if (not bad and math.isfinite(s)) else math.inf


def rank(score, keep):
    """(best_index [keep], best_score [keep], n_bad) of one chain's scores [m]: the candidates in
    ascending (score, index) order - ties, the +inf ones too, go to the smaller index; where
    m < keep the remaining entries are index -1 and score +inf"""
    score = [float(s) for s in score]
    assert not any(math.isnan(s) for s in score), "a score is a number or +inf, never a NaN"
    order = sorted(range(len(score)), key=lambda j: (score[j], j))[:keep]
    idx = np.full(keep, -1, dtype=np.int32)
    val = np.full(keep, math.inf)
    idx[:len(order)] = order
    val[:len(order)] = [score[j] for j in order]
    return idx, val, sum(1 for s in score if s == math.inf)


def grid(base, axes):
    """candidate_grid's definition: base [d] with column axes[k][0] replaced by the Cartesian
    product of the axes' values, row-major, the first axis slowest: (cand [m, d], shape)"""
    rows = [list(base)]
    for col, vals in axes:
        rows = [r[:col] + [float(v)] + r[col + 1:] for r in rows for v in vals]
    return np.array(rows, dtype=np.float64), tuple(len(v) for _, v in axes)
