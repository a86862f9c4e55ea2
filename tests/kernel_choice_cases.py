"""The problems of tests/golden/kernel_choice_cases.csv: one row per problem, its switches, its
functions as tokens, and what mhx_kernel_name() (or the refusal) said when the row was recorded on
the MI355X.  test_finalize_host.py feeds the rows to the choice rules on the CPU,
test_gpu_kernel_choice.py builds the real engines.

A function token is model/s0/s1/n_idx/lik/form/prior/data/x:
  model   poly gauss lorentz (what the function is, or what its expression is recognised as)
  s0, s1  backgrounds and peaks (0/0: a polynomial)
  n_idx   parameters
  lik     normal cutoff poisson expr, or exprnotext (MHX_LIK_EXPR, mhx_set_likelihood_expr never called)
  form    enum, rexpr (an expression that IS the model), expr (one that is not), expr2 (reads xcol1), unset
  prior   1: a prior body
  data    shared cols2 unset, or planes-none -shared -chain -point (a dataset per walker, by sigma kind)
  x       grid (64 points), piecewise (two scans of different steps, 2 x 2048 + 5 points),
          irregular (64), long (a grid of 4 x 2048 + 5 points: the 16-wave family's)"""
import csv
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "kernel_choice_cases.csv")
KNOBS = ["MHX_FORCE_GENERIC", "MHX_NO_RTC_SPECIALISE", "MHX_EARLY_REJECT", "MHX_NO_RECOGNISE",
         "MHX_NO_WINDOW_GRIDS", "MHX_PLANES_NO_LDS", "MHX_FAMILY_WPG"]
FIELDS = ["model", "s0", "s1", "n_idx", "lik", "form", "prior", "data", "x"]
MODELS = {"poly": 0, "gauss": 1, "lorentz": 2}
LIKS = {"normal": 0, "cutoff": 1, "poisson": 2, "expr": 3, "exprnotext": 3}
SIGMA_KINDS = {"none": 0, "shared": 1, "chain": 2, "point": 3}
X_POINTS = {"grid": 64, "irregular": 64, "piecewise": 2 * 2048 + 5, "long": 4 * 2048 + 5}


def rows():
    with open(CASES, newline="") as f:
        out = list(csv.DictReader(f))
    for r in out:
        r["fns"] = [dict(zip(FIELDS, r[c].split("/"))) for c in ("fn0", "fn1") if r[c] != "-"]
        for fn in r["fns"]:
            for k in ("s0", "s1", "n_idx", "prior"):
                fn[k] = int(fn[k])
    return out


def x_of(kind):
    i = np.arange(X_POINTS[kind], dtype=np.float64)
    if kind == "piecewise":
        return np.where(i < 2048, i * 0.01, 20.48 + (i - 2048) * 0.02)
    if kind == "irregular":
        return i * 0.25 + 0.01 * ((i * i) % 7)
    return i * 0.25 if kind == "grid" else i * 0.002


def expr_text(fn):
    """(text, names) of a function given as an expression"""
    if fn["form"] == "expr2":
        return "a*xcol0 + b*xcol1", ["a", "b"]
    assert (fn["model"], fn["s0"], fn["s1"], fn["n_idx"]) == ("gauss", 1, 1, 4)
    return "b0 + a1*exp(-ipow((x - mu1)/w1, %d))" % (2 if fn["form"] == "rexpr" else 4), ["b0", "a1", "mu1", "w1"]


def theta_of(fn, x):
    """finite parameters of one function: backgrounds 0.5, 0.01, 0 ..; peaks of height 1 and width a
    tenth of the range, spread over it"""
    nbg = fn["s0"] if fn["model"] != "poly" else fn["n_idx"]
    th = [0.5, 0.01][:nbg] + [0.0] * max(nbg - 2, 0)
    if fn["form"] == "expr2":
        return [0.5, 0.25]
    span = float(x[-1] - x[0])
    for p in range(fn["s1"]):
        th += [1.0, x[0] + span * (p + 1) / (fn["s1"] + 1), 0.1 * span]
    assert len(th) == fn["n_idx"], (fn, th)
    return th


def build(mhx, row):
    """the engine of a row and one finite parameter vector; raises capi.MhxError where the ABI
    refuses the problem before it is finalised (finalisation itself happens at the first logpost)"""
    capi = mhx.capi
    fns = row["fns"]
    C, d = int(row["chains"]), sum(fn["n_idx"] for fn in fns)
    e = mhx.Engine(C, d, len(fns), seed=3,
                   adapt_mode=capi.ADAPT_POOLED if row["adapt"] == "pooled" else capi.ADAPT_FAITHFUL)
    theta, first = [], 0
    rng = np.random.default_rng(11)
    for k, fn in enumerate(fns):
        index = list(range(first, first + fn["n_idx"]))
        first += fn["n_idx"]
        x = x_of(fn["x"])
        theta += theta_of(fn, x)
        if fn["form"] == "enum":
            shape = (fn["s0"], fn["s1"]) if fn["model"] != "poly" else ()
            e.set_function(k, MODELS[fn["model"]], shape, index)
        elif fn["form"] != "unset":
            text, names = expr_text(fn)
            e.set_function_expr(k, text, names, index)
        if fn["prior"]:
            e.set_prior_expr(k, "bounds_total + (q > 50.0 ? -1e9 : 0.0)", ["q"], [index[0]])
        y = 1.0 + np.floor(3.0 * rng.random(x.size))   # (counts: Poisson takes them too)
        lik = LIKS[fn["lik"]]
        if fn["data"].startswith("planes-"):
            kind = SIGMA_KINDS[fn["data"][7:]]
            sigma = {0: None, 1: np.full(x.size, 0.5), 2: np.full(C, 0.5), 3: np.full((C, x.size), 0.5)}[kind]
            e.set_dataset_planes(k, x, np.tile(y, (C, 1)), sigma, kind, lik)
        elif fn["data"] == "cols2":
            e.set_dataset(k, np.column_stack([x, 0.5 * x]), y, 0.5, lik)
        elif fn["data"] == "shared":
            e.set_dataset(k, x, y, 0.5, lik)
        if fn["lik"] == "expr":
            e.set_likelihood_expr(k, "0.0 - (0.5*(((y - model)/error)*((y - model)/error)))")
    return e, np.array(theta)
