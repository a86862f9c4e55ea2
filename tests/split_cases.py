"""The split launch forms, read per value: form selection, a probe that reads a split form's
log-posterior at a vector a test chose, the case tables, and the pair / slot / slice arithmetic of
the kernels restated for the host.  Shared by tests/test_split_cases_host.py (no GPU: every case
reaches the place its comment names, and the faithful oracle stays within the tolerance of the
high-precision reference) and tests/test_gpu_split_values.py (the device).

THE PROBE.  mhx_logpost always takes the batch path.  A split form's value at theta is read by
walking: init_chains(theta), then take_step(L = 0, temperature = 1e300).  The proposal is
theta + 0 z = theta; the accept test (p1 > p0) || ((p1 - p0) / 1e300 > log u) holds for every
finite p1 and every u < 1; state()["logpost"] is then what the split form computed at theta.  A
chain that did not take the step (age still 1) fails the probe: it would report k_init's batch
value.  A vector whose log-posterior is not finite is trapped by k_init already
(MHX_CHAIN_FP_TRAP) and never walks.

THE ARITHMETIC (csrc/mhx_kernels.hpp, csrc/mhx_engine.cpp, csrc/mhx_plan.hpp):
  per chain     choose_split under MHX_SPLIT=k: min(max(longest / (512 W), 1), k) slices of W wave
                slots; k_split_sweep_body: pairs = ceil(n / 128), per = ceil(pairs / slots), slot s
                takes pairs [s per, min((s + 1) per, pairs))
  tile-sliced   choose_tsplit under MHX_TSPLIT=k: min(k, windows of the longest dataset) slices;
                build_ts_table: function by function per = ceil(windows / slices) windows a slice,
                slice s starts at point s per 2048 and holds min(per 2048, n - off) points (none
                past the data); the window of a slice stays in LDS (FnDesc::solo) in the
                persistent form of a problem of ONE function whose every slice is ONE window
"""
import collections
import functools
import os

import numpy as np

import offset_cases as oc
import problems as pb

KWAVE = 64             # kWave
PAIR = 2 * KWAVE       # the points a lane pair of sweep_direct takes per iteration
WINDOW = 2048          # kPadPoints
REL = 1e-12            # the project's stated tolerance: REL * sum |term|, no additive constant
PRIOR_ULP = 2.0 ** -52 * 1e10   # per violated bound (tests/test_gpu_tile_plan.py states the rule)
ROUNDS = 40            # plain steps after the probe step

KNOBS = ("MHX_SPLIT", "MHX_TSPLIT", "MHX_NO_PERSIST", "MHX_PERSIST_TS", "MHX_NO_RESIDENT_SLICES",
         "MHX_NO_YW", "MHX_FAMILY_WPG", "MHX_NO_GRAPH")


def ceil_div(a, b):
    return -(-a // b)


# ---- the kernels' arithmetic, restated --------------------------------------------------------
def tile_points(wpg):
    return 2 * KWAVE * wpg


def forced_split_slices(longest, k, wpg=8):
    """choose_split with MHX_SPLIT=k"""
    return 0 if k <= 0 else min(max(longest // (512 * wpg), 1), k)


def chain_slots(n, slices, wpg=8):
    """[(b0, b1)] per wave slot: the pairs of 128 points slot s of k_split_sweep takes"""
    slots = slices * wpg
    pairs = ceil_div(n, PAIR)
    per = ceil_div(pairs, slots)
    return [(min(s * per, pairs), min(s * per + per, pairs)) for s in range(slots)]


def forced_ts_slices(longest, k):
    """choose_tsplit with MHX_TSPLIT=k: never more slices than windows, at least two"""
    want = min(k, ceil_div(longest, WINDOW))
    return want if want >= 2 else 0


def ts_table(n, slices):
    """build_ts_table for one function: (windows per slice, [(first point, points)] per slice,
    (0, 0) for a slice past the data)"""
    per = ceil_div(ceil_div(n, WINDOW), slices)
    out = []
    for s in range(slices):
        off = s * per * WINDOW
        out.append((0, 0) if off >= n else (off, min(per * WINDOW, n - off)))
    return per, out


def ts_resident(lens, slices, wpg=8):
    """whether the persistent form keeps each slice's window in LDS"""
    return (len(lens) == 1 and WINDOW <= 2 * tile_points(wpg)
            and all(ts_table(n, slices)[0] == 1 for n in lens))


def window_steps(x):
    """window_grids (csrc/mhx_finalize.hpp): the grid step of every 2048-point window, tried with
    the previous grid window's first, 0 where the window is no grid"""
    x = np.asarray(x, float)

    def fits(w, h):
        if len(w) < 2 or h == 0.0:
            return False
        tol = 8.0 * 2.0 ** -52 * max(abs(w[0]), abs(w[-1]))
        return bool((np.abs(w - (w[0] + np.arange(len(w)) * h)) <= tol).all())

    out, h_prev = [], 0.0
    for i0 in range(0, len(x), WINDOW):
        w = x[i0:i0 + WINDOW]
        h = h_prev if fits(w, h_prev) else ((w[-1] - w[0]) / (len(w) - 1) if len(w) > 1 else 0.0)
        if not fits(w, h):
            h = 0.0
        out.append(h)
        h_prev = h or h_prev
    return out


# ---- problems, all with bounds off: the number is the likelihood alone -------------------------
def _two_peak_on(x, seed, model=pb.GAUSS, lik=pb.NORMAL):
    rng = np.random.default_rng(seed)
    th = np.array([0.5, 0.3, 1.0, 0.3, 0.05, 0.7, 0.7, 0.08])  # b0 b1 A1 mu1 w1 A2 mu2 w2
    sig = rng.uniform(0.05, 0.15, len(x))
    y = pb.model_eval_np(model, (2, 2), th, x) + sig * rng.standard_normal(len(x))
    s = pb.Spec(8)
    s.add(model, (2, 2), range(8), x, y, sig, lik, None)
    s.theta_star = th
    return s


def pvoigt_global(lens, seed=3):
    """problems.global_fit with a length per dataset (x not a grid) and no bounds"""
    rng = np.random.default_rng(seed)
    n_sets = len(lens)
    d = 8 + 3 * n_sets
    th = np.zeros(d)
    th[:8] = [0.35, 0.06, 0.4, 0.65, 0.09, 0.6, 0.8, 0.1]   # mu1 w1 eta1 mu2 w2 eta2 rho c2
    s = pb.Spec(d)
    for k, n in enumerate(lens):
        th[8 + 3 * k: 11 + 3 * k] = (rng.uniform(0.5, 2.0), rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3))
        idx = [8 + 3 * k, 9 + 3 * k, 10 + 3 * k, 0, 1, 2, 3, 4, 5, 6, 7]
        x = np.sort(rng.uniform(0, 1, n))
        sig = rng.uniform(0.03, 0.08, n)
        y = pb.pvoigt_eval(th[idx], x) + sig * rng.standard_normal(n)
        s.add(pb.PVOIGT2, (), idx, x, y, sig, pb.NORMAL, None)
    s.theta_star = th
    return s


@functools.lru_cache(maxsize=None)
def problem(kind, lens):
    """the Spec of (kind, dataset lengths): built once per process; nobody changes it"""
    n = lens[0]
    seed = 40 + sum(lens) % 97
    if kind == "grid":          # the recurrence path
        s = pb.two_peak(n=n, seed=seed, bounds=False)
    elif kind == "cutoff":
        s = pb.two_peak(n=n, seed=seed, lik=pb.CUTOFF, bounds=False)
    elif kind == "bounded":     # the prior cases
        s = pb.two_peak(n=n, seed=seed, bounds=True)
    elif kind == "jitter":      # no grid in any window: the direct path
        h = 1.0 / max(n - 1, 1)
        x = np.linspace(0.0, 1.0, n) + 0.3 * h * np.random.default_rng(seed).uniform(-1, 1, n)
        s = _two_peak_on(x, seed)
    elif kind == "lorentz":
        s = _two_peak_on(np.linspace(0.0, 1.0, n), seed, model=pb.LORENTZ)
    elif kind == "poisson":
        s = pb.poisson_peaks(n=n, seed=seed)
        s.bounds[0] = None
    elif kind == "pvoigt":
        s = pvoigt_global(lens, seed)
    elif kind == "piecewise":
        s = pb.two_peak_piecewise(n=n, seed=seed)
        s.bounds[0] = None
    else:
        raise KeyError(kind)
    assert tuple(len(d[0]) for d in s.data) == tuple(lens)
    return s


# (parameter, value) of the odd vectors: a width of 1e-4, a negative width, a centre far outside
# the data (the three of test_gpu_tile_plan.proposal_vectors), a negative amplitude, and one more
# of the kind's own - Poisson: a background that makes the rate negative between the peaks (the
# reference is NaN: the chain must be trapped); cutoff: a background 12 above the data, where
# r^2 / 2 runs from 3200 to 28800 and the clamp at -5000 cuts some terms and not others
_PEAKS22 = [(4, 1e-4), (7, -0.03), (3, 7.5), (2, -0.8)]
ODD = {
    "grid": _PEAKS22, "jitter": _PEAKS22, "lorentz": _PEAKS22, "piecewise": _PEAKS22, "bounded": [],
    "cutoff": _PEAKS22 + [(0, 12.5)],
    "poisson": [(3, 1e-4), (6, -0.03), (5, 7.5), (1, -10.0), (0, -5.0)],
    "pvoigt": [(1, 1e-4), (4, -0.09), (0, 7.5), (8, -0.7)],
}
ODD_ROWS = (1, 3, 4, 5, 6)   # where they sit among the 17: any 7 leading rows hold them all
N_VECTORS = 17


@functools.lru_cache(maxsize=None)
def all_vectors(kind, lens):
    """17 vectors of problem(kind, lens): theta*, perturbations by 2 % and the odd ones"""
    s = problem(kind, lens)
    th = pb.perturbed(s.theta_star, N_VECTORS, 0.02, seed=4)
    th[0] = s.theta_star
    for row, (j, v) in zip(ODD_ROWS, ODD[kind]):
        th[row] = s.theta_star
        th[row, j] = v
    th.setflags(write=False)
    return th


def rates_positive(s, theta):
    """False where a Poisson function's rate is <= 0 at some point: the reference is not finite"""
    for (model, shape, idx), (x, y, sig, lik) in zip(s.fns, s.data):
        if lik == pb.POISSON and not (pb.model_eval_np(model, shape, np.asarray(theta)[idx], x) > 0).all():
            return False
    return True


_HP = {}


def hp_reference(s, theta):
    """(log-posterior as a float, sum |term|) by offset_cases.hp_logpost - mpmath at 120 bits -,
    (nan, nan) where a Poisson rate is not positive; once per (problem, vector)"""
    key = (id(s), np.asarray(theta, float).tobytes())
    if key not in _HP:
        if rates_positive(s, theta):
            v, scale = oc.hp_logpost(s, theta)
            _HP[key] = (s, float(v), scale)
        else:
            _HP[key] = (s, float("nan"), float("nan"))
    return _HP[key][1:]


def oracle_reference(op, theta):
    """the same pair from the faithful oracle (the long and the piecewise cases: per-point mpmath
    is too slow there; tests/test_gpu_tile_plan.py does the same at 131073 points)"""
    return op.logpost(theta), op.abs_terms(theta)


def sum_half_r2(s, theta):
    """sum r_i^2 / 2 of a normal-likelihood problem, r = (y - f) / sigma: the scale of the
    reordering bound (a bound's scale needs no extra precision)"""
    total = 0.0
    for (model, shape, idx), (x, y, sig, lik) in zip(s.fns, s.data):
        assert lik == pb.NORMAL
        r = (y - pb.model_eval_np(model, shape, np.asarray(theta)[idx], x)) / sig
        total += 0.5 * float(np.sum(r * r))
    return total


def reorder_depths(n, slices):
    """(D_batch, D_split): the longest chain of additions that ends in the log-posterior, batch
    sweep against tile-sliced form, for ONE function of n points (see
    test_gpu_split_values.test_tile_sliced_values for the derivation)"""
    nwin = ceil_div(n, WINDOW)
    per = ceil_div(nwin, slices)
    lane = WINDOW // KWAVE // 2          # 16 points of a lane per accumulator and window
    butterfly = 6                        # wave_sum: xor 32, 16, 8, 4, 2, 1
    d_batch = lane * nwin + 1 + butterfly + 1
    d_split = lane * per + 1 + butterfly + ceil_div(slices, KWAVE) + butterfly + 1
    return d_batch, d_split


# ---- the launch forms --------------------------------------------------------------------------
Form = collections.namedtuple("Form", "label env name persistent")


def per_chain_forms(k):
    return [Form("two launches", {"MHX_SPLIT": str(k), "MHX_NO_PERSIST": "1"}, " split x", False),
            Form("persistent", {"MHX_SPLIT": str(k)}, "persistent split x", True)]


def tile_sliced_forms(k, wpg, extras=True):
    base = {"MHX_TSPLIT": str(k), "MHX_FAMILY_WPG": str(wpg)}
    two = Form("two launches", dict(base, MHX_PERSIST_TS="0"), " tsplit x", False)
    per = Form("persistent", dict(base, MHX_PERSIST_TS="1"), "persistent tsplit x", True)
    out = [two, per]
    if extras:
        out += [Form("persistent, no resident windows", dict(per.env, MHX_NO_RESIDENT_SLICES="1"), per.name, True),
                Form("two launches, no yw tiles", dict(two.env, MHX_NO_YW="1"), two.name, False),
                Form("persistent, no yw tiles", dict(per.env, MHX_NO_YW="1"), per.name, True)]
    return out


def engine_in_form(mhx, spec, chains, form, slices, wpg=8, extra_env=None, **kw):
    """an engine of `chains` chains finalised under the form's knobs, every variable this touches
    restored; the launch form is asserted through kernel_name()"""
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(form.env)
    os.environ.update(extra_env or {})
    try:
        e = spec.engine(mhx, chains, **kw)
        name = e.kernel_name()   # finalises under these settings
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    ok = (name.startswith("w%d/" % wpg) and name.endswith("%s%d" % (form.name, slices))
          and ("persistent" in name) == form.persistent)
    if not ok:
        e.close()
        raise AssertionError("wanted w%d/...%s%d, got %r" % (wpg, form.name, slices, name))
    return e


def probe(mhx, e, theta, finite):
    """the form's log-posterior at every row of theta (one chain each); finite: where the
    reference is finite.  Asserts that every such chain took the step at the very vector."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    d = theta.shape[1]
    e.init_chains(theta)
    e.take_step(np.zeros((d, d)), 1e300)
    st, status = e.state(), e.chain_status()[0]
    assert np.array_equal(st["theta"].view(np.uint64), theta.view(np.uint64)), "theta moved"
    want = np.where(finite, 2, 1)
    assert np.array_equal(st["age"], want) and np.array_equal(st["length"], want), (st["age"], st["length"], finite)
    assert np.array_equal(status == mhx.capi.CHAIN_FP_TRAP, ~np.asarray(finite)), (status, finite)
    assert (status[np.asarray(finite)] == mhx.capi.CHAIN_DONE).all(), status
    return st["logpost"].copy()


def newest_probs(mhx, e, take):
    """[chains, take]: the `take` newest entries of every chain's prob history, newest first"""
    out = e.traces(take, cols=[mhx.capi.TRACE_PROB])
    assert (out["n_out"] == take).all(), out["n_out"]
    return out["values"][:, :take, 0]


def rounds(mhx, e, finite, L=None):
    """ROUNDS plain steps after the probe step; with L = 0 every chain proposes its own vector
    again and the history's 1 + ROUNDS newest entries are what the form computed there round
    after round.  (A round whose value came out LOWER would be accepted only with probability
    exp(difference): what this holds is that no round's value enters the history with other bits.)
    Returns the histories [chains, 1 + ROUNDS] of the chains that walk."""
    d = e.d
    e.many_steps(ROUNDS, np.zeros((d, d)) if L is None else L)
    st = e.state()
    fin = np.asarray(finite)
    assert (st["age"][fin] == ROUNDS + 2).all() and (st["age"][~fin] == 1).all(), st["age"]
    if not fin.all():   # (a trapped chain has one entry: the others are read one by one)
        hist = np.full((len(fin), ROUNDS + 1), np.nan)
        for c in np.flatnonzero(fin):
            hist[c] = e.trace(int(c), ROUNDS + 1)[0]
        return hist
    return newest_probs(mhx, e, ROUNDS + 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """bit equality that takes NaN == NaN of the same payload (trapped chains)"""
    return np.array_equal(bits(a), bits(b))


# ---- case tables -------------------------------------------------------------------------------
# Per-chain form, 8-wave family (MHX_SPLIT=k; one slice of 8 wave slots for short data).
#   used: slots that hold pairs, per function;  last: pairs in the last slot used (< per: the
#   ragged last chunk);  tail: data points in the last pair (< 128: reads into the padded tail)
PerChain = collections.namedtuple("PerChain", "id kind lens k chains rows slices per used last tail")
PER_CHAIN_CASES = [
    # one pair, then two: all but the first slots are empty
    PerChain("grid-1", "grid", (1,), 1, 1, (4,), 1, (1,), (1,), (1,), (1,)),
    PerChain("grid-127", "grid", (127,), 1, 3, (0, 1, 3), 1, (1,), (1,), (1,), (127,)),
    PerChain("grid-128", "grid", (128,), 1, 7, None, 1, (1,), (1,), (1,), (128,)),
    PerChain("grid-129", "grid", (129,), 1, 3, (0, 4, 5), 1, (1,), (2,), (1,), (1,)),
    PerChain("jitter-129", "jitter", (129,), 1, 1, (1,), 1, (1,), (2,), (1,), (1,)),
    PerChain("poisson-127", "poisson", (127,), 1, 7, None, 1, (1,), (1,), (1,), (127,)),
    PerChain("cutoff-129", "cutoff", (129,), 1, 3, (0, 5, 6), 1, (1,), (2,), (1,), (1,)),
    # eight pairs, one per slot
    PerChain("grid-1024", "grid", (1024,), 1, 7, None, 1, (1,), (8,), (1,), (128,)),
    PerChain("lorentz-1024", "lorentz", (1024,), 1, 1, (3,), 1, (1,), (8,), (1,), (128,)),
    # nine pairs, per = 2: slots 5 to 7 empty, slot 4 half full
    PerChain("grid-1025", "grid", (1025,), 1, 7, None, 1, (2,), (5,), (1,), (1,)),
    PerChain("grid-1025-one", "grid", (1025,), 1, 1, (5,), 1, (2,), (5,), (1,), (1,)),
    PerChain("jitter-1025", "jitter", (1025,), 1, 3, (0, 1, 4), 1, (2,), (5,), (1,), (1,)),
    PerChain("cutoff-1025", "cutoff", (1025,), 1, 7, None, 1, (2,), (5,), (1,), (1,)),
    PerChain("poisson-1025", "poisson", (1025,), 1, 7, None, 1, (2,), (5,), (1,), (1,)),
    PerChain("lorentz-1025", "lorentz", (1025,), 1, 3, (0, 1, 5), 1, (2,), (5,), (1,), (1,)),
    # 24 slots, 97 pairs, per = 5: the last slots beyond the data
    PerChain("grid-12289-x3", "grid", (12289,), 3, 7, None, 3, (5,), (20,), (2,), (1,)),
    PerChain("grid-12289-x3-three", "grid", (12289,), 3, 3, (2, 3, 6), 3, (5,), (20,), (2,), (1,)),
    # the cap by the data: min(max(12289 / 4096, 1), 99) = 3
    PerChain("grid-12289-x99", "grid", (12289,), 99, 1, (1,), 3, (5,), (20,), (2,), (1,)),
    # a global fit whose short function occupies slot 0 only (split_logpost's k > 0 sums)
    PerChain("pvoigt-1+12289", "pvoigt", (1, 12289), 3, 3, (0, 1, 5), 3, (1, 5), (1, 20), (1, 2), (1, 1)),
]

# Tile-sliced form (MHX_TSPLIT=k), 9 chains in the 8-wave family and 17 in the 16-wave family: a
# full group and one more chain.
#   n: points per slice, per function (0: an empty slice);  resident: the persistent form keeps
#   every slice's window in LDS;  ref: "hp" (mpmath) or "oracle";  sharp: the reordering bound
#   against the batch kernel is held as well (two_peak normal, one function)
TileSliced = collections.namedtuple("TileSliced", "id kind lens k slices n resident ref sharp vectors")
TILE_SLICED_CASES = [
    # the second slice holds one point
    TileSliced("grid-2049-ts2", "grid", (2049,), 2, 2, ((2048, 1),), True, "hp", True, 17),
    TileSliced("poisson-2049-ts2", "poisson", (2049,), 2, 2, ((2048, 1),), True, "hp", False, 17),
    # two whole resident windows
    TileSliced("grid-4096-ts2", "grid", (4096,), 2, 2, ((2048, 2048),), True, "hp", True, 17),
    TileSliced("jitter-4096-ts2", "jitter", (4096,), 2, 2, ((2048, 2048),), True, "hp", False, 17),
    # slices of two windows and one: not resident; then three slices, the last holding one point
    TileSliced("grid-4097-ts2", "grid", (4097,), 2, 2, ((4096, 1),), False, "hp", True, 17),
    TileSliced("grid-4097-ts3", "grid", (4097,), 3, 3, ((2048, 2048, 1),), True, "hp", True, 17),
    TileSliced("cutoff-4097-ts2", "cutoff", (4097,), 2, 2, ((4096, 1),), False, "hp", False, 17),
    # more slices asked for than there are windows
    TileSliced("grid-6144-ts7", "grid", (6144,), 7, 3, ((2048, 2048, 2048),), True, "hp", True, 9),
    TileSliced("lorentz-6144-ts7", "lorentz", (6144,), 7, 3, ((2048, 2048, 2048),), True, "hp", False, 9),
    # a global fit whose first function leaves slices 2 and 3 empty
    TileSliced("pvoigt-2049+9000-ts4", "pvoigt", (2049, 9000), 4, 4,
               ((2048, 1, 0, 0), (4096, 4096, 808, 0)), False, "hp", False, 9),
    # per-window grids: slices that start on windows whose grid differs from window 0's (shifted
    # tgh).  12288 points: windows 2, 3, 4 hold a junction and are no grid; 20480 points: also
    # windows on the steps 0.6 h and 1.7 h, and the jittered window 1.  (Kernels that follow a
    # per-window grid table are compiled at run time, once per family: the first of these cases
    # pays for that, about ten seconds where the on-disk cache is cold)
    TileSliced("piecewise-12288-ts3", "piecewise", (12288,), 3, 3, ((4096,) * 3,), False, "oracle", False, 17),
    TileSliced("piecewise-12288-ts6", "piecewise", (12288,), 6, 6, ((2048,) * 6,), True, "oracle", False, 17),
    TileSliced("piecewise-20480-ts5", "piecewise", (20480,), 5, 5, ((4096,) * 5,), False, "oracle", False, 17),
    TileSliced("piecewise-20480-ts10", "piecewise", (20480,), 10, 10, ((2048,) * 10,), True, "oracle", False, 17),
    # 66 windows a slice: slice 1 starts at window 66 and crosses its own 64th window (the reload
    # of window masks and seed x)
    TileSliced("grid-270336-ts2", "grid", (2048 * 132,), 2, 2, ((2048 * 66,) * 2,), False, "oracle", False, 9),
]

# the prior cases: vectors that violate 0, 1 and 3 bounds of two_peak (0.5 theta*, 1.5 theta*)
# by at most 0.1 - b0 0.8 > 0.75, A1 1.55 > 1.5, mu2 1.1 > 1.05
PRIOR_ROWS = [[], [(0, 0.8)], [(0, 0.8), (2, 1.55), (6, 1.1)]]


def case_vectors(case):
    th = all_vectors(case.kind, case.lens)
    if isinstance(case, PerChain):
        return th[list(case.rows)] if case.rows is not None else th[:case.chains]
    return th[:case.vectors]


def prior_vectors(s):
    th = np.tile(s.theta_star, (len(PRIOR_ROWS), 1))
    for row, moves in zip(th, PRIOR_ROWS):
        for j, v in moves:
            row[j] = v
    return th


def violated(s, theta):
    n = 0
    for b in s.bounds:
        if b is not None:
            v = np.asarray(theta)[b[0]]
            n += int((~((np.asarray(b[1]) < v) & (v < np.asarray(b[2])))).sum())
    return n


def references(case, orc=None):
    """(reference log-posteriors, sum |term|) of the case's vectors, NaN where not finite"""
    s = problem(case.kind, case.lens)
    if getattr(case, "ref", "hp") == "oracle":
        op = s.oracle(orc)
        pairs = [oracle_reference(op, t) for t in case_vectors(case)]
    else:
        pairs = [hp_reference(s, t) for t in case_vectors(case)]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


class Worst:
    """the worst observed ratio to each bound, per form: printed, never a threshold"""

    def __init__(self):
        self.r = {}

    def add(self, what, ratio):
        self.r[what] = max(self.r.get(what, 0.0), float(ratio))

    def show(self, title):
        same = collections.OrderedDict()   # (forms that gave the same bits share a figure)
        for what, ratio in sorted(self.r.items()):
            same.setdefault("%.3g" % ratio, []).append(what)
        print("%s: " % title + "; ".join("%s [%s]" % (v, ", ".join(k)) for v, k in same.items()))
