"""The host yardstick of the batched traces (mhx_get_traces): for every chain its own trace,
e.trace(c, take), and numpy / plain Python - the three predicates on uint64 views of prob, the
thinning of `thin` (mcmc-fitting.lisp:149-157), and the envelope as the sequential loop the header
writes down.  Nothing here calls Engine.traces.  Every comparison is bit for bit: doubles are
compared as uint64."""
import numpy as np

PROB = -1
FILTERS = ("steps", "unique", "forward")


def kept_indices(prob, filt):
    """the steps of a newest-first window that the filter keeps, newest first"""
    t = len(prob)
    if filt == "steps":
        return list(range(t))
    if filt == "unique":    # M:492-496: `equal` on double-floats is the same bits; the oldest stays
        bits = np.asarray(prob, dtype=np.float64).view(np.uint64)
        return [s for s in range(t) if s == t - 1 or bits[s] != bits[s + 1]]
    assert filt == "forward"    # M:497-502
    return [s for s in range(t - 1) if not prob[s] <= prob[s + 1]]


def bucket_extremes(v, stride, start):
    """(first, lo, hi) of every bucket of `stride` items of the list v from item `start` on: lo and
    hi start as the bucket's first value and move only where a later value is strictly beyond"""
    first, lo, hi = [], [], []
    for k0 in range(start, len(v), stride):
        a = b = v[k0]
        for x in v[k0 + 1:k0 + stride]:
            if x < a:
                a = x
            if x > b:
                b = x
        first.append(v[k0])
        lo.append(a)
        hi.append(b)
    return first, lo, hi


class Yardstick:
    """what mhx_get_traces has to return for engine e, from e.trace alone.  The windows, the kept
    lists and the columns' bucket extremes are computed once and kept."""

    def __init__(self, e):
        self.e, self._windows, self._kept, self._buckets = e, {}, {}, {}

    def windows(self, take):
        if take not in self._windows:
            self._windows[take] = [self.e.trace(c, take) for c in range(self.e.n_chains)]
        return self._windows[take]

    def kept(self, take, filt):
        if (take, filt) not in self._kept:
            self._kept[take, filt] = [kept_indices(prob, filt) for prob, _ in self.windows(take)]
        return self._kept[take, filt]

    def buckets(self, take, filt, stride, start, col):
        """per chain (first, lo, hi) of column col (PROB: the prob) of the kept list"""
        key = (take, filt, stride, start, col)
        if key not in self._buckets:
            out = []
            for (prob, th), kept in zip(self.windows(take), self.kept(take, filt)):
                column = prob if col == PROB else th[:, col]
                out.append(bucket_extremes(column[kept].tolist() if kept else [], stride, start))
            self._buckets[key] = out
        return self._buckets[key]

    def want(self, take, cols, filt="steps", stride=1, start=0, max_out=None, envelope=False):
        n = self.e.n_chains
        kept = self.kept(take, filt)
        if max_out is None:
            max_out = max(len(range(start, take, stride)), 1)
        out = {"values": np.zeros((n, max_out, len(cols)))}
        if envelope:
            out["lo"], out["hi"] = np.zeros((n, max_out, len(cols))), np.zeros((n, max_out, len(cols)))
        out["n_out"] = np.array([min(len(range(start, len(k), stride)), max_out) for k in kept], dtype=np.int32)
        out["n_kept"] = np.array([len(k) for k in kept], dtype=np.int32)
        out["n_used"] = np.array([len(p) for p, _ in self.windows(take)], dtype=np.int32)
        for j, col in enumerate(cols):
            per_chain = self.buckets(take, filt, stride, start, col)
            for c in range(n):
                no = int(out["n_out"][c])
                for name, side in zip(("values", "lo", "hi") if envelope else ("values",), per_chain[c]):
                    out[name][c, :no, j] = np.array(side[:no], dtype=np.float64)
        return out


def differences(got, want):
    """the names of the arrays that differ in a bit (empty: the same)"""
    bad = [k for k in want if k not in got] + [k for k in got if k not in want]
    for k in want:
        if k in got:
            g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
            if g.dtype != w.dtype or g.shape != w.shape:
                bad.append(k)
            elif g.dtype == np.float64:
                if not np.array_equal(g.view(np.uint64), w.view(np.uint64)):
                    bad.append(k)
            elif not np.array_equal(g, w):
                bad.append(k)
    return bad


def rows_beyond_are_zero(r):
    """rows n_out .. of values, lo and hi are all-bits-zero"""
    beyond = np.arange(r["values"].shape[1])[None, :] >= r["n_out"][:, None]
    return all(not r[k].view(np.uint64)[beyond].any() for k in ("values", "lo", "hi") if k in r)
