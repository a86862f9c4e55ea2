"""The four split launch forms, per value.  `-m gpu`: needs an MI355X.

tests/test_gpu_split.py holds the split forms to settled walks; here every form's log-posterior is
read at vectors the test chose (tests/split_cases.py: the probe) on the smallest datasets that
reach each place of the split-only code - the pair and slot arithmetic of k_split_sweep and
k_persist with its empty slots and ragged last chunk, reads into the padded tail, the slice table
of k_split_tsweep and k_persist_ts with its shifted pointers and window tables, empty slices,
resident windows, the reload of window masks past a slice's 64th window, split_logpost - and
compared with a high-precision reference (mpmath, 120 bits) under the project's stated tolerance
1e-12 * sum |term| with no additive constant.  tests/test_split_cases_host.py shows on the CPU
that every case reaches its place and that the references agree among themselves.

What must be the same bits: the two launches and the persistent form; resident windows and
MHX_NO_RESIDENT_SLICES=1; MHX_NO_YW=1 and the default; the 8- and the 16-wave family at equal
slicing; every one of 41 rounds at the same vector; a probe in all-probe company and among chains
that walk wildly.  None of these had to be relaxed.  Every test prints the worst ratio it saw to
each bound, per form; on an MI355X: at most 0.005 of 1e-12 sum |term| against mpmath (0.01 on
the piecewise grids and 0.03 at 270336 points, against the faithful oracle), at most 0.055 of
the reordering bound.
"""
import numpy as np
import pytest

import split_cases as sc

pytestmark = pytest.mark.gpu
SEED = 8


@pytest.fixture(scope="module")
def mhx():
    import lisp_mcmc_amd
    return lisp_mcmc_amd


def hold(got, ref, scale, finite, extra=0.0):
    """|got - ref| <= 1e-12 sum |term| (+ extra) on every finite chain: the worst ratio"""
    worst = 0.0
    for c in np.flatnonzero(finite):
        tol = sc.REL * scale[c] + (extra[c] if np.ndim(extra) else extra)
        err = abs(got[c] - ref[c])
        assert err <= tol, (c, got[c], ref[c], err, tol)
        worst = max(worst, err / tol if tol > 0 else 0.0)
    return worst


def probe_and_rounds(mhx, e, th, finite):
    """the probe value of every chain and the same bits in each of the 40 rounds after it"""
    got = sc.probe(mhx, e, th, finite)
    hist = sc.rounds(mhx, e, finite)
    for c in np.flatnonzero(finite):
        assert (sc.bits(hist[c]) == sc.bits(got[c:c + 1])[0]).all(), (c, got[c], hist[c])
    return got


@pytest.mark.parametrize("case", sc.PER_CHAIN_CASES, ids=[c.id for c in sc.PER_CHAIN_CASES])
def test_per_chain_values(mhx, orc, case):
    """k_split_sweep + k_split_step and k_persist (FixedSpec::loglik_part -> sweep_direct /
    sweep_direct_rec) at 1, 3 and 7 chains: within 1e-12 sum |term| of the high-precision
    reference, the same bits in both forms and in every one of 41 rounds.  (The per-chain form
    seeds its recurrence from the slice's start, not from windows - sweep_direct_rec's comment -
    so it is held to the stated tolerance only, not to the batch kernel's bits.)"""
    s = sc.problem(case.kind, case.lens)
    th = sc.case_vectors(case)
    ref, scale = sc.references(case, orc)
    finite = np.isfinite(ref)
    got, worst = {}, sc.Worst()
    for form in sc.per_chain_forms(case.k):
        e = sc.engine_in_form(mhx, s, case.chains, form, case.slices, seed=SEED)
        try:
            got[form.label] = probe_and_rounds(mhx, e, th, finite)
        finally:
            e.close()
        worst.add(form.label, hold(got[form.label], ref, scale, finite))
    worst.show("%s, ratio to 1e-12 sum |term|" % case.id)
    assert sc.same_bits(got["two launches"][finite], got["persistent"][finite]), got


def family_chains(th, wpg):
    """9 chains in the 8-wave family, 17 in the 16-wave family: a full group and one more chain
    (the vectors of a case that has only 9 are gone through again)"""
    chains = wpg + 1
    return th[np.arange(chains) % len(th)]


@pytest.mark.parametrize("case", sc.TILE_SLICED_CASES, ids=[c.id for c in sc.TILE_SLICED_CASES])
def test_tile_sliced_values(mhx, orc, case):
    """k_split_tsweep + k_split_step and k_persist_ts on the slice table of build_ts_table, both
    kernel families: within 1e-12 sum |term| of the reference; the same bits in the two launches
    and the persistent form, with resident windows and without, with the yw tiles and without, in
    the 8- and the 16-wave family (slices are whole windows: the partial sums are the same), and
    in every one of 41 rounds - where a resident window that went stale, or a window table shifted
    by one, would show.

    THE REORDERING BOUND (two_peak, normal likelihood, one function: `sharp`).  Per point the
    tile-sliced form runs the batch sweep's arithmetic - sweep() on a FnDesc of whole windows:
    the same window masks, the same seeds, r = fma(-m, w, y) - so the two values differ only in
    how the exactly formed r_i^2 are added.  Every addition rounds once, and all terms are >= 0,
    so a sum reached through a chain of D additions lies within D 2^-53 S (first order) of
    S = sum r_i^2.
      batch (sweep(), finish_lik):  a lane adds its 32 points of a window alternately into acc0
        and acc1 (acc = fma(r, r, acc)): 16 W additions per accumulator over W windows; acc0 +
        acc1: 1; wave_sum's butterfly: 6; fma(-0.5, S, lik_const): 1.
        D_batch = 16 W + 8
      tile-sliced:  the same within a slice of P windows, 16 P + 1 + 6; the slice's sum is
        handed over exactly (-2 * fma(-0.5, S, 0)); split_logpost: a lane adds its slots in
        order, ceil(slices / 64) additions; the butterfly: 6; finish_by_lik's fma: 1.
        D_split = 16 P + 7 + ceil(slices / 64) + 7
    and |split - batch| <= (D_batch + D_split) 2^-53 sum r_i^2 / 2.  (The finishing fma rounds
    relative to the log-posterior itself, which is of the size of sum r_i^2 / 2 in these
    problems; it is counted as one addition of each chain.)  At n = 4096 in two slices this is
    71 * 2^-53 = 7.9e-15 of sum r_i^2 / 2, a hundred times finer than the stated tolerance."""
    s = sc.problem(case.kind, case.lens)
    th_all = sc.case_vectors(case)
    ref_all, scale_all = sc.references(case, orc)
    long_case = max(case.lens) > 100000   # (the two forms and nothing else: seconds)
    got, worst = {}, sc.Worst()
    for wpg in (8, 16):
        rows = np.arange(wpg + 1) % len(th_all)
        th, ref, scale = family_chains(th_all, wpg), ref_all[rows], scale_all[rows]
        finite = np.isfinite(ref)
        for form in sc.tile_sliced_forms(case.k, wpg, extras=not long_case):
            e = sc.engine_in_form(mhx, s, len(th), form, case.slices, wpg=wpg, seed=SEED)
            try:
                v = got[wpg, form.label] = probe_and_rounds(mhx, e, th, finite)
                batch = e.logpost(th) if case.sharp else None
            finally:
                e.close()
            worst.add("w%d %s" % (wpg, form.label), hold(v, ref, scale, finite))
            if case.sharp:
                db, ds = sc.reorder_depths(case.lens[0], case.slices)
                for c in np.flatnonzero(finite):
                    bound = (db + ds) * 2.0 ** -53 * sc.sum_half_r2(s, th[c])
                    assert abs(v[c] - batch[c]) <= bound, (wpg, form.label, c, v[c], batch[c], bound)
                    worst.add("w%d %s against the batch kernel, reordering bound" % (wpg, form.label),
                              abs(v[c] - batch[c]) / bound)
        base = got[wpg, "two launches"]
        for (w_, label), v in got.items():
            if w_ == wpg:
                assert sc.same_bits(base[finite], v[finite]), (wpg, label, base, v)
    f9 = np.isfinite(ref_all[np.arange(9) % len(th_all)])
    assert sc.same_bits(got[8, "two launches"][f9], got[16, "two launches"][:9][f9]), "8 against 16 waves"
    worst.show("%s, ratio to 1e-12 sum |term|" % case.id)


COMPANY = ([c for c in sc.PER_CHAIN_CASES if c.id in ("grid-1025", "poisson-1025", "grid-12289-x3")],
           [c for c in sc.TILE_SLICED_CASES if c.id in ("grid-4096-ts2", "grid-4097-ts2", "piecewise-12288-ts6",
                                                        "pvoigt-2049+9000-ts4")])


@pytest.mark.parametrize("case", COMPANY[0] + COMPANY[1], ids=[c.id for c in COMPANY[0] + COMPANY[1]])
def test_probes_keep_their_bits_in_wild_company(mhx, orc, case):
    """per-chain factors: the even chains are probes (L = 0), the odd chains walk from
    diag(0.4 |theta*|) - wild proposals, layout votes that change from round to round, chains
    that end trapped.  Over 40 plain steps the probes' prob history stays the bits it has in
    all-probe company, in all four forms (test_chain_slot_independence holds the batch kernels to
    this)."""
    s = sc.problem(case.kind, case.lens)
    per_chain = isinstance(case, sc.PerChain)
    ref, _ = sc.references(case, orc)
    if per_chain:
        th, forms, wpg = sc.case_vectors(case), sc.per_chain_forms(case.k), 8
    else:
        rows = np.arange(9) % len(sc.case_vectors(case))
        th, ref, forms, wpg = sc.case_vectors(case)[rows], ref[rows], sc.tile_sliced_forms(case.k, 8, extras=False), 8
    finite = np.isfinite(ref)
    C, d = th.shape
    wild = np.zeros((C, d, d))
    wild[1::2] = np.diag(0.4 * np.abs(s.theta_star))
    probes = [c for c in range(0, C, 2) if finite[c]]
    assert len(probes) >= 2 and C >= 3
    for form in forms:
        hist = {}
        for label, L in (("alone", None), ("company", wild)):
            e = sc.engine_in_form(mhx, s, C, form, case.slices, wpg=wpg, seed=SEED)
            try:
                sc.probe(mhx, e, th, finite)
                e.many_steps(sc.ROUNDS, np.zeros((d, d)) if L is None else L)
                st = e.state()
                assert (st["age"][probes] == sc.ROUNDS + 2).all(), (form.label, label, st["age"])
                if label == "company":   # the odd chains had their wild proposals judged, round after
                    status = e.chain_status()[0]   # round, until the end or a trap
                    for c in range(1, C, 2):
                        if finite[c]:
                            assert st["age"][c] == sc.ROUNDS + 2 or (
                                st["age"][c] >= 2 and status[c] == mhx.capi.CHAIN_FP_TRAP), (form.label, c, st["age"])
                hist[label] = np.array([e.trace(c, sc.ROUNDS + 1)[0] for c in probes])
            finally:
                e.close()
        assert hist["alone"].shape == (len(probes), sc.ROUNDS + 1)
        assert sc.same_bits(hist["alone"], hist["company"]), (case.id, form.label)


def test_prior_in_both_branches(mhx, orc):
    """split_logpost forms the prior after the sums in the two launches and in a branch of its
    own, before the sums arrive, in the persistent forms: two_peak with its bounds on, vectors
    that violate 0, 1 and 3 bounds by at most 0.1.  Reference: the high-precision likelihood of
    the same data plus the oracle's prior; tolerance: the likelihood's plus 4 * 2^-52 * 1e10 per
    violated bound (tests/test_gpu_tile_plan.py states the rule)."""
    lens = (4097,)
    s, twin = sc.problem("bounded", lens), sc.problem("grid", lens)
    op = s.oracle(orc)
    th3 = sc.prior_vectors(s)
    ref3, scale3, extra3 = [], [], []
    for t in th3:
        ll, scale = sc.hp_reference(twin, t)
        ref3.append(ll + op.logpost(t, parts=True)[1][1])
        scale3.append(scale)
        extra3.append(4 * sc.PRIOR_ULP * sc.violated(s, t))
    assert [x > 0 for x in extra3] == [False, True, True]
    worst = sc.Worst()
    for mode, forms, chains, slices in (("per chain", sc.per_chain_forms(1), 3, 1),
                                        ("tile-sliced", sc.tile_sliced_forms(2, 8, extras=False), 9, 2)):
        rows = np.arange(chains) % 3
        th = th3[rows]
        ref, scale, extra = np.array(ref3)[rows], np.array(scale3)[rows], np.array(extra3)[rows]
        finite = np.ones(chains, bool)
        got = {}
        for form in forms:
            e = sc.engine_in_form(mhx, s, chains, form, slices, seed=SEED)
            try:
                got[form.label] = probe_and_rounds(mhx, e, th, finite)
            finally:
                e.close()
            worst.add("%s, %s" % (mode, form.label), hold(got[form.label], ref, scale, finite, extra))
        assert sc.same_bits(got["two launches"], got["persistent"]), (mode, got)
    worst.show("prior cases, ratio to 1e-12 sum |term| + 4 * 2^-52 * 1e10 per violated bound")


def test_two_launches_issued_one_by_one(mhx, orc):
    """MHX_NO_GRAPH=1: the kernels of the two-launch form issued one by one give the bits of the
    captured and replayed portion, probe step and 40 rounds"""
    case = [c for c in sc.PER_CHAIN_CASES if c.id == "grid-12289-x3"][0]
    s = sc.problem(case.kind, case.lens)
    th = sc.case_vectors(case)
    finite = np.isfinite(sc.references(case, orc)[0])
    form = sc.per_chain_forms(case.k)[0]
    got = []
    for env in (None, {"MHX_NO_GRAPH": "1"}):
        e = sc.engine_in_form(mhx, s, case.chains, form, case.slices, extra_env=env, seed=SEED)
        try:
            got.append(probe_and_rounds(mhx, e, th, finite))
        finally:
            e.close()
    assert sc.same_bits(got[0], got[1]), got
