"""CPU checks of the host-pure rules of the highest-density-interval read-out: carve_hdi and
one_item_fits (csrc/mhx_stage.hpp) and the path rule hdi_use_lds / hdi_lds_bytes / hdi_pad
(csrc/mhx_plan.hpp), driven as tests/test_histo_stage_plan.py drives its header: a small program
compiled against the headers (tests/hdi_cases.py has it) answers for a grid of shapes.  A portion's
carved bytes stay within the budget, its pieces lie in the engine's order without reaching into
each other, by the planner's accounting one more chain would not fit, and the one shape whose keys
exceed a portion for a single chain is refused."""
import itertools
import shutil

import pytest

import hdi_cases as hd

B = 1 << 26
LDS = 20 << 10


@pytest.fixture(scope="module")
def ask():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return hd.driver_answers


def test_portions_stay_within_the_budget_and_one_more_chain_would_not_fit(ask):
    shapes = []
    for nc, nm, nl, take, wv in itertools.product((1, 2, 8, 33, 63), (0, 1, 8), (0, 2, 101, 4096),
                                                  (1, 1000, 8192, 1 << 17), (0, 1)):
        for key_pitch in (0, hd.pad(take)):         # the LDS path carves no keys
            shapes.append((nc, nm, nl, take, wv, key_pitch))
    answers = ask(["%d %d %d %d %d %d" % s for s in shapes])
    refused = []
    for shape, line in zip(shapes, answers):
        need = hd.carve_need(*shape)
        head, *carvings = line.split("|")
        P, fits = (int(w) for w in head.split())
        per, slack = sum(need), 256 * len(need)
        assert fits == (per + slack <= B), (shape, line)
        if not fits:
            refused.append(shape)
            continue
        assert P == (B - slack) // per >= 1, (shape, line)
        assert (P + 1) * per + slack > B, (shape, line)                 # one more chain would not fit
        for n, carving in zip((1, P), carvings):
            total, *off = (int(w) for w in carving.split())
            assert len(off) == len(need) == 8, (shape, line)
            assert all(o % 256 == 0 for o in off) and off[0] == 0, (shape, n, off)
            for k in range(len(off)):
                assert off[k] + n * need[k] <= (off[k + 1] if k + 1 < len(off) else total), (shape, n, k, off)
            assert total <= B, (shape, n, total)
    # what must be refused: 63 columns of a window of 2^17 steps are 66 060 288 bytes of keys, which
    # the ladders of 4096 ranks (2 064 384 bytes) take past the 64 MiB; so do keys and staged values
    # together.  Nothing else of the grid is refused, and nothing at all on the LDS path.
    assert refused and all(s[0] >= 33 and s[3] == 1 << 17 and (s[5] or s[4]) for s in refused), refused
    assert (63, 0, 4096, 1 << 17, 0, 1 << 17) in refused and (63, 0, 101, 1 << 17, 0, 1 << 17) not in refused
    assert (63, 8, 101, 1 << 17, 1, 1 << 17) in refused and (33, 8, 4096, 1 << 17, 0, 1 << 17) not in refused
    assert not any(s[4] == 0 and s[5] == 0 for s in refused)


def test_the_path_rule(ask):
    cases = [(take, nc, off) for take in (1, 2, 3, 57, 1000, 1024, 1025, 2048, 4096, 8192, 1 << 17)
             for nc in (1, 2, 3, 8, 9, 10, 19, 20, 33, 63) for off in (0, 1)]
    lds_seen = set()
    for (take, nc, off), line in zip(cases, ask(["p %d %d %d" % c for c in cases])):
        use, nbytes, p = (int(w) for w in line.split())
        assert p == hd.pad(take) and p >= max(take, 2) and p & (p - 1) == 0 and (p == 2 or p < 2 * take)
        assert nbytes == 8 * nc * (p + 1), (take, nc)
        assert use == (0 if off else int(nbytes <= LDS)), (take, nc, off)
        lds_seen.add((take, nc, use))
    # two columns of 1000 steps sort in one workgroup's LDS, three do not; a window of 8192 steps at
    # three columns could not whatever the layout and the budget (3 x 8192 x 8 = 196 608 bytes are
    # more than a CU has); 33 columns fit at 57 steps
    assert (1000, 2, 1) in lds_seen and (1000, 3, 0) in lds_seen and (1000, 8, 0) in lds_seen
    assert (8192, 3, 0) in lds_seen and 3 * 8192 * 8 > 160 << 10
    assert (57, 33, 1) in lds_seen and (57, 63, 0) in lds_seen and (2048, 1, 1) in lds_seen and (2048, 2, 0) in lds_seen
