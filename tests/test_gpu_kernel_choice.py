"""The engine's kernel choice on the GPU: every accepted problem of
tests/golden/kernel_choice_cases.csv is built at the smallest shape that takes its branch, and
mhx_kernel_name() must say, to the letter, what the row recorded; one log-posterior of a finite
parameter vector is finite.  No walk.  (tests/test_finalize_host.py runs the same rows through the
choice rules on the CPU; identical programs share the compile cache.)"""
import numpy as np
import pytest

import kernel_choice_cases as kc

pytestmark = pytest.mark.gpu
ACCEPTED = [r for r in kc.rows() if int(r["code"]) == 0]


@pytest.mark.parametrize("row", ACCEPTED, ids=[r["id"] for r in ACCEPTED])
def test_kernel_name_is_the_recorded_one(row, monkeypatch):
    import lisp_mcmc_amd as mhx
    for k in kc.KNOBS:   # (read when the problem is finalised: at the first logpost)
        if row[k] == "-":
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, row[k])
    e, theta = kc.build(mhx, row)
    try:
        lp = e.logpost(theta)
        assert e.kernel_name() == row["expected"]
        assert lp.shape == (1,) and np.isfinite(lp[0])
    finally:
        e.close()
