"""The lists of the device sources agree with what the sources include.

The Makefile's DEV is the one list of what libmhx.so embeds for hiprtc (tools/embed_src.py and
tools/rtc_check.py read it); kStepHeaders (csrc/mhx_rtc.cpp) is the hand-written list of what a
stepping program is handed.  A device header added to an #include chain and to neither list compiles
ahead of time and fails at the first run-time compile, on a GPU: here it fails on the CPU.  And the
model-free read-out kernels, which only the primary family's unit compiles, are in neither."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lisp-mcmc_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import embed_src  # noqa: E402


def reached(start):
    """the files reached from csrc/<start> by quoted #includes, start included, as paths"""
    seen, todo = set(), [os.path.join(CSRC, start)]
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        with open(path) as f:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                todo.append(os.path.join(os.path.dirname(path), inc))
    return seen


def step_headers():
    """the names in kStepHeaders, as paths"""
    with open(os.path.join(CSRC, "mhx_rtc.cpp")) as f:
        body = re.search(r"kStepHeaders = \{(.*?)\};", f.read(), re.S).group(1)
    names = re.findall(r'\{kSrc_\w+, "([^"]+)"\}', body)
    assert names
    return {os.path.normpath(os.path.join(CSRC, n)) for n in names}


def test_every_device_source_is_listed():
    dev = {path for _, path in embed_src.dev_files()}
    step = reached("mhx_kernels.hpp")
    derived = reached("mhx_derived.hpp")
    assert os.path.join(CSRC, "mhx_kernels.hpp") in step and os.path.join(CSRC, "mhx_kernels.hpp") in derived
    assert step <= dev, sorted(step - dev)
    assert derived <= dev, sorted(derived - dev)
    assert step <= step_headers(), sorted(step - step_headers())
    free = os.path.join(CSRC, "mhx_readout_kernels.hpp")
    assert os.path.exists(free)
    assert free not in dev and free not in step_headers()
