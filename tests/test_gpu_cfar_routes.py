"""Every call of tests/golden/cfar_routes.json -- the smallest shapes on each side of every decision of the CFAR route
(sfe_cfar_route.h) -- gives the oracle's mask, and the oracle's threshold map where one is asked, bit for bit.  Which
kernel a call takes is not visible from here: tools/cfar_routes.py shows it under a kernel trace, and
tests/test_cfar_route_rules.py checks the route against the recorded trace on the CPU.  The calls are made by the tool's
make_call (device pointers offset inside larger allocations for the unaligned cases, bit streams unpacked on the host with
their pad bits zero); images are uniform random uint8 with the last frame all 255."""
import importlib.util
import os

import numpy as np
import pytest

import oracle
from sonar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("cfar_routes", os.path.join(ROOT, "tools", "cfar_routes.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

CALLS = tool.load_calls()
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("call", [c for c in CALLS if c["expect"] != "refused"], ids=lambda c: c["name"])
def test_call_equals_the_oracle(ctx, call):
    frames = tool.frames_of(call)
    rc, masks, thr = tool.make_call(ctx, call, frames)
    assert rc == 0
    for f, img in enumerate(frames):
        want = oracle.cfar(img, call["alg"], call["T"], call["G"], call["tau"], k=call["k"], want_threshold=call["thr"])
        want_mask, want_thr = want if call["thr"] else (want, None)
        if call["gate"] >= 0:
            want_mask = oracle.gate(img, want_mask, call["gate"])
        assert np.array_equal(masks[f], want_mask), f
        if call["thr"]:
            assert thr[f].tobytes() == np.asarray(want_thr, np.float32).tobytes(), f


@pytest.mark.parametrize("call", [c for c in CALLS if c["expect"] == "refused"], ids=lambda c: c["name"])
def test_refused_call_leaves_the_context_usable(ctx, call):
    rc, _, _ = tool.make_call(ctx, call, tool.frames_of(call))
    assert rc == _lib.SFE_ERR_ARG
    nxt = CALLS[0]
    frames = tool.frames_of(nxt)
    rc, masks, _ = tool.make_call(ctx, nxt, frames)
    assert rc == 0
    assert np.array_equal(masks[0], oracle.cfar(frames[0], nxt["alg"], nxt["T"], nxt["G"], nxt["tau"]))
