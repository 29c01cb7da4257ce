"""Every call of tests/golden/icp_routes.json -- the smallest job lists on each side of every decision of the ICP
launcher's plan (sfe_icp_sweep_plan.h) -- takes the recorded route for every job on a device with the recorded CU count,
and gives the status, the iteration count and the pose of the same call with every job on the 1024-thread builds
(tuning sw_tiers = 0, sw_multi = 0, sw_tiny = 0): bit for bit, as tests/test_gpu_icp_tiers.py compares the two, and
within its 1e-6 for jobs shared by several workgroups (their sums are added share by share).  Which kernels a call
launches is not visible from here: tools/icp_routes.py shows it under a kernel trace, and tests/test_icp_plan_rules.py
checks the plan against the recorded trace on the CPU.  The calls are made by the tool's make_call on its synthetic
clouds."""
import importlib.util
import os

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("icp_routes", os.path.join(ROOT, "tools", "icp_routes.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

FIXTURE = tool.load_fixture()
TOL_SPLIT = 1e-6
ONE_SIZE = dict(sw_tiers=0, sw_multi=0, sw_tiny=0)
pytestmark = pytest.mark.gpu


def _pose_diff(Ta, Tb):
    a, b = synth.pose_of(Ta), synth.pose_of(Tb)
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]), abs(np.arctan2(np.sin(a[2] - b[2]), np.cos(a[2] - b[2]))))


@pytest.mark.parametrize("call", FIXTURE["calls"], ids=lambda c: c["name"])
def test_call_takes_the_recorded_routes(ctx, call):
    assert ctx.n_cu == FIXTURE["n_cu"]
    clouds = tool.clouds_of(call)
    T, status, iters, routes = tool.make_call(ctx, call, clouds)
    assert tool.runs_of(routes) == call["routes"]
    T1, status1, iters1, routes1 = tool.make_call(ctx, call, clouds, **ONE_SIZE)
    assert set(routes1) <= {L.ICP_ROUTE_Q, L.ICP_ROUTE_LDS, L.ICP_ROUTE_GLB}
    assert np.array_equal(status, status1) and np.array_equal(iters, iters1)
    for j, r in enumerate(routes):
        if r == L.ICP_ROUTE_SPLIT:
            assert status[j] != 0 or _pose_diff(T[j], T1[j]) < TOL_SPLIT, (j, _pose_diff(T[j], T1[j]))
        else:
            assert np.array_equal(T[j], T1[j], equal_nan=True), j
