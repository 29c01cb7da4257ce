"""GPU: ICP chains with data-point filters against the real bruce_slam.pcl (libpointmatcher), through the fixture
tools/pin_thirdparty.py writes on a machine that has the compiled module (tests/golden/thirdparty_pcl_dpf.npz).  Skipped
while the fixture is absent: the filter rules are restated from libpointmatcher's published source and unpinned until
then (icp_config)."""
import json
import os

import numpy as np
import pytest

from sonar_slam_amd import pcl, synth

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thirdparty_pcl_dpf.npz")
TOL_REF = 1e-4      # the bar of the other third-party pins: float sums in a different order


@pytest.mark.skipif(not os.path.exists(FIXTURE), reason="thirdparty_pcl_dpf.npz not pinned yet (tools/pin_thirdparty.py)")
def test_chains_with_filters_match_libpointmatcher(ctx, tmp_path):
    fix = np.load(FIXTURE)
    for name in json.loads(str(fix["chains"])):
        f = tmp_path / ("%s.yaml" % name)
        f.write_text(str(fix["yaml_" + name]))
        icp = pcl.ICP(ctx)
        icp.loadFromYaml(str(f))
        for k in range(3):
            msg, T = icp.compute(fix["src%d" % k], fix["tgt%d" % k], fix["guess%d" % k])
            assert msg == str(fix["msg_%s_%d" % (name, k)]), (name, k)
            a, b = synth.pose_of(T), synth.pose_of(fix["T_%s_%d" % (name, k)])
            assert max(abs(x - y) for x, y in zip(a, b)) < TOL_REF, (name, k)
