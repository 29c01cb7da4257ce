"""CPU side of chained.SessionBatch(nssm_enable=True): its arguments are FrontEnd's (same defaults, same assertions), the search's
host decisions are the functions FrontEnd itself runs, and the many-job store entry points are declared in the C header and
typed in _lib (their device results: tests/test_gpu_chained_loop_closure.py)."""
import inspect
import os

import numpy as np
import pytest

from sonar_slam_amd import _lib, chained, replay
from sonar_slam_amd.pose2 import Pose2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANY = ("sfe_cloud_store_get_points_keys_many", "sfe_cloud_store_fov_select_many", "sfe_cloud_store_compact_selected_many",
        "sfe_cloud_store_match_keys_many")
NSSM_ARGS = ("nssm_initialization", "nssm_initialization_params", "nssm_min_st_sep", "nssm_min_points", "nssm_max_translation",
             "nssm_max_rotation", "nssm_source_frames", "nssm_cov_samples", "oculus_max_range", "oculus_horizontal_aperture",
             "mcd_random_state")


def test_session_batch_takes_the_front_end_search_arguments_with_their_defaults():
    sb = inspect.signature(chained.SessionBatch.__init__).parameters
    fe = inspect.signature(replay.FrontEnd.__init__).parameters
    for name in NSSM_ARGS:
        assert name in sb, name
        assert np.array_equal(np.asarray(sb[name].default, dtype=object), np.asarray(fe[name].default, dtype=object)), name
    assert sb["nssm_enable"].default is False                   # an existing batch runs, sizes and records what it did


@pytest.mark.parametrize("kw", [dict(nssm_source_frames=8), dict(nssm_min_st_sep=4, nssm_source_frames=5),
                                dict(nssm_cov_samples=500)])
def test_session_batch_refuses_what_front_end_refuses(kw):
    with pytest.raises(AssertionError):
        replay.FrontEnd(None, **kw)
    with pytest.raises(AssertionError):      # (before anything touches the device)
        chained.SessionBatch(None, None, None, "SOCA", 65, None, 2, 10, np.zeros((2, 10, 3)), nssm_enable=True, **kw)


def test_many_job_entry_points_are_declared_and_typed():
    header = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    for name in MANY:
        assert name + "(" in header and name in _lib.SIGNATURES, name


def test_shared_host_decisions_are_what_front_end_runs():
    """FrontEnd's field-of-view bounds are replay.fov_bounds; the MinCovDet step of compute_icp_with_cov is
    replay.robust_covariance; the gate is replay.large_transformation"""
    rng = np.random.default_rng(1)
    fe = replay.FrontEnd(None)
    covs = [np.diag(rng.uniform(0.01, 0.2, 3)) for _ in range(3)]
    fe.keyframes = []
    for c in covs:
        kf = replay.Keyframe(True, 0.0, Pose2())
        kf.pose, kf.cov = Pose2(*rng.normal(0, 3, 3)), c
        fe.keyframes.append(kf)
    a = fe._fov_bounds([2, 1, 0])
    b = replay.fov_bounds([fe.keyframes[f].pose for f in (2, 1, 0)], [covs[f] for f in (2, 1, 0)], fe.oculus_max_range,
                          fe.oculus_horizontal_aperture)
    assert a[1] == b[1] and a[2] == b[2] and [t.matrix().tolist() for t in a[0]] == [t.matrix().tolist() for t in b[0]]
    bounds = replay.nssm_pose_bounds(covs[0])
    assert bounds.shape == (3, 2) and np.all(bounds[:, 0] == -bounds[:, 1])
    Ts = np.zeros((12, 3, 3), np.float32)
    for i, p in enumerate(rng.normal(0, [0.2, 0.2, 0.02], (12, 3))):
        Ts[i] = Pose2(*p).matrix()
    ok = np.arange(12) % 5 != 0
    msg, centre, cov, xyt = replay.robust_covariance(Ts, ok, 0, fe.icp_odom_sigmas)
    assert msg == "success" and len(xyt) == ok.sum() and xyt.dtype == np.float32 and cov.shape == (3, 3)
    assert replay.robust_covariance(Ts[:4], np.ones(4, bool), 0, fe.icp_odom_sigmas)[0] == "Too few samples for covariance computation"
    assert replay.large_transformation(Pose2(), Pose2(11.0, 0.0, 0.0), 10.0, 1.0)
    assert not replay.large_transformation(Pose2(), Pose2(1.0, 0.0, 0.5), 10.0, 1.0)
