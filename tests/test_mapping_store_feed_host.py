"""The host side of the store feed of a single map (Mapping.add_keyframe_store, replay.FrontEnd(mapping=...)): the ABI, the
`mapping` argument's checks, the feed counters and the hit table both map classes hand the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
import mapping_ref  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd import mapping, replay  # noqa: E402

NEW = ("sfe_map_hit_table", "sfe_map_measure_store", "sfe_map_measure_store_undecided", "sfe_map_measure_store_finish")


def test_single_map_store_feed_entry_points_are_declared_and_typed():
    header = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    for name in NEW:
        assert name + "(" in header and name in _lib.SIGNATURES, name
        # the set's contract with the `maps` argument dropped: one int32 pointer fewer, nothing else
        twin = _lib.SIGNATURES[name.replace("sfe_map_", "sfe_mapset_")]
        res, args = _lib.SIGNATURES[name]
        assert res is twin[0]
        if name == "sfe_map_measure_store":
            assert list(args) == list(twin[1][:3]) + list(twin[1][4:])
        else:
            assert list(args) == list(twin[1])
    lib = _lib.load_library()          # dlopen works without a GPU
    for name in NEW:
        assert hasattr(lib, name), name
    assert hasattr(mapping.Mapping, "add_keyframe_store")


def test_front_end_checks_its_mapping_argument_before_anything_is_allocated():
    ping = mapping_ref.SessionPing(64, 128, 0.1)
    with pytest.raises(ValueError, match="needs a `ping`"):
        replay.FrontEnd(None, mapping=dict(feed="store"))
    for feed in ("device", "", None, 1):
        with pytest.raises(ValueError, match="feed must be"):
            replay.FrontEnd(None, mapping=dict(ping=ping, feed=feed))
    with pytest.raises(ValueError, match="needs a `store`"):
        replay.FrontEnd(None, mapping=dict(ping=ping, feed="store"))
    # (each of them before pcl.ICP(ctx), the first thing the constructor makes: with ctx=None and no GPU that would raise
    #  something else)


def test_feed_stats_are_zero_after_construction():
    m = mapping.Mapping()
    assert m.feed_stats == {"points": 0, "undecided": 0, "calls": 0}
    assert m.point_cloud is None
    pts = np.zeros((3, 2))
    m.point_cloud = pts                 # assigning keeps working
    assert m.point_cloud is pts


@pytest.mark.parametrize("geom", [(128, 256, 0.04), (256, 128, 0.08), (512, 1024, np.float64(30.0 / 1024))])
def test_hit_table_helper_hands_out_the_spline_table_and_the_margin(geom):
    """mapping.hit_table_args for a Mapping = spline_table / guard_margin of its oculus, its skips and its ranges; and
    device_hit_table registers a geometry once"""
    m = mapping.Mapping()
    m._configure_host()
    ping = mapping_ref.SessionPing(*geom)
    m._register_geometry = lambda xy, shape: 0          # (no device here)
    m._new_keyframe(None, ping)
    o = m.oculus
    breaks, coef = mapping.spline_table(o)
    bearings, nb, b, c, n_iv, margin, num_ranges, res, wide, r_skip, c_skip = mapping.hit_table_args(m)
    assert bearings.dtype == np.float32 and np.array_equal(bearings, o.bearings) and nb == len(o.bearings) == geom[0]
    assert np.array_equal(b, breaks) and np.array_equal(c, coef) and n_iv == len(coef) == len(breaks) - 1
    assert margin == mapping.guard_margin(o, breaks, coef)
    assert (num_ranges, res) == (geom[1], float(geom[2]))
    assert wide == int((np.float32(1.0) / geom[2]).dtype == np.float64)     # the row's arithmetic, as numpy promotes it
    assert (r_skip, c_skip) == (int(m.oculus_r_skip), int(m.oculus_c_skip))
    # stored once per geometry, under the key _register_geometry's owner took
    m._hit_key = mapping.Mapping._new_hit_key(m)
    calls, tabs = [], {}

    def register(*args):
        calls.append(args)
        args[-1]._obj.value = 7
        return 0
    m._check = lambda rc: rc
    assert mapping.device_hit_table(m, tabs, register) == 7 and mapping.device_hit_table(m, tabs, register) == 7
    assert len(calls) == 1 and list(tabs) == [m._hit_key]
    assert calls[0][1:2] + calls[0][4:11] == (nb, n_iv, margin, num_ranges, res, wide, r_skip, c_skip)
