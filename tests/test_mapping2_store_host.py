"""The store route of method 2 without a device (Mapping.get_occupancy_grid2_store, FrontEnd.occupancy_grid2): the three new
entry points of the library, the refusals that need no device, and the selection's multiset rule -- what the device makes of
a frame list -- restated here and held to mapping.select_points."""
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import mapping2_ref  # noqa: E402
import oracle  # noqa: E402
from sonar_slam_amd import _lib, mapping, replay  # noqa: E402

NEW = ("sfe_map_render2_store", "sfe_mapset_render2_store", "sfe_cloud_store_put_keys")


def test_library_declares_and_exports_the_store_route():
    hdr = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    declared = set(re.findall(r"\b(sfe_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()          # dlopen works without a GPU
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # the argument counts of the declarations are those the Python side passes
    for name in NEW:
        args = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


class _Store(object):
    ctx = None
    handle = None


def test_what_is_missing_is_named():
    m = mapping.Mapping()
    with pytest.raises(NotImplementedError, match="configure"):
        m.get_occupancy_grid2_store(_Store(), 0)
    m.pub_occupancy2 = False
    m._configure_host()
    with pytest.raises(RuntimeError, match="pub_occupancy2=False"):
        m.get_occupancy_grid2_store(_Store(), 0)
    b = mapping.MapBatch(None, 2)
    with pytest.raises(NotImplementedError, match="configure"):
        b.get_occupancy_grid2_store(_Store(), [0, 1])


def test_front_end_names_what_it_lacks():
    fe = replay.FrontEnd(None)
    with pytest.raises(RuntimeError, match="no map"):
        fe.occupancy_grid2()
    fe.map = mapping.Mapping()
    fe.map._configure_host()
    with pytest.raises(RuntimeError, match="no store"):
        fe.occupancy_grid2()
    fe.map.pub_occupancy2 = False
    with pytest.raises(RuntimeError, match="pub_occupancy2=False"):
        fe.occupancy_grid2()


def multiplicity(keys, frames):
    """the device's rule (map2_select_kernel): a point is taken once for every list entry that equals its key"""
    listed = mapping.frame_list(frames)
    return np.array([int(np.sum(listed == k)) for k in keys], np.int64)


def rows_of(points):
    return Counter(tuple(p) for p in np.asarray(points, np.float64))


@pytest.mark.parametrize("frames", [[1, 0], [0, 0, 2], [3], [-1, 2], [7, 1, 7, 7], [99, 4], [], [2.0, 1.5, 2 ** 31, 2 ** 40, -5],
                                    [np.int64(4), np.uint32(0)]])
def test_multiplicities_give_select_points_multiset(frames):
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 6, 200)
    cloud = np.c_[rng.normal(0, 5, (200, 2)), np.zeros(200), keys].astype(np.float32)
    want = rows_of(mapping.select_points(cloud, frames))
    assert want == rows_of(mapping2_ref.select(cloud, frames))
    mult = multiplicity(cloud[:, 3].astype(np.int64), frames)
    assert rows_of(np.repeat(cloud[:, :2], mult, axis=0)) == want
    assert mapping.frame_list(frames).dtype == np.int32 and len(mapping.frame_list(frames)) == len(frames)


def test_weighted_count_is_the_filter_over_the_repeated_rows():
    """the filter's decision over the multiset: every neighbour counts mult times, the point's own copies too; and on the
    cloud of tests/test_gpu_mapping2.py's grown map the doubled key changes what is kept (the case the device test renders)"""
    import test_gpu_mapping2 as base
    _, cloud = base.history_clouds(base.HISTORY, 3)
    radius, min_points = base.SETTINGS["outlier_filter_radius"], base.SETTINGS["outlier_filter_min_points"]
    kept = {}
    for frames in ([0, 2], [0, 0, 2]):
        mult = multiplicity(cloud[:, 3].astype(np.int64), frames)
        p = cloud[:, :2].astype(np.float32)
        d = p[:, None, :] - p[None, :, :]
        near = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) <= np.float32(radius * radius)
        keep = (mult > 0) & ((near * mult[None, :]).sum(axis=1) > min_points)
        want = oracle.remove_outlier(np.asarray(mapping.select_points(cloud, frames), np.float32), radius, min_points)
        assert rows_of(np.repeat(p, mult * keep, axis=0)) == rows_of(want), frames
        kept[len(frames)] = set(rows_of(want))
    assert len(kept[3] - kept[2]) >= 10 and kept[2] <= kept[3]
