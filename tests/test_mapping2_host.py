"""Method 2 (get_occupancy_grid2) without a device: the numpy restatement (tests/mapping2_ref.py) and the product's host side
(the selection of the cloud, the known region and the sizes) against tests/golden/mapping2_session.npz, which the
reference's own mapping.py wrote; and the two new entry points of the library."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import mapping2_ref  # noqa: E402
import oracle  # noqa: E402
from sonar_slam_amd import _lib, mapping  # noqa: E402

STAGES = ("adds", "lc")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(HERE, "golden", "mapping2_session.npz"))


@pytest.fixture(scope="module")
def cells():
    """stage -> [(r, c) or None per key]: the reference's cell lists, as mapping_session.npz recorded them"""
    first = np.load(os.path.join(HERE, "golden", "mapping_session.npz"))
    n = 1 + max(int(k.split("_")[-1]) for k in first.files if k.startswith("r_adds_"))
    return {st: [(first["r_%s_%d" % (st, k)], first["c_%s_%d" % (st, k)]) if "r_%s_%d" % (st, k) in first.files else None
                 for k in range(n)] for st in STAGES}


def cases(fix):
    pubs = json.loads(str(fix["pubs"]))
    return [(st, name) + tuple(pubs[name]) for st in STAGES for name in pubs]


def stage_map(fix, stage, over):
    """the map's numbers at a stage, with a publication's changed settings"""
    s = json.loads(str(fix["stages"]))[stage]
    settings = json.loads(str(fix["settings"]))
    m = types.SimpleNamespace(x0=s["x0"], y0=s["y0"], resolution=settings["resolution"], dilate_size=int(fix["dilate_size"]),
                              outlier_filter_radius=settings["outlier_filter_radius"],
                              outlier_filter_min_points=settings["outlier_filter_min_points"])
    m.rmin, m.rmax, m.cmin, m.cmax = s["box"]
    for k, v in over.items():
        setattr(m, k, v)
    return m, s


def cloud_of(fix, stage, which):
    return np.zeros((0, 4), np.float32) if which == "empty" else fix["%s_%s" % (which, stage)]


def test_fixture_is_what_the_issue_describes(fix):
    assert [tuple(fix["pub_adds_%s_info" % n][[3, 2]].astype(int)) for n in ("all", "frames", "coarse", "frames_coarse")] == \
        [(177, 173), (158, 137), (71, 69), (44, 68)]
    assert int(fix["pub_adds_all_kept"]) < len(fix["pub_adds_all_points"])          # the filter drops points
    stages = json.loads(str(fix["stages"]))
    settings = json.loads(str(fix["settings"]))
    # the adds grow the map on top and on the left after the first cell lists were written; the loop closure grows it again
    assert stages["adds"]["x0"] < settings["x0"] and stages["adds"]["y0"] < settings["y0"]
    assert stages["lc"]["rows"] > stages["adds"]["rows"]
    assert {int(v) for v in np.unique(fix["pub_lc_all_data"])} == {-1, 0, 100}
    assert any("getStructuringElement" in s for s in json.loads(str(fix["stand_ins"])))


def test_restatement_equals_the_reference(fix, cells):
    for stage, name, kw, which, over in cases(fix):
        m, _ = stage_map(fix, stage, over)
        got = mapping2_ref.occupancy_grid2(m, cells[stage], cloud_of(fix, stage, which), oracle.remove_outlier, **kw)
        tag = "pub_%s_%s_" % (stage, name)
        assert np.array_equal(got["points"], fix[tag + "points"]) and got["points"].shape == fix[tag + "points"].shape, tag
        assert got["kept"] == int(fix[tag + "kept"]), tag
        assert list(got["box"]) == list(fix[tag + "box"]), tag
        assert list(got["info"]) == list(fix[tag + "info"]), tag
        assert got["data"].dtype == np.int8 and np.array_equal(got["data"].ravel(), fix[tag + "data"]), tag
    m, _ = stage_map(fix, "lc", {})
    with pytest.raises(IndexError):
        mapping2_ref.occupancy_grid2(m, cells["lc"], fix["cloud32_lc"], oracle.remove_outlier, frames=[3, 99])


def host_map(fix, stage, over):
    """a Mapping with the host state of a stage and no device: keyframes that carry their box and slot"""
    ref, s = stage_map(fix, stage, over)
    m = mapping.Mapping()
    for k, v in json.loads(str(fix["settings"])).items():
        setattr(m, k, v)
    m._configure_host()
    for k in ("x0", "y0", "rmin", "rmax", "cmin", "cmax", "dilate_size", "outlier_filter_min_points"):
        setattr(m, k, getattr(ref, k))
    m.rows, m.cols = s["rows"], s["cols"]
    for key, box in enumerate(s["kf_boxes"]):
        kf = None
        if box is not None:
            kf = mapping.Submap(m, len([k for k in m.keyframes if k is not None]))
            kf.k, kf.box, kf.base = key, tuple(box), (0, 0)
        m.keyframes.append(kf)
    return m


def test_host_selection_and_plan_equal_the_reference(fix):
    for stage, name, kw, which, over in cases(fix):
        tag = "pub_%s_%s_" % (stage, name)
        m = host_map(fix, stage, over)
        pts = mapping.select_points(cloud_of(fix, stage, which), kw.get("frames"))
        want = fix[tag + "points"]
        assert pts.shape == want.shape and np.array_equal(pts, want), tag
        assert pts.dtype == (np.float64 if "frames" in kw or which == "cloud64" else np.float32), tag
        slots, box, (y0, x0), (oh, ow), inv, resize, resolution = m._render2_plan(kw.get("frames"), kw.get("resolution"))
        info = fix[tag + "info"]
        assert list(box) == list(fix[tag + "box"]), tag
        assert [x0, y0, ow, oh, resolution] == list(info), tag
        listed = [k for k in (kw["frames"] if "frames" in kw else range(len(m.keyframes)))
                  if k < len(m.keyframes) and m.keyframes[k] is not None]
        assert list(slots) == [m.keyframes[k]._slot for k in listed], tag         # a key listed twice is marked twice
        h, w = box[1] - box[0] + 1, box[3] - box[2] + 1
        assert (resize == 0 and (oh, ow) == (h, w) and inv == 1.0) or (resize == 1 and inv == kw["resolution"] / m.resolution)
        msg = m._grid_msg(box, resolution, np.zeros((oh, ow), np.int8), (y0, x0))
        assert [msg.info.origin.position.x, msg.info.origin.position.y, msg.info.width, msg.info.height,
                msg.info.resolution] == list(info), tag
    with pytest.raises(IndexError, match="known region"):
        host_map(fix, "adds", {})._render2_plan([3, 99], None)


def test_what_is_missing_is_named():
    m = mapping.Mapping()
    with pytest.raises(NotImplementedError, match="configure"):         # (an unconfigured map keeps its old answer)
        m.get_occupancy_grid2()
    m._configure_host()
    with pytest.raises(RuntimeError, match="point_cloud"):
        m.get_occupancy_grid2()
    m.pub_occupancy2 = False
    m.point_cloud = np.zeros((3, 4), np.float32)
    with pytest.raises(RuntimeError, match="pub_occupancy2=False"):
        m.get_occupancy_grid2()
    with pytest.raises(NotImplementedError, match="get_intensity_grid"):
        m.get_intensity_grid()


def test_library_declares_and_exports_render2():
    hdr = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    declared = set(re.findall(r"\b(sfe_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()          # dlopen works without a GPU
    for name in ("sfe_map_render2", "sfe_mapset_render2"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
