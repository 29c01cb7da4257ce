"""CPU checks of the intensity mosaic: tests/intensity_ref.py against the reference's recorded session
(tests/golden/intensity_session.npz, written by the reference's own mapping.py with pub_intensity), the ``intensity_skips``
setting, the per-cell expression of csrc/sfe_map_intensity.h against numpy, and the new symbols."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import intensity_ref  # noqa: E402
import oracle  # noqa: E402
from make_golden import Pose2  # noqa: E402
from sonar_slam_amd import _lib, mapping  # noqa: E402

NEW = ["sfe_%s_%s" % (kind, name) for kind in ("map", "mapset")
       for name in ("enable_intensity", "set_intensity", "set_intensity_dev", "render_intensity", "read_intensity",
                    "slot_intensity")]


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(HERE, "golden", "intensity_session.npz"))


@pytest.fixture(scope="module")
def map_fix():
    return np.load(os.path.join(HERE, "golden", "mapping_session.npz"))


@pytest.mark.parametrize("image_kw", [True, False])
def test_restatement_reproduces_the_reference_session(fix, map_fix, image_kw):
    """box, origin, size and the digests of both grids and of every keyframe's i after every step; the cropped grids and three
    keyframes' i in full after the adds and after the loop closure; the published image and its info"""
    settings, geoms, steps, points, _ = intensity_ref.fixture_session(fix, map_fix)
    m = intensity_ref.Mapping()
    m.remove_outlier = oracle.remove_outlier
    for k, v in settings.items():
        setattr(m, k, v)
    m.configure()

    def check(i, st):
        got = dict(box=[int(m.rmin), int(m.rmax), int(m.cmin), int(m.cmax)], x0=m.x0, y0=m.y0, rows=m.rows, cols=m.cols,
                   intensity=intensity_ref.sha(m.intensity_grid), counter=intensity_ref.sha(m.counter_grid),
                   i=intensity_ref.kf_i_digest(m))
        for k, v in got.items():
            assert v == st[k], (i, k)
        if st["op"] == "add":
            assert [int(m.oculus_r_skip), int(m.oculus_c_skip)] == st["skips"] and list(m.oculus_image_size) == st["image"]
        last = i + 1 == len(steps) or steps[i + 1].get("pass_") != st.get("pass_")
        tag = {"add": "adds"}.get(st["op"], st.get("pass_"))
        if last and "intensity_%s" % tag in fix:
            box = (slice(m.rmin, m.rmax + 1), slice(m.cmin, m.cmax + 1))
            assert np.array_equal(m.intensity_grid[box], fix["intensity_%s" % tag])
            assert np.array_equal(m.counter_grid[box], fix["counter_%s" % tag])
            for k in (0, 7, 19):
                assert np.array_equal(m.keyframes[k].i, fix["i_%s_%d" % (tag, k)])

    intensity_ref.replay(m, steps, geoms, points, Pose2, check=check, image_kw=image_kw)
    msg = m.get_intensity_grid()
    assert np.array_equal(np.array(msg.data, np.int8), fix["pub_data"])
    assert intensity_ref.info_of(msg) == list(fix["pub_info"])


def test_session_covers_what_it_should(fix):
    steps = json.loads(str(fix["steps"]))
    adds = [s for s in steps if s["op"] == "add"]
    assert 3 not in [s["key"] for s in adds] and {tuple(s["skips"]) for s in adds} == {(5, 1), (2, 2)}
    assert [r for r in dict.fromkeys(s["rows"] for s in steps)][0] == 100 and max(s["rows"] for s in steps) == 250
    assert len({s["rows"] for s in steps if s.get("pass_") == "lc"}) > 1      # growth in the middle of the pose pass
    assert {s["cols"] for s in steps} == {240}                                 # (the reference's column growth raises)
    data = fix["pub_data"]
    assert data.min() == -1 and data.max() == 100 and int(fix["ties"]) > 0
    stand_ins = json.loads(str(fix["stand_ins"]))
    assert any("r_skip" in s for s in stand_ins) and any("r2n" in s for s in stand_ins) and len(stand_ins) == 7


def test_intensity_skips_setting():
    assert "intensity_skips" in mapping.SETTINGS and mapping.Mapping().intensity_skips is None
    # the default keeps the refusals, and says why and what to set
    m = mapping.Mapping()
    m.pub_intensity = True
    with pytest.raises(NotImplementedError, match="pub_intensity") as e:
        m.configure()
    assert "mapping.py:242" in str(e.value) and "intensity_skips" in str(e.value)
    with pytest.raises(NotImplementedError, match="pub_intensity"):
        mapping.MapBatch(None, 2, 4, pub_intensity=True).configure()
    # "oculus" passes the host side of configure
    m.intensity_skips = "oculus"
    m._configure_host()
    assert m._intensity and (m.rows, m.cols) == (500, 500)
    assert m.intensity_grid is None and m.counter_grid is None           # (no device map yet)
    with pytest.raises(NotImplementedError, match="get_intensity_grid"):
        m.get_intensity_grid()
    # anything else is a ValueError, with pub_intensity or without
    for pub in (True, False):
        m = mapping.Mapping()
        m.pub_intensity, m.intensity_skips = pub, "sonar"
        with pytest.raises(ValueError, match="intensity_skips"):
            m._configure_host()
        with pytest.raises(ValueError, match="intensity_skips"):
            mapping.MapBatch(None, 2, 4, pub_intensity=pub, intensity_skips=(5, 1)).configure()
    # MapBatch takes the setting; a misspelt one is still a TypeError
    b = mapping.MapBatch(None, 2, 4, pub_intensity=True, intensity_skips="oculus")
    assert (b.pub_intensity, b.intensity_skips) == (True, "oculus")
    with pytest.raises(TypeError, match="unknown setting 'intensity_skip'"):
        mapping.MapBatch(None, 2, 4, intensity_skip="oculus")
    with pytest.raises(NotImplementedError, match="get_intensity_grid"):
        b.get_intensity_grid()


def test_front_end_refuses_the_mosaic():
    from sonar_slam_amd import replay
    ping = intensity_ref.Ping(128, 256, 0.04)
    with pytest.raises(ValueError, match=r"Mapping\.add_keyframe"):
        replay.FrontEnd(None, mapping=dict(ping=ping, pub_intensity=True, intensity_skips="oculus"))


def test_cell_expression_equals_numpy(tmp_path):
    """csrc/sfe_map_intensity.h, built for the host, against np.int8(np.round(I / 255.0 * 100.0 / cnt)) for every cnt in
    1 .. 64 crossed with every I in 0 .. 255 cnt (and -1 for cnt = 0)"""
    exe, out = str(tmp_path / "map_intensity_check"), str(tmp_path / "values.bin")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "map_intensity_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe, "64", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert r.returncode == 0 and "map_intensity_check: ok" in r.stdout, r.stdout
    got = np.fromfile(out, np.int8)
    want = [np.full(256, -1, np.int8)]
    for cnt in range(1, 65):
        inten = np.arange(255 * cnt + 1, dtype=np.uint32)
        want.append(np.int8(np.round(inten / 255.0 * 100.0 / np.full(len(inten), cnt, np.uint16))))
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
    # the ties that tell half-even from half-up
    at = lambda inten, cnt: int(got[256 + sum(255 * c + 1 for c in range(1, cnt)) + inten])
    assert [at(51, 8), at(255, 8), at(153, 8), at(357, 8)] == [2, 12, 8, 18]


def test_new_symbols_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    declared = set(re.findall(r"\b(sfe_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
