#!/usr/bin/env python
"""Pin the ORACLE to the real third-party libraries, on a machine that has them.

The arithmetic of SURVEY 8 rows a5 (cv2.remap), a7 (OctreeGridDataPointsFilter), a8 (RadiusOutlierRemoval), a12 (PM::ICP),
a14 (KDTreeMatcher), f2 (cv2.dilate) and f3 (applyColorMap) lives in OpenCV, PCL, libpointmatcher and libnabo.  None of
them is in the build image or on the GPU box, so `oracle/` restates their published behaviour and the parity of those rows is
"unpinned" (DESIGN 3).  This tool is the hook for the day a machine has the libraries:

    python tools/pin_thirdparty.py            # writes what it can, says what it skipped
    python -m pytest tests/test_golden.py -k thirdparty

  * `import cv2` works           -> tests/golden/thirdparty_cv2.npz: remap (0/1 mask and raw image, INTER_LINEAR) on two
                                    geometries, getStructuringElement(MORPH_ELLIPSE) for half sizes 1..6, dilate of sparse
                                    grids with them, applyColorMap(COLORMAP_JET) of all 256 levels
  * `from bruce_slam import pcl` -> tests/golden/thirdparty_pcl.npz: downsample (both overloads), remove_outlier, match, and
                                    ICP().loadFromYaml(icp.yaml as shipped).compute on scan pairs that succeed, on the two
                                    failure classes (messages and the guess returned, pcl.cpp:203,207-210), on 1-point clouds
                                 -> tests/golden/thirdparty_pcl_dpf.npz: ICP().loadFromYaml(chain).compute with each supported
                                    data-point filter and the libpointmatcher form of the point-to-plane chain (DPF_CHAINS;
                                    read by tests/test_gpu_icp_dpf_pin.py)

Each file holds the INPUTS next to the libraries' outputs (a fixture is data), the library versions, and is committed by
whoever ran this.  `tests/test_golden.py::test_oracle_matches_the_real_*` compare the oracle with them and are skipped while
the files are absent; `tests/golden/make_golden.py` picks the real modules up by the same probe (tests/golden/thirdparty.py).
Nothing here touches the product: the oracle is test infrastructure and so is this."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)
import thirdparty  # noqa: E402
from sonar_slam_amd import icp_config, synth  # noqa: E402
from sonar_slam_amd.feature_extraction import build_maps, oculus_bearings  # noqa: E402


def cv2_inputs():
    """the synthetic inputs of the cv2 fixture (seeded: the same on every machine)"""
    d = {}
    for i, (rows, beams) in enumerate([(256, 128), (512, 256)]):
        img = synth.sonar_frame(seed=300 + i, rows=rows, cols=beams, n_blobs=12)
        res, height, rows_, width, cols, map_x, map_y = build_maps(oculus_bearings(beams), 30.0 / rows, rows)
        rng = np.random.default_rng(310 + i)
        mask = (rng.random((rows, beams)) < 0.02).astype(np.uint8)       # a 0/1 image like `peaks` (feature_extraction.py:224)
        mask[rows // 3:rows // 3 + 3, 10:40] = 1                          # ... with a solid patch and an edge
        d.update({"img%d" % i: img, "mask%d" % i: mask, "map_x%d" % i: map_x, "map_y%d" % i: map_y})
    rng = np.random.default_rng(320)
    for i, (h, w, n) in enumerate([(90, 120, 60), (200, 160, 300)]):
        g = np.zeros((h, w), np.uint8)
        g[rng.integers(0, h, n), rng.integers(0, w, n)] = 255            # slam.py:516-521: target cells set to 255
        g[0, 0] = g[h - 1, w - 1] = 255                                   # the border cases
        d["grid%d" % i] = g
    return d


def cv2_fixture(cv2):
    """inputs + what `cv2` (the real module; the plumbing test passes the oracle's stand-in) makes of them"""
    d = cv2_inputs()
    for i in range(2):
        d["remap_mask%d" % i] = cv2.remap(d["mask%d" % i], d["map_x%d" % i], d["map_y%d" % i], cv2.INTER_LINEAR)
        d["remap_img%d" % i] = cv2.remap(d["img%d" % i], d["map_x%d" % i], d["map_y%d" % i], cv2.INTER_LINEAR)
    for hs in range(1, 7):
        k = cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (2 * hs + 1, 2 * hs + 1), (hs, hs))      # slam.py:522-526
        d["ellipse%d" % hs] = k
        for i in range(2):
            d["dilate%d_hs%d" % (i, hs)] = cv2.dilate(d["grid%d" % i], k)                          # slam.py:527
    d["jet"] = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(1, 256), cv2.COLORMAP_JET)[0]  # feature_extraction.py:227
    d["versions"] = np.array(json.dumps({"cv2": getattr(cv2, "__version__", "stand-in"), "numpy": np.__version__}))
    return d


def pin_cv2():
    cv2 = thirdparty.real_cv2()
    if cv2 is None:
        return "cv2 does not import here: thirdparty_cv2.npz not written"
    np.savez_compressed(os.path.join(GOLDEN, "thirdparty_cv2.npz"), **cv2_fixture(cv2))
    return "wrote thirdparty_cv2.npz (OpenCV %s)" % cv2.__version__


def pcl_inputs():
    d = {}
    rng = np.random.default_rng(400)
    # feature-cloud-like inputs of the two filters (feature_extraction.py:241-249): clustered points + scatter, duplicates,
    # one point, none
    clouds = []
    for n in (1500, 300, 1, 0):
        c = np.r_[rng.normal(0, 0.4, (n // 2, 2)) * [3.0, 0.3] + [12.0, 1.0], rng.uniform([1, -20], [29, 20], (n - n // 2, 2))]
        clouds.append(np.ascontiguousarray(c, np.float32))
    clouds[1][10:20] = clouds[1][0]                                       # exact duplicates
    for i, c in enumerate(clouds):
        d["cloud%d" % i] = c
        d["keys%d" % i] = rng.integers(0, 9, len(c)).astype(np.float32)
    d["n_clouds"] = len(clouds)
    # scan pairs: converging ones, and the failure classes of pcl.cpp:207-210
    pairs = [synth.scan_pair(seed=410 + i, n_src=n, n_tgt=m) for i, (n, m) in enumerate([(800, 900), (2500, 2300), (300, 260)])]
    far = synth.scan_pair(seed=420, n_src=200, n_tgt=200)
    far_src = far[0] + np.float32(500.0)                                  # nothing within maxDist: "no outlier to filter" class
    one = (np.array([[3.0, 1.0]], np.float32), np.array([[3.1, 1.05]], np.float32), np.eye(3, dtype=np.float32))
    jobs = [(s, t, g) for s, t, g, _ in pairs] + [(far_src, far[1], far[2]), one]
    for i, (s, t, g) in enumerate(jobs):
        d["src%d" % i], d["tgt%d" % i], d["guess%d" % i] = s, t, np.asarray(g, np.float32)
    d["n_jobs"] = len(jobs)
    return d


def find_icp_yaml(pcl):
    """bruce_slam/config/icp.yaml of the checkout the compiled module came from (slam.py:99-100 loads it by that name)"""
    for a in sys.argv[1:]:
        if a.startswith("--icp-yaml="):
            return a.split("=", 1)[1]
    here = os.path.dirname(os.path.abspath(getattr(pcl, "__file__", "")))
    for up in ("../../config", "../../../config", "../config"):
        cand = os.path.normpath(os.path.join(here, up, "icp.yaml"))
        if os.path.isfile(cand):
            return cand
    cand = "/root/reference/bruce_slam/config/icp.yaml"
    return cand if os.path.isfile(cand) else None


def pcl_fixture(pcl, icp_compute, versions):
    """inputs + what `pcl` / `icp_compute` (the real compiled module and ICP().loadFromYaml(icp.yaml).compute; the plumbing
    test passes the oracle's stand-ins) make of them"""
    d = pcl_inputs()
    for i in range(int(d["n_clouds"])):
        c, k = d["cloud%d" % i], d["keys%d" % i]
        for res in (0.5, 0.25):
            tag = "%d_res%03d" % (i, int(res * 100))
            d["down" + tag] = np.asarray(pcl.downsample(c, res), np.float32).reshape(-1, 2)        # pcl.cpp:128-141
            p2, k2 = pcl.downsample(c, k.reshape(-1, 1), res)                                       # pcl.cpp:143-159
            d["downk_points" + tag] = np.asarray(p2, np.float32).reshape(-1, 2)
            d["downk_keys" + tag] = np.asarray(k2, np.float32).reshape(-1)
        for radius, min_points in ((1.0, 5), (0.5, 2)):
            d["outlier%d_r%03d_k%d" % (i, int(radius * 100), min_points)] = \
                np.asarray(pcl.remove_outlier(c, radius, min_points), np.float32).reshape(-1, 2)    # pcl.cpp:54-74
    for i in range(int(d["n_jobs"])):
        s, t, g = d["src%d" % i], d["tgt%d" % i], d["guess%d" % i]
        for md in (0.5, 3.0):
            ids, dist = pcl.match(t, s, 1, md)                                                      # pcl.cpp:161-174
            d["match_ids%d_md%03d" % (i, int(md * 100))] = np.asarray(ids, np.int32).reshape(1, -1)
            d["match_d2%d_md%03d" % (i, int(md * 100))] = np.asarray(dist, np.float32).reshape(1, -1)
        msg, T = icp_compute(s, t, g)                                                               # pcl.cpp:198-212
        d["icp_msg%d" % i], d["icp_T%d" % i] = np.array(str(msg)), np.asarray(T, np.float32)
    d["versions"] = np.array(json.dumps(versions))
    return d


def pin_pcl():
    pcl = thirdparty.real_pcl()
    if pcl is None:
        return "bruce_slam.pcl does not import here (no catkin workspace with the compiled module): thirdparty_pcl.npz not written"
    yaml_path = find_icp_yaml(pcl)
    if yaml_path is None:
        return "icp.yaml not found (pass --icp-yaml=PATH): thirdparty_pcl.npz not written"
    icp = pcl.ICP()
    icp.loadFromYaml(yaml_path)
    d = pcl_fixture(pcl, icp.compute, {"bruce_slam.pcl": getattr(pcl, "__file__", "?"), "numpy": np.__version__,
                                       "icp_yaml": yaml_path})
    # (the chain the yaml configures, as this repo's parser reads it: the check refuses a fixture made with another chain)
    d["icp_yaml_params"] = np.array(json.dumps(icp_config.parse_icp_yaml(open(yaml_path).read()).as_dict()))
    np.savez_compressed(os.path.join(GOLDEN, "thirdparty_pcl.npz"), **d)
    return "wrote thirdparty_pcl.npz"


# ICP chains with data-point filters (icp_config.parse_icp_chain): (name, readingDataPointsFilters entries,
# referenceDataPointsFilters entries, point-to-plane?) spliced into the shipped icp.yaml
DPF_CHAINS = [
    ("reading_maxdist", "  - MaxDistDataPointsFilter:\n      maxDist: 15\n", "", False),
    ("reference_maxdist_y", "", "  - MaxDistDataPointsFilter:\n      dim: 1\n      maxDist: 8\n", False),
    ("reading_mindist", "  - MinDistDataPointsFilter:\n      minDist: 2\n", "", False),
    ("reference_box", "", "  - BoundingBoxDataPointsFilter:\n      xMin: -3\n      xMax: 3\n      yMin: -3\n"
                          "      yMax: 3\n      removeInside: 1\n", False),
    ("both_octree", "  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.3\n      samplingMethod: 3\n",
     "  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.2\n      samplingMethod: 3\n", False),
    ("point_to_plane_normals", "", "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n      epsilon: 0\n"
                                   "      keepNormals: 1\n", True),
]


def dpf_chain_yaml(shipped, reading, reference, point_to_plane):
    y = shipped.replace("readingDataPointsFilters:\n", "readingDataPointsFilters:\n" + reading, 1).replace(
        "referenceDataPointsFilters:\n", "referenceDataPointsFilters:\n" + reference, 1)
    if point_to_plane:
        y = y.replace("  PointToPointErrorMinimizer\n", "").replace(
            "  # PointToPlaneErrorMinimizer:\n  #   force2D: 1", "  PointToPlaneErrorMinimizer:\n    force2D: 1")
    icp_config.parse_icp_chain(y)       # (a chain this repo's parser refuses is not worth pinning)
    return y


def pin_pcl_dpf():
    """tests/golden/thirdparty_pcl_dpf.npz: ICP().loadFromYaml(chain).compute for every chain of DPF_CHAINS on three scan
    pairs; the fixture holds the chains' YAML, the inputs and the outputs (tests/test_gpu_icp_dpf_pin.py reads it)"""
    import tempfile
    pcl = thirdparty.real_pcl()
    if pcl is None:
        return "bruce_slam.pcl does not import here: thirdparty_pcl_dpf.npz not written"
    yaml_path = find_icp_yaml(pcl)
    if yaml_path is None:
        return "icp.yaml not found (pass --icp-yaml=PATH): thirdparty_pcl_dpf.npz not written"
    shipped = open(yaml_path).read()
    d = {"versions": np.array(json.dumps({"bruce_slam.pcl": getattr(pcl, "__file__", "?"), "numpy": np.__version__}))}
    for k in range(3):
        src, tgt, guess, _ = synth.scan_pair(seed=700 + k, n_src=1500, n_tgt=1400)
        d.update({"src%d" % k: src, "tgt%d" % k: tgt, "guess%d" % k: guess})
    names = []
    for name, reading, reference, p2plane in DPF_CHAINS:
        y = dpf_chain_yaml(shipped, reading, reference, p2plane)
        with tempfile.NamedTemporaryFile("w", suffix=".yaml", delete=False) as fh:
            fh.write(y)
        icp = pcl.ICP()
        icp.loadFromYaml(fh.name)
        os.unlink(fh.name)
        d["yaml_" + name] = np.array(y)
        for k in range(3):
            msg, T = icp.compute(d["src%d" % k], d["tgt%d" % k], d["guess%d" % k])
            d["msg_%s_%d" % (name, k)] = np.array(msg)
            d["T_%s_%d" % (name, k)] = np.asarray(T, np.float32)
        names.append(name)
    d["chains"] = np.array(json.dumps(names))
    np.savez_compressed(os.path.join(GOLDEN, "thirdparty_pcl_dpf.npz"), **d)
    return "wrote thirdparty_pcl_dpf.npz"


def main():
    for line in (pin_cv2(), pin_pcl(), pin_pcl_dpf()):
        print(line)


if __name__ == "__main__":
    main()
