#!/usr/bin/env python
"""Generate tests/golden/mapping_session.npz FROM THE REFERENCE's own occupancy map code.

Run in the build container (needs /root/reference; the GPU box does not have it):

    python tests/golden/make_golden_mapping.py

``bruce_slam/src/bruce_slam/mapping.py`` is exec'd with its imports replaced by stand-ins for what this image lacks, and
``OculusProperty`` / ``OculusFireMsg`` are cut out of ``sonar.py`` by AST:
  * cv2 -> tests/mapping_ref.py's getGaussianKernel / filter2D (direct sum) / resize (INTER_NEAREST);
  * pcl.remove_outlier -> the C oracle's remove_outlier;
  * gtsam.Pose2 -> the Pose2 of make_golden.py (gtsam's published Pose2 algebra);
  * nav_msgs.msg.OccupancyGrid -> tests/mapping_ref.py's attribute-path stand-in.
One line of the reference is patched, and the patch is recorded in ``stand_ins``: ``adjust_bounds`` shifts every entry of
``self.keyframes`` and raises on the None a missed key leaves there (mapping.py:523,563); the patched loop skips it, as the
product does.

The session (two sonar geometries, the second with c_skip = 2; a missed key; a keyframe without points; one with its first
hit in polar row 0; a loop closure that moves every keyframe; growth on all four sides from a small initial map; the three
published forms) records per step the box, origin, size and the sha256 of the float32 grid and of every keyframe's r/c/l,
and in full: each keyframe's log-odds image, r/c/l after its add and after each pose pass, and the grid at those points.

Nothing of the reference is copied into the repository: only the numbers it produces.
"""
import ast
import hashlib
import json
import os
import sys
import textwrap
import types

import numpy as np
from scipy.interpolate import interp1d
from scipy.special import expit, logit

REF = "/root/reference/bruce_slam/src/bruce_slam"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import mapping_ref  # noqa: E402
from make_golden import Pose2  # noqa: E402

OUT = os.path.join(HERE, "mapping_session.npz")

# map settings of the session: a 20 m map grown by 6 m steps
SETTINGS = dict(x0=-10.0, y0=-10.0, width=20.0, height=20.0, inc=6.0, resolution=0.2, outlier_filter_radius=2.0,
                outlier_filter_min_points=8, min_translation=0.5, min_rotation=0.05)
# (n_beams, n_ranges, range_resolution): A has r_skip 5, c_skip 1; B has r_skip 2, c_skip 2
GEOMS = {"A": (128, 256, 0.04), "B": (256, 128, 0.08)}


def bearings_centideg(n):
    return np.round(np.linspace(-6500.0, 6500.0, n)).astype(np.int16)


class Ping(object):
    __slots__ = ("num_ranges", "range_resolution", "bearings", "fire_msg", "part_number")

    def __init__(self, geom):
        nb, nr, rr = GEOMS[geom]
        self.num_ranges, self.range_resolution, self.bearings = nr, rr, list(bearings_centideg(nb))
        self.fire_msg = types.SimpleNamespace(mode=1, gamma=255, flags=0, range=nr * rr, gain=50.0, speed_of_sound=1500.0,
                                              salinity=0.0)
        self.part_number = 1032


def reference_mapping():
    src = open(os.path.join(REF, "sonar.py")).read()
    tree = ast.parse(src)
    cls = {n.name: textwrap.dedent(ast.get_source_segment(src, n)) for n in ast.walk(tree)
           if isinstance(n, ast.ClassDef) and n.name in ("OculusFireMsg", "OculusProperty")}
    ns_s = {"np": np, "interp1d": interp1d, "cv2": mapping_ref.cv2, "r2n": None}
    for name in ("OculusFireMsg", "OculusProperty"):
        exec(compile(cls[name], "reference:sonar.py", "exec"), ns_s)

    import oracle
    src = open(os.path.join(REF, "mapping.py")).read()
    keep = [ln for ln in src.splitlines() if not ln.startswith(("import cv2", "from scipy", "from nav_msgs", "from ."))]
    body = "\n".join(keep)
    loop = "for keyframe in self.keyframes:"
    assert body.count(loop) == 2
    body = body.replace(loop, "for keyframe in [kf for kf in self.keyframes if kf is not None]:")
    pcl = types.SimpleNamespace(remove_outlier=lambda pts, r, k: oracle.remove_outlier(np.asarray(pts, np.float32), r, k))
    ns = {"np": np, "cv2": mapping_ref.cv2, "logit": logit, "expit": expit, "OccupancyGrid": mapping_ref.OccupancyGrid,
          "OculusProperty": ns_s["OculusProperty"], "OculusFireMsg": ns_s["OculusFireMsg"], "pcl": pcl, "r2n": None}
    exec(compile(body, "reference:mapping.py", "exec"), ns)
    stand_ins = ["cv2.getGaussianKernel / filter2D / resize -> tests/mapping_ref.py (fixed tables / sigma formula in "
                 "double; direct-sum filter2D; INTER_NEAREST with cvRound size)",
                 "pcl.remove_outlier -> oracle.remove_outlier", "gtsam.Pose2 -> make_golden.Pose2",
                 "nav_msgs.msg.OccupancyGrid -> mapping_ref.OccupancyGrid",
                 "mapping.py adjust_bounds: None entries of self.keyframes skipped when shifting r / c"]
    return ns["Mapping"], stand_ins


def wall_points(rng, bearing_lo, bearing_hi, rho_lo, rho_hi, n):
    b = rng.uniform(bearing_lo, bearing_hi, n)
    rho = rng.uniform(rho_lo, rho_hi, n)
    # the SLAM node's keyframe frame: a return at bearing b, range rho lies at (rho cos b, rho sin b)
    return np.c_[rho * np.cos(b), rho * np.sin(b)].astype(np.float32).astype(np.float64)


def session():
    """[(key, geom, (x, y, theta), points)] -- key 3 is missed"""
    rng = np.random.default_rng(7)
    plan = [  # heading east, north, west, south: the fans leave the 20 m map on every side
        (0, "A", (0.0, 0.0, 0.0)), (1, "A", (2.0, 0.5, 0.1)), (2, "A", (4.0, 1.0, 0.3)),
        (4, "A", (5.0, 3.0, 1.5)), (5, "A", (4.5, 6.0, 1.6)), (6, "B", (3.0, 8.0, 2.2)),
        (7, "B", (0.0, 8.5, 3.0)), (8, "B", (-3.0, 8.0, -2.9)), (9, "B", (-6.0, 6.0, -2.4)),
        (10, "A", (-8.0, 3.0, -1.8)), (11, "A", (-8.5, 0.0, -1.6)), (12, "A", (-8.0, -3.0, -1.2)),
        (13, "A", (-5.0, -6.0, -0.6)), (14, "A", (-2.0, -7.0, -0.2)), (15, "A", (1.0, -6.5, 0.2)),
        (16, "A", (4.0, -5.0, 0.8)), (17, "A", (6.0, -2.0, 1.2)), (18, "A", (6.5, 1.0, 1.4)),
        (19, "A", (5.5, 2.0, 2.0)),
    ]
    out = []
    for key, geom, pose in plan:
        if key == 5:
            pts = np.zeros((0, 2))                                          # no points: the whole fan is a miss
        elif key == 7:
            pts = np.r_[wall_points(rng, -0.6, 0.6, 0.02, 0.06, 40),       # first hit in polar row 0
                        wall_points(rng, -0.3, 0.4, 6.0, 7.5, 60)]
        else:
            pts = np.r_[wall_points(rng, -0.9, -0.2, 5.0, 6.0, 50), wall_points(rng, 0.1, 0.8, 7.0, 9.5, 70),
                        wall_points(rng, -1.1, 1.1, 9.8, 10.0, 6)]          # a few strays for the outlier filter
        out.append((key, geom, pose, pts))
    return out


def loop_closure(pose, key):
    """every keyframe moves; keys 6-9 far enough to grow the map in the middle of the pass"""
    x, y, th = pose
    return (x + 0.3, y + (0.9 * key if 6 <= key <= 9 else -0.2), th + 0.06)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    Mapping, stand_ins = reference_mapping()
    m = Mapping()
    defaults = {k: v for k, v in vars(m).items() if isinstance(v, (bool, int, float, str, type(None)))}
    for k, v in SETTINGS.items():
        setattr(m, k, v)
    m.configure()
    out = {"defaults": np.array(json.dumps(defaults)), "settings": np.array(json.dumps(SETTINGS)),
           "geoms": np.array(json.dumps(GEOMS))}
    steps = []

    def kf_digest():
        return sha(*[a for kf in m.keyframes if kf is not None for a in (kf.r, kf.c, kf.l)])

    def record(op, **extra):
        steps.append(dict(op=op, box=[int(m.rmin), int(m.rmax), int(m.cmin), int(m.cmax)], x0=float(m.x0), y0=float(m.y0),
                          rows=int(m.rows), cols=int(m.cols), width=float(m.width), height=float(m.height),
                          grid=sha(m.logodds_grid), keyframes=kf_digest(), **extra))

    def dump_all(tag):
        out["grid_%s" % tag] = m.logodds_grid.copy()
        for i, kf in enumerate(m.keyframes):
            if kf is not None:
                out["r_%s_%d" % (tag, i)], out["c_%s_%d" % (tag, i)], out["l_%s_%d" % (tag, i)] = \
                    kf.r.copy(), kf.c.copy(), kf.l.copy()   # (growth shifts r / c in place later)

    sess = session()
    poses = {}
    for key, geom, pose, pts in sess:
        m.add_keyframe(key, Pose2(*pose), Ping(geom), pts)
        kf = m.keyframes[key]
        out["points_%d" % key] = pts.astype(np.float32)
        out["logodds_%d" % key] = kf.logodds
        out["r_add_%d" % key], out["c_add_%d" % key], out["l_add_%d" % key] = kf.r.copy(), kf.c.copy(), kf.l.copy()
        poses[key] = pose
        record("add", key=key, geom=geom, pose=list(pose), skips=[int(m.oculus_r_skip), int(m.oculus_c_skip)],
               image=list(m.oculus_image_size))
    dump_all("adds")
    for p, keys in (("lc", [k for k, _, _, _ in sess]), ("nudge", [0, 1, 2, 4, 6, 8, 10, 12])):
        for key in keys:
            if p == "lc":
                new = loop_closure(poses[key], key)
            else:   # alternately below and above the thresholds: pose_changed gates half of these
                x, y, th = poses[key]
                new = (x + (0.2 if key % 4 == 0 else 0.9), y, th)
            m.update_pose(key, Pose2(*new))
            if m.pose_changed(Pose2(*poses[key]), Pose2(*new)):
                poses[key] = new
            record("update", key=key, pass_=p, pose=list(new))
        dump_all(p)
    m.update_pose(3, Pose2(1.0, 1.0, 0.0))      # the missed key: nothing happens
    record("update", key=3, pass_="missed", pose=[1.0, 1.0, 0.0])

    pubs = {"all": dict(), "frames": dict(frames=[19, 3, 0, 99, 7, 12, 7]), "coarse": dict(resolution=0.5),
            "frames_coarse": dict(frames=[2, 9, 16], resolution=0.45), "near": dict(resolution=0.21)}
    for name, kw in pubs.items():
        msg = m.get_occupancy_grid(**kw)
        out["pub_%s_data" % name] = np.array(msg.data, np.int8)
        out["pub_%s_info" % name] = np.array([msg.info.origin.position.x, msg.info.origin.position.y, msg.info.width,
                                              msg.info.height, msg.info.resolution], np.float64)
    out["pubs"] = np.array(json.dumps(pubs))
    out["steps"] = np.array(json.dumps(steps))
    out["stand_ins"] = np.array(json.dumps(stand_ins))
    np.savez_compressed(OUT, **out)
    grows = [(s["op"], s.get("key"), s["rows"], s["cols"], s["y0"], s["x0"]) for s in steps]
    prev = None
    for g in grows:
        if prev and g[2:] != prev[2:]:
            print("growth at", g)
        prev = g
    print("wrote %s (%d bytes, %d steps)" % (OUT, os.path.getsize(OUT), len(steps)))


if __name__ == "__main__":
    main()
