#!/usr/bin/env python
"""Generate tests/golden/mapping2_session.npz FROM THE REFERENCE's own point-projection map (mapping.py:357-439,
get_occupancy_grid2).

Run where the reference tree is (make_golden_mapping.py says where it is looked for; a machine without it cannot run this):

    python tests/golden/make_golden_mapping2.py

The reference's ``mapping.py`` is exec'd as in make_golden_mapping.py (same stand-ins, same patched line, same session) and
its ``cv2`` additionally gets ``getStructuringElement`` / ``dilate`` from tests/golden/thirdparty.py (the oracle's ellipse
element and cost_grid where OpenCV is not installed).  ``pcl.remove_outlier`` stays the oracle's, wrapped to note what it was
handed and how many points it kept.  Every stand-in is recorded in ``stand_ins``.

Two stages: after the adds (which grow the map on all four sides, so the earlier cell lists are shifted) and after the
loop-closure pass (which moves every keyframe, rewrites every cell list and grows the map once more).
The cell lists at both stages are those of mapping_session.npz (checked here), so they are not stored again.  Before the
publications of a stage ``point_cloud`` is the keyed global cloud registered with the current poses (float32 x, y, 0, key),
extended with a few points far outside the known region and a few exactly on (k + 0.5) * resolution from the region's
corner; ``cloud64`` is the same cloud taken in float64, ties exact, for the publication without the filter.

Per publication: data, the five info numbers, the known region's box, the points selected and the number the filter kept.
Nothing of the reference is copied into the repository: only the numbers it produces.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_mapping as gm  # noqa: E402  (puts tests/ and the repository root on the path)
import mapping_ref  # noqa: E402
import oracle  # noqa: E402
import thirdparty  # noqa: E402
from make_golden import Pose2  # noqa: E402

OUT = os.path.join(HERE, "mapping2_session.npz")

# name -> (get_occupancy_grid2's arguments, which cloud, settings changed for this publication)
PUBS = {
    "all": (dict(), "cloud32", dict()),
    "frames": (dict(frames=[19, 3, 0, 99, 7, 12, 7]), "cloud32", dict()),          # duplicate, missed key, key out of range
    "coarse": (dict(resolution=0.5), "cloud32", dict()),
    "frames_coarse": (dict(frames=[2, 9, 16], resolution=0.45), "cloud32", dict()),
    "near": (dict(resolution=0.21), "cloud32", dict()),                             # no resize
    "nofilter64": (dict(), "cloud64", dict(outlier_filter_min_points=1)),
    "frames_nofilter64": (dict(frames=[7, 1, 7]), "cloud64", dict(outlier_filter_min_points=1)),
    "dilate1": (dict(), "cloud32", dict(dilate_size=1)),
    "dilate11": (dict(frames=[0, 4, 10, 15]), "cloud32", dict(dilate_size=11)),
    "empty": (dict(), "empty", dict()),
    "no_points": (dict(frames=[5, 99]), "cloud32", dict()),                         # keyframe 5 exists and has no points
}


def global_cloud(sess, poses, m, boxes):
    """-> (float32 [n x 4], float64 [n x 4]): x, y, 0, key"""
    parts = []
    for key, _, _, pts in sess:
        x, y, th = poses[key]
        c, s = np.cos(th), np.sin(th)
        g = np.c_[c * pts[:, 0] - s * pts[:, 1] + x, s * pts[:, 0] + c * pts[:, 1] + y]
        parts.append(np.c_[g, np.zeros(len(g)), np.full(len(g), float(key))])
    cloud = np.concatenate(parts).astype(np.float32).astype(np.float64)
    rmin, rmax = min(b[0] for b in boxes), max(b[1] for b in boxes)
    cmin, cmax = min(b[2] for b in boxes), max(b[3] for b in boxes)
    res = m.resolution
    x0, y0 = m.x0 + cmin * res, m.y0 + rmin * res
    w, h = (cmax - cmin + 1) * res, (rmax - rmin + 1) * res
    far = [(x0 - 40.0, y0 + 3.0, 0.0, 0.0), (x0 + w + 25.0, y0 + h + 25.0, 0.0, 7.0), (x0 + 1.0, y0 - 31.0, 0.0, 12.0),
           (x0 + w + 0.3, y0 + 2.0, 0.0, 19.0), (x0 + 2.0, y0 + h + 0.31, 0.0, 0.0), (1e9, -1e9, 0.0, 7.0)]
    # exactly half a cell from the corner (in float64): ties of the rounding, next to live points so the filter keeps them
    ties = []
    for i in (0, 200, 700, 1500, 2100):
        px, py = cloud[i % len(cloud), :2]
        kx, ky = np.floor((px - x0) / res), np.floor((py - y0) / res)
        ties += [(x0 + (kx + 0.5) * res, py, 0.0, cloud[i % len(cloud), 3]), (px, y0 + (ky + 0.5) * res, 0.0, 7.0),
                 (x0 + (kx + 1.5) * res, y0 + (ky + 1.5) * res, 0.0, 1.0)]
    cloud64 = np.concatenate([cloud, np.array(far), np.array(ties)])
    return cloud64.astype(np.float32), cloud64


def main():
    Mapping, stand_ins = gm.reference_mapping()
    g = Mapping.get_occupancy_grid2.__globals__
    tp = thirdparty.cv2(oracle)
    g["cv2"] = types.SimpleNamespace(**dict(vars(mapping_ref.cv2), MORPH_ELLIPSE=tp.MORPH_ELLIPSE,
                                            getStructuringElement=tp.getStructuringElement, dilate=tp.dilate))
    seen = {}

    def remove_outlier(pts, r, k):
        out = oracle.remove_outlier(np.asarray(pts, np.float32), r, k)
        seen["points"], seen["kept"] = np.array(pts), len(out)
        return out
    g["pcl"] = types.SimpleNamespace(remove_outlier=remove_outlier)
    stand_ins = stand_ins + json.loads(str(thirdparty.record())) + [
        "pcl.remove_outlier -> oracle.remove_outlier behind a wrapper that records its input and the kept count"]

    m = Mapping()
    for k, v in gm.SETTINGS.items():
        setattr(m, k, v)
    m.configure()
    first = np.load(os.path.join(HERE, "mapping_session.npz"))
    out = {"settings": np.array(json.dumps(gm.SETTINGS)), "pubs": np.array(json.dumps(PUBS)),
           "dilate_size": np.array(m.dilate_size)}
    sess = gm.session()
    poses = {}
    stages = {}

    def publish(stage):
        live = [kf for kf in m.keyframes if kf is not None]
        boxes = [(int(kf.r.min()), int(kf.r.max()), int(kf.c.min()), int(kf.c.max())) for kf in live]
        for i, kf in enumerate(m.keyframes):         # the cell lists are mapping_session.npz's
            if kf is not None:
                assert np.array_equal(kf.r, first["r_%s_%d" % (stage, i)]) and np.array_equal(kf.c, first["c_%s_%d" % (stage, i)])
        cloud32, cloud64 = global_cloud(sess, poses, m, boxes)
        clouds = {"cloud32": cloud32, "cloud64": cloud64, "empty": np.zeros((0, 4), np.float32)}
        out["cloud32_%s" % stage], out["cloud64_%s" % stage] = cloud32, cloud64
        stages[stage] = dict(x0=float(m.x0), y0=float(m.y0), box=[int(m.rmin), int(m.rmax), int(m.cmin), int(m.cmax)],
                             rows=int(m.rows), cols=int(m.cols), n_keyframes=len(m.keyframes),
                             kf_boxes=[None if kf is None else [int(kf.r.min()), int(kf.r.max()), int(kf.c.min()),
                                                                int(kf.c.max())] for kf in m.keyframes])
        keep = {k: getattr(m, k) for k in ("outlier_filter_min_points", "dilate_size")}
        for name, (kw, which, over) in PUBS.items():
            for k, v in dict(keep, **over).items():
                setattr(m, k, v)
            m.point_cloud = clouds[which]
            seen.clear()
            msg = m.get_occupancy_grid2(**kw)
            tag = "%s_%s" % (stage, name)
            data = np.array(msg.data, np.int8)
            info = np.array([msg.info.origin.position.x, msg.info.origin.position.y, msg.info.width, msg.info.height,
                             msg.info.resolution], np.float64)
            # the known region, from the reference's own cell lists
            frames = kw.get("frames")
            ks = [k for k in (range(len(m.keyframes)) if frames is None else frames)
                  if k < len(m.keyframes) and m.keyframes[k] is not None]
            box = [min(int(m.keyframes[k].r.min()) for k in ks), max(int(m.keyframes[k].r.max()) for k in ks),
                   min(int(m.keyframes[k].c.min()) for k in ks), max(int(m.keyframes[k].c.max()) for k in ks)]
            assert info[0] == m.x0 + box[2] * m.resolution and info[1] == m.y0 + box[0] * m.resolution
            if "points" in seen:
                points, kept = seen["points"], seen["kept"]
            else:       # the filter did not run: the selection as mapping.py:365-372 writes it
                pc = m.point_cloud
                points = pc[:, :2] if frames is None else np.concatenate(
                    [np.zeros((0, 2))] + [pc[np.uint32(pc[:, 3]) == k, :2] for k in frames])
                kept = len(points)
            out["pub_%s_data" % tag], out["pub_%s_info" % tag] = data, info
            out["pub_%s_box" % tag] = np.array(box, np.int32)
            out["pub_%s_points" % tag] = np.asarray(points)
            out["pub_%s_kept" % tag] = np.array(kept)
            print("%-24s %4d x %-4d  %5d points, %5d kept, %5d occupied, %5d free" % (
                tag, info[3], info[2], len(points), kept, int((data == 100).sum()), int((data == 0).sum())))
        for k, v in keep.items():
            setattr(m, k, v)
        try:
            m.get_occupancy_grid2(frames=[3, 99])
            raise AssertionError("frames=[3, 99] did not raise")
        except IndexError:
            pass

    for key, geom, pose, pts in sess:
        m.add_keyframe(key, Pose2(*pose), gm.Ping(geom), pts)
        poses[key] = pose
    publish("adds")
    for key in [k for k, _, _, _ in sess]:
        new = gm.loop_closure(poses[key], key)
        m.update_pose(key, Pose2(*new))
        if m.pose_changed(Pose2(*poses[key]), Pose2(*new)):
            poses[key] = new
    publish("lc")
    out["stages"] = np.array(json.dumps(stages))
    out["stand_ins"] = np.array(json.dumps(stand_ins))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
