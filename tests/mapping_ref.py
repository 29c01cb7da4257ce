"""Independent numpy restatement of bruce_slam's log-odds occupancy map (mapping.py method 1) and of the OpenCV pieces it
calls (tests only: the oracle of tests/test_mapping_host.py and tests/test_gpu_mapping.py).

What OpenCV is restated as (cv2 is not in this image; tests/golden/make_golden_mapping.py hands these same functions to the
reference's own mapping.py as its ``cv2``, and records that in the fixture's ``stand_ins``):
  * ``getGaussianKernel(n, -1)``: OpenCV's fixed tables for odd n <= 7, otherwise sigma = ((n-1)*0.5 - 1)*0.3 + 0.8, the
    taps exp(-0.5 x^2 / sigma^2) summed in order and scaled by 1/sum, all in double;
  * ``filter2D(src, CV_32F, kernel, ..., 0.0, BORDER_CONSTANT)``: the kernel rounded to float32, then per output pixel a
    direct sum over the kernel's non-zero coefficients in row-major order, starting at delta = 0, one float32 rounding per
    step (no contraction: the images summed here hold 0 and 1, so a fused multiply-add rounds the same);
  * ``resize(src, None, None, f, f, INTER_NEAREST)``: size cvRound(n * f) (half to even), source index
    min(floor(i * (1 / f)), n - 1).
"""
import math
import types

import numpy as np
from scipy.interpolate import interp1d
from scipy.special import expit, logit

# ---- cv2 pieces ------------------------------------------------------------------------------------------------------
CV_32F = 5
BORDER_CONSTANT = 0
INTER_NEAREST = 0
_SMALL_GAUSSIAN = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
                   7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def getGaussianKernel(n, sigma, ktype=None):
    n = int(n)
    fixed = _SMALL_GAUSSIAN.get(n) if (n % 2 == 1 and sigma <= 0) else None
    sig = sigma if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2x = -0.5 / (sig * sig)
    taps, total = [], 0.0
    for i in range(n):
        x = i - (n - 1) * 0.5
        t = float(fixed[i]) if fixed is not None else math.exp(scale2x * x * x)
        taps.append(t)
        total += t
    total = 1.0 / total
    return np.array([t * total for t in taps], np.float64).reshape(n, 1)


def filter2D(src, ddepth, kernel, dst=None, anchor=None, delta=0.0, borderType=BORDER_CONSTANT):
    assert ddepth == CV_32F and borderType == BORDER_CONSTANT and delta == 0.0 and src.dtype == np.float32
    k32 = np.asarray(kernel).astype(np.float32)
    kh, kw = k32.shape
    ay, ax = kh // 2, kw // 2
    rows, cols = src.shape
    pad = np.zeros((rows + kh - 1, cols + kw - 1), np.float32)
    pad[ay:ay + rows, ax:ax + cols] = src
    out = np.zeros((rows, cols), np.float32)
    for i in range(kh):
        for j in range(kw):
            if k32[i, j] != 0:
                out = (out + k32[i, j] * pad[i:i + rows, j:j + cols]).astype(np.float32)
    return out


def resize_nearest(src, f):
    rows, cols = src.shape[:2]
    dw, dh = int(np.rint(cols * f)), int(np.rint(rows * f))
    inv = 1.0 / f
    sx = np.minimum(np.floor(np.arange(dw) * inv).astype(np.int64), cols - 1)
    sy = np.minimum(np.floor(np.arange(dh) * inv).astype(np.int64), rows - 1)
    return src[sy][:, sx]


def resize(src, dsize, dst, fx, fy, interpolation=INTER_NEAREST):
    assert dsize is None and fx == fy and interpolation == INTER_NEAREST
    return resize_nearest(src, fx)


cv2 = types.SimpleNamespace(CV_32F=CV_32F, BORDER_CONSTANT=BORDER_CONSTANT, INTER_NEAREST=INTER_NEAREST,
                            getGaussianKernel=getGaussianKernel, filter2D=filter2D, resize=resize)


# ---- nav_msgs/OccupancyGrid ------------------------------------------------------------------------------------------
class OccupancyGrid(object):
    def __init__(self):
        ns = types.SimpleNamespace
        self.header = ns(frame_id="")
        self.info = ns(origin=ns(position=ns(x=0.0, y=0.0, z=0.0), orientation=ns(x=0.0, y=0.0, z=0.0, w=0.0)),
                       width=0, height=0, resolution=0.0)
        self.data = []


# ---- the OculusProperty subset the map reads (sonar.py: ranges, bearings, b2c, ra2ro) ---------------------------------
class Oculus(object):
    def __init__(self):
        self.num_ranges = self.range_resolution = self.ranges = None
        self.max_range = 30.0
        self.num_bearings = self.bearings = self.angular_resolution = None
        self.b2c = self.ra2ro = None

    def configure(self, ping):
        changed = False
        if ping.num_ranges != self.num_ranges or ping.range_resolution != self.range_resolution:
            self.num_ranges = ping.num_ranges
            self.range_resolution = ping.range_resolution
            self.ranges = self.range_resolution * (1 + np.arange(self.num_ranges))
            self.max_range = self.ranges[-1]
            rr = self.range_resolution
            self.ra2ro = lambda ra: np.round(ra / rr - 1)
            changed = True
        if len(ping.bearings) != self.num_bearings:
            self.num_bearings = len(ping.bearings)
            self.bearings = np.deg2rad(np.array(ping.bearings, np.float32) / 100)
            self.angular_resolution = abs(self.bearings[-1] - self.bearings[0]) / self.num_bearings
            self.b2c = interp1d(self.bearings, np.arange(self.num_bearings), kind="cubic", bounds_error=False,
                                fill_value=-1, assume_sorted=True)
            changed = True
        return changed


# ---- the map ---------------------------------------------------------------------------------------------------------
class Submap(object):
    def __init__(self):
        self.k = 0
        self.pose = None
        self.sonar_xy = None
        self.logodds = None
        self.r = self.c = self.l = None


def measurement(mask_shape, hits_rc, hr, hc, hit_prob, miss_prob, stages=None):
    """polar hit cells -> float32 log-odds image (mapping.py:170-228).  `stages` (a dict) receives the intermediates."""
    mask = np.zeros(mask_shape, np.float32)
    if hits_rc is None:
        mask += miss_prob
    else:
        mask[hits_rc[0], hits_rc[1]] = 1.0
        if stages is not None:
            stages["hits"] = mask.copy()
        kernel_r = getGaussianKernel(2 * hr + 1, -1)
        kernel_c = getGaussianKernel(2 * hc + 1, -1)
        kernel = kernel_r.dot(kernel_c.T)
        mask = filter2D(mask, CV_32F, kernel, None, None, 0.0, BORDER_CONSTANT)
        if stages is not None:
            stages["filtered"] = mask.copy()
        mask /= kernel[hr, hc] / hit_prob
        mask = np.clip(mask, 0.5, hit_prob)
        first_hits = np.argmax(mask > 0.5, axis=0)
        first_hits[first_hits == 0] = mask.shape[0]
        for j in range(mask.shape[1]):
            mask[: first_hits[j], j] = miss_prob
        if stages is not None:
            stages["first_hits"] = first_hits.copy()
    if stages is not None:
        stages["prob"] = mask.copy()
    return logit(mask).ravel().astype(np.float32)


class Mapping(object):
    def __init__(self):
        self.x0 = -50.0
        self.y0 = -50.0
        self.width = 100.0
        self.height = 100.0
        self.inc = 50.0
        self.resolution = 0.2
        self.rows = None
        self.cols = None
        self.oculus = Oculus()
        self.oculus_image_size = None
        self.oculus_r_skip = None
        self.oculus_c_skip = None
        self.pub_occupancy1 = True
        self.hit_prob = 0.8
        self.miss_prob = 0.3
        self.logodds_grid = None
        self.inflation_angle = 0.05
        self.inflation_range = 0.5
        self.outlier_filter_radius = 5.0
        self.outlier_filter_min_points = 20
        self.min_translation = 0.5
        self.min_rotation = 0.05
        self.rmin = self.rmax = self.cmin = self.cmax = None
        self.keyframes = []
        # what remove_outlier is (the C oracle's in the tests)
        self.remove_outlier = None

    def configure(self):
        xs = np.arange(0, self.width, self.resolution)
        ys = np.arange(0, self.height, self.resolution)
        self.rows, self.cols = len(ys), len(xs)
        self.logodds_grid = np.zeros((ys.shape[0], xs.shape[0]), np.float32)
        self.rmax = self.cmax = 0
        self.rmin = ys.shape[0] - 1
        self.cmin = xs.shape[0] - 1
        self.inc_r = int(self.inc / self.resolution)
        self.inc_c = int(self.inc / self.resolution)

    def pose_changed(self, pose, new_pose):
        dp = pose.between(new_pose)
        dt = np.linalg.norm(np.array([dp.x(), dp.y()]))
        dr = abs(dp.theta())
        return dt > self.min_translation or dr > self.min_rotation

    def geometry(self, ping, keyframe):
        """oculus.configure + the skips and sonar_xy when the geometry changed (mapping.py:143-164)"""
        if self.oculus.configure(ping):
            self.oculus_r_skip = max(1, np.int32(np.floor(self.resolution / self.oculus.range_resolution)))
            range_resolution = self.oculus.angular_resolution * self.oculus.max_range
            self.oculus_c_skip = max(1, np.int32(np.floor(self.resolution / range_resolution)))
            B, R = np.meshgrid(self.oculus.bearings[:: self.oculus_c_skip], self.oculus.ranges[:: self.oculus_r_skip])
            X, Y = np.cos(B) * R, np.sin(B) * R
            keyframe.sonar_xy = np.c_[X.ravel(), Y.ravel()].astype(np.float32)
            self.oculus_image_size = X.shape

    def hits(self, points):
        """points -> (rows, cols) of the hit cells of the downsampled polar image and (hr, hc); None for no hit"""
        if not len(points):
            return None, 0, 0
        if self.outlier_filter_min_points > 1:
            points = self.remove_outlier(points[:, :2], self.outlier_filter_radius, self.outlier_filter_min_points)
        o = self.oculus
        c = o.b2c(np.arctan2(points[:, 1], points[:, 0]))
        c = np.clip(np.int32(np.round(c)), 0, o.num_bearings - 1)
        r = o.ra2ro(np.linalg.norm(points[:, :2], axis=1))
        r = np.clip(np.int32(np.round(r)), 0, o.num_ranges - 1)
        hc = int(round(self.inflation_angle / o.angular_resolution / self.oculus_c_skip))
        hr = int(round(self.inflation_range / o.range_resolution / self.oculus_r_skip))
        return (r // self.oculus_r_skip, c // self.oculus_c_skip), hr, hc

    def add_keyframe(self, key, pose, ping, points, stages=None):
        keyframe = Submap()
        keyframe.k = len(self.keyframes)
        keyframe.pose = pose
        self.geometry(ping, keyframe)
        rc, hr, hc = self.hits(points)
        keyframe.logodds = measurement(self.oculus_image_size, rc, hr, hc, self.hit_prob, self.miss_prob, stages)
        self._append(key, keyframe)

    def add_keyframe_logodds(self, key, pose, ping, logodds):
        keyframe = Submap()
        keyframe.k = len(self.keyframes)
        keyframe.pose = pose
        self.geometry(ping, keyframe)
        keyframe.logodds = np.ascontiguousarray(logodds, np.float32).ravel()
        self._append(key, keyframe)

    def _append(self, key, keyframe):
        self.fit_grid(keyframe)
        self.inc_grid(keyframe)
        while len(self.keyframes) < key:
            self.keyframes.append(None)
        self.keyframes.append(keyframe)

    def update_pose(self, key, new_pose):
        assert key < len(self.keyframes)
        keyframe = self.keyframes[key]
        if not keyframe:
            return
        if not self.pose_changed(keyframe.pose, new_pose):
            return
        keyframe.pose = new_pose
        self.dec_grid(keyframe)
        self.fit_grid(keyframe)
        self.inc_grid(keyframe)

    def get_occupancy_grid1(self, frames=None, resolution=None):
        occ_msg = OccupancyGrid()
        occ_msg.header.frame_id = "map"
        if frames is None:
            grid = self.logodds_grid
            rmin, rmax, cmin, cmax = self.rmin, self.rmax, self.cmin, self.cmax
        else:
            grid = np.zeros_like(self.logodds_grid)
            rmin, rmax, cmin, cmax = self.rmax, self.rmin, self.cmax, self.cmin
            for k in frames:
                if k >= len(self.keyframes) or self.keyframes[k] is None:
                    continue
                kf = self.keyframes[k]
                grid[kf.r, kf.c] += kf.l
                rmin, rmax = min(rmin, kf.r.min()), max(rmax, kf.r.max())
                cmin, cmax = min(cmin, kf.c.min()), max(cmax, kf.c.max())
        self.last_frames_grid = grid
        probs = expit(grid[rmin: rmax + 1, cmin: cmax + 1])
        if resolution is not None and resolution > 0 and abs(resolution - self.resolution) > self.resolution * 1e-1:
            assert resolution >= self.resolution
            ratio = self.resolution / resolution
            probs = resize_nearest(probs, ratio)
            resolution = self.resolution / ratio
        else:
            resolution = self.resolution
        occ = np.int8(np.clip(100 * probs, 0, 100))
        occ_msg.info.origin.position.x = self.x0 + cmin * resolution
        occ_msg.info.origin.position.y = self.y0 + rmin * resolution
        occ_msg.info.origin.orientation.w = 1
        occ_msg.info.width = occ.shape[1]
        occ_msg.info.height = occ.shape[0]
        occ_msg.info.resolution = resolution
        occ_msg.data = list(occ.ravel())
        occ_msg.occ = occ
        occ_msg.probs = probs
        return occ_msg

    def inc_grid(self, kf):
        self.logodds_grid[kf.r, kf.c] += kf.l
        if len(kf.r):
            self.rmin, self.rmax = min(self.rmin, kf.r.min()), max(self.rmax, kf.r.max())
        if len(kf.c):
            self.cmin, self.cmax = min(self.cmin, kf.c.min()), max(self.cmax, kf.c.max())

    def dec_grid(self, kf):
        self.logodds_grid[kf.r, kf.c] -= kf.l

    def sonar_xy_of(self, kf):
        if kf.sonar_xy is not None:
            return kf.sonar_xy
        k = kf.k - 1
        while k >= 0:
            if self.keyframes[k] and self.keyframes[k].sonar_xy is not None:
                return self.keyframes[k].sonar_xy
            k -= 1
        raise AssertionError("no geometry")

    def fit_grid(self, kf):
        yaw = kf.pose.theta()
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, -s], [s, c]])
        t = np.array([kf.pose.x(), kf.pose.y()])
        xy = R.dot(self.sonar_xy_of(kf).T).T + t
        r = np.int32(np.round((xy[:, 1] - self.y0) / self.resolution))
        c = np.int32(np.round((xy[:, 0] - self.x0) / self.resolution))
        r, c = self.adjust_bounds(r, c)
        _, sel = np.unique(r * self.cols + c, return_index=True)
        kf.r = np.uint16(r[sel])
        kf.c = np.uint16(c[sel])
        kf.l = kf.logodds[sel]

    def _shift(self, attr, inc):
        # the reference shifts every entry of self.keyframes and stops at a missed key (None); here None is skipped
        for kf in self.keyframes:
            if kf is not None:
                setattr(kf, attr, getattr(kf, attr) + np.uint16(inc))

    def adjust_bounds(self, r, c):
        g = self.logodds_grid
        while not np.all(r >= 0):
            r += self.inc_r
            self.rmin += self.inc_r
            self.rmax += self.inc_r
            self.rows += self.inc_r
            self.y0 -= self.inc_r * self.resolution
            self.height += self.inc_r * self.resolution
            g = self.logodds_grid = np.r_[np.zeros((self.inc_r, self.cols), g.dtype), g]
            self._shift("r", self.inc_r)
        while not np.all(r < self.rows):
            self.rows += self.inc_r
            self.height += self.inc_r * self.resolution
            g = self.logodds_grid = np.r_[g, np.zeros((self.inc_r, self.cols), g.dtype)]
        while not np.all(c >= 0):
            c += self.inc_c
            self.cmin += self.inc_c
            self.cmax += self.inc_c
            self.cols += self.inc_c
            self.x0 -= self.inc_c * self.resolution
            self.width += self.inc_c * self.resolution
            g = self.logodds_grid = np.c_[np.zeros((self.rows, self.inc_c), g.dtype), g]
            self._shift("c", self.inc_c)
        while not np.all(c < self.cols):
            self.cols += self.inc_c
            self.width += self.inc_c * self.resolution
            g = self.logodds_grid = np.c_[g, np.zeros((self.rows, self.inc_c), g.dtype)]
        return r, c


# ---- the recorded session of tests/golden/mapping_session.npz, replayed on any Mapping-like object ------------------
class SessionPing(object):
    """the ping fields the map reads: num_ranges, range_resolution, bearings (1/100 degree)"""

    def __init__(self, n_beams, n_ranges, range_resolution):
        self.num_ranges, self.range_resolution = n_ranges, range_resolution
        self.bearings = list(np.round(np.linspace(-6500.0, 6500.0, n_beams)).astype(np.int16))


def replay(m, fix, pose2, from_logodds=False, batched=False, check=None):
    """drive `m` (configured by the caller from fix["settings"]) through the fixture's session; after every recorded step
    call check(step_index, step_record).  `batched`: each pose pass as one update_poses call (the steps inside it are
    then checked only at its end)."""
    import json
    geoms = json.loads(str(fix["geoms"]))
    steps = json.loads(str(fix["steps"]))
    i = 0
    while i < len(steps):
        st = steps[i]
        if st["op"] == "add":
            ping = SessionPing(*geoms[st["geom"]])
            pose = pose2(*st["pose"])
            if from_logodds:
                m.add_keyframe_logodds(st["key"], pose, ping, fix["logodds_%d" % st["key"]])
            else:
                m.add_keyframe(st["key"], pose, ping, fix["points_%d" % st["key"]].astype(np.float64))
            check and check(i, st)
            i += 1
        elif batched:
            j = i
            while j < len(steps) and steps[j]["op"] == "update" and steps[j]["pass_"] == st["pass_"]:
                j += 1
            m.update_poses([s["key"] for s in steps[i:j]], [pose2(*s["pose"]) for s in steps[i:j]])
            check and check(j - 1, steps[j - 1])
            i = j
        else:
            m.update_pose(st["key"], pose2(*st["pose"]))
            check and check(i, st)
            i += 1
