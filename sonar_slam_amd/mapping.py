"""bruce_slam's log-odds occupancy map (bruce_slam/mapping.py, method 1) with the per-pixel work on the device.

``Mapping`` keeps the reference's attributes, defaults and control flow; the polar measurement image, the fit of every
pixel of a keyframe to grid cells with its deduplication, the ordered add / subtract of the cells on the float32 grid, growth
and rendering run in HIP kernels (csrc/sfe_map.hip, one ``sfe_map`` per Mapping).  What stays here is small or carries
rounding the device cannot reproduce bit for bit: the OculusProperty subset (ranges, bearings, the cubic b2c, ra2ro), the
skips, sonar_xy (once per geometry), the outlier filter (pcl.remove_outlier), the hit indices, the Gaussian kernel, the
per-keyframe cos / sin of the pose, pose_changed and the growth decisions of adjust_bounds.

Extensions: ``update_poses(keys, poses)`` (the loop of update_pose calls, batched: the same bits) and
``add_keyframe_logodds(key, pose, ping, logodds)`` (a ready polar log-odds image instead of points).  Refused:
method 2 (``get_occupancy_grid2``) and the intensity grid.  INTEGRATION.md lists the deviations.
"""
import ctypes as C
import math
import types

import numpy as np
from scipy.interpolate import interp1d
from scipy.special import logit

from . import _lib as _L
from . import pcl

_SMALL_GAUSSIAN = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
                   7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def gaussian_kernel(n):
    """cv2.getGaussianKernel(n, -1) (float64 column): OpenCV's fixed taps for odd n <= 7, otherwise
    sigma = ((n - 1) * 0.5 - 1) * 0.3 + 0.8 and the taps normalised by their sum, in double"""
    fixed = _SMALL_GAUSSIAN.get(n) if n % 2 == 1 else None
    sigma = ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2x = -0.5 / (sigma * sigma)
    taps, total = [], 0.0
    for i in range(n):
        x = i - (n - 1) * 0.5
        t = float(fixed[i]) if fixed is not None else math.exp(scale2x * x * x)
        taps.append(t)
        total += t
    total = 1.0 / total
    return np.array([t * total for t in taps], np.float64).reshape(n, 1)


class OccupancyGrid(object):
    """nav_msgs/OccupancyGrid's attribute paths that mapping.py writes, plus ``occ`` (the int8 image)"""

    def __init__(self):
        ns = types.SimpleNamespace
        self.header = ns(frame_id="")
        self.info = ns(origin=ns(position=ns(x=0.0, y=0.0, z=0.0), orientation=ns(x=0.0, y=0.0, z=0.0, w=0.0)),
                       width=0, height=0, resolution=0.0)
        self.data = []
        self.occ = None


class _Oculus(object):
    """the part of OculusProperty (sonar.py:140-245) the map reads"""

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
            res = self.range_resolution
            self.ra2ro = lambda ra: np.round(ra / res - 1)
            changed = True
        if len(ping.bearings) != self.num_bearings:   # the count decides, as in the reference
            self.num_bearings = len(ping.bearings)
            self.bearings = np.deg2rad(np.array(ping.bearings, np.float32) / 100)
            self.angular_resolution = abs(self.bearings[-1] - self.bearings[0]) / self.num_bearings
            self.b2c = interp1d(self.bearings, np.arange(self.num_bearings), kind="cubic", bounds_error=False,
                                fill_value=-1, assume_sorted=True)
            changed = True
        return changed


class Submap(object):
    """one keyframe: ``k`` and ``pose`` live on the host; ``r``, ``c``, ``l`` and ``logodds`` are read back from the device"""

    def __init__(self, owner, slot):
        self._m = owner
        self._slot = slot
        self.k = 0
        self.pose = None
        self.geom = -1
        self.sonar_xy = None          # set on the keyframe that brought a new geometry (host copy)
        self.box = None               # (rmin, rmax, cmin, cmax) of its cells when written ...
        self.base = (0, 0)            # ... and the growth counters then

    def _cells(self):
        m = self._m
        n = int(np.prod(m._geom_shape[self.geom]))
        r, c, l = np.zeros(n, np.uint16), np.zeros(n, np.uint16), np.zeros(n, np.float32)
        got = C.c_int(0)
        m._check(m._lib.sfe_map_cells(m._h, self._slot, r.ctypes.data_as(C.POINTER(C.c_uint16)),
                                      c.ctypes.data_as(C.POINTER(C.c_uint16)), _L.ptr(l, C.c_float), n, C.byref(got)))
        k = got.value
        return r[:k].copy(), c[:k].copy(), l[:k].copy()

    @property
    def r(self):
        return self._cells()[0]

    @property
    def c(self):
        return self._cells()[1]

    @property
    def l(self):
        return self._cells()[2]

    @property
    def logodds(self):
        m = self._m
        n = int(np.prod(m._geom_shape[self.geom]))
        out = np.zeros(n, np.float32)
        m._check(m._lib.sfe_map_logodds(m._h, self._slot, _L.ptr(out, C.c_float), n))
        return out

    def cell_box(self):
        """(rmin, rmax, cmin, cmax) of its cells in the grid's current coordinates"""
        dr, dc = self._m._grow[0] - self.base[0], self._m._grow[1] - self.base[1]
        r0, r1, c0, c1 = self.box
        return r0 + dr, r1 + dr, c0 + dc, c1 + dc


class Mapping(object):
    def __init__(self, ctx=None):
        self.ctx = ctx
        # map size: (x0, y0) is the corner of cell (0, 0); grown by `inc` metres on whichever side a keyframe leaves it
        self.x0 = -50.0
        self.y0 = -50.0
        self.width = 100.0
        self.height = 100.0
        self.inc = 50.0
        self.resolution = 0.2
        self.rows = None
        self.cols = None

        self.oculus = _Oculus()
        self.oculus_image_size = None
        self.oculus_r_skip = None
        self.oculus_c_skip = None

        self.intensity_grid = None
        self.counter_grid = None

        # method 1: log-odds update rule
        self.pub_intensity = False
        self.pub_occupancy1 = True
        self.hit_prob = 0.8
        self.miss_prob = 0.3
        self.inflation_angle = 0.05
        self.inflation_range = 0.5
        # method 2: point projection (refused; its bookkeeping is kept)
        self.pub_occupancy2 = True
        self.point_cloud = None
        self.inflation_radius = 0.5

        self.outlier_filter_radius = 5.0
        self.outlier_filter_min_points = 20

        self.min_translation = 0.5
        self.min_rotation = 0.05

        self.rmin, self.rmax = None, None
        self.cmin, self.cmax = None, None

        self.keyframes = []
        self.save_fig = False

        self._h = None
        self._geom = -1               # geometry of the next keyframe
        self._geom_shape = []
        self._grow = [0, 0]           # rows grown on top, columns grown on the left (sfe_map_shape)

    # ---- configuration ---------------------------------------------------------------------------------------------
    def load_yaml(self, path):
        """the parameters MappingNode.init_node reads (mapping_node.py:22-49), with its quirk: `inflation_range` is read
        into inflation_radius (then overwritten by `inflation_radius`), so inflation_range keeps its default"""
        import yaml
        with open(path, "r") as fh:
            cfg = yaml.safe_load(fh)
        self.x0, self.y0 = cfg["origin"]
        self.width, self.height = cfg["size"]
        self.resolution = cfg["resolution"]
        self.inc = cfg["inc"]
        self.pub_occupancy1 = cfg["pub_occupancy1"]
        self.hit_prob = cfg["hit_prob"]
        self.miss_prob = cfg["miss_prob"]
        self.inflation_angle = cfg["inflation_angle"]
        self.inflation_radius = cfg["inflation_range"]
        self.pub_occupancy2 = cfg["pub_occupancy2"]
        self.inflation_radius = cfg["inflation_radius"]
        self.outlier_filter_radius = cfg["outlier_filter_radius"]
        self.outlier_filter_min_points = cfg["outlier_filter_min_points"]
        self.pub_intensity = cfg["pub_intensity"]
        self.min_translation = cfg["min_translation"]
        self.min_rotation = cfg["min_rotation"]
        self.configure()

    def configure(self):
        if self.pub_intensity:
            raise NotImplementedError("Mapping.configure: pub_intensity=True (the intensity grid) is not implemented")
        self.hit_logodds = logit(self.hit_prob)
        self.miss_logodds = logit(self.miss_prob)
        xs = np.arange(0, self.width, self.resolution)
        ys = np.arange(0, self.height, self.resolution)
        self.rows = len(ys)
        self.cols = len(xs)
        if self.pub_occupancy2:
            dilate_hs = int(np.ceil(self.inflation_radius / self.resolution))
            self.dilate_size = 2 * dilate_hs + 1
        self.rmax = self.cmax = 0
        self.rmin = ys.shape[0] - 1
        self.cmin = xs.shape[0] - 1
        self.inc_r = int(self.inc / self.resolution)
        self.inc_c = int(self.inc / self.resolution)
        self.close()
        if self.ctx is None:
            self.ctx = _L.default_context()
        self._lib = self.ctx.lib
        h = C.c_void_p()
        self._check(self._lib.sfe_map_create(self.ctx.handle, self.rows, self.cols, C.byref(h)))
        self._h = h
        self._grow = [0, 0]
        self._geom = -1
        self._geom_shape = []
        self.keyframes = []
        self.oculus = _Oculus()

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._lib.sfe_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        return self.ctx._check(rc)

    # ---- the reference's methods -----------------------------------------------------------------------------------
    def pose_changed(self, pose, new_pose):
        dp = pose.between(new_pose)
        dt = np.linalg.norm(np.array([dp.x(), dp.y()]))
        dr = abs(dp.theta())
        return dt > self.min_translation or dr > self.min_rotation

    def _new_keyframe(self, pose, ping):
        kf = Submap(self, len(self.keyframes))
        kf.k = len(self.keyframes)
        kf.pose = pose
        if self.oculus.configure(ping):
            o = self.oculus
            self.oculus_r_skip = max(1, np.int32(np.floor(self.resolution / o.range_resolution)))
            range_resolution = o.angular_resolution * o.max_range
            self.oculus_c_skip = max(1, np.int32(np.floor(self.resolution / range_resolution)))
            B, R = np.meshgrid(o.bearings[:: self.oculus_c_skip], o.ranges[:: self.oculus_r_skip])
            X, Y = np.cos(B) * R, np.sin(B) * R
            kf.sonar_xy = np.ascontiguousarray(np.c_[X.ravel(), Y.ravel()].astype(np.float32))
            self.oculus_image_size = X.shape
            gid = C.c_int(0)
            self._check(self._lib.sfe_map_geometry(self._h, _L.ptr(kf.sonar_xy, C.c_float), X.shape[0], X.shape[1],
                                                    C.byref(gid)))
            self._geom = gid.value
            self._geom_shape.append(X.shape)
        kf.geom = self._geom
        # the slot of a keyframe is its index in self.keyframes (missed keys leave their slot unused)
        return kf

    def _hits(self, points):
        """-> (hits [n x 2] int32 of the downsampled image, hr, hc); None for no points (mapping.py:172-205)"""
        if not len(points):
            return None, -1, 0
        if self.outlier_filter_min_points > 1:
            points = pcl.remove_outlier(points[:, :2], self.outlier_filter_radius, self.outlier_filter_min_points,
                                        ctx=self.ctx)
        o = self.oculus
        c = o.b2c(np.arctan2(points[:, 1], points[:, 0]))
        c = np.clip(np.int32(np.round(c)), 0, o.num_bearings - 1)
        r = o.ra2ro(np.linalg.norm(points[:, :2], axis=1))
        r = np.clip(np.int32(np.round(r)), 0, o.num_ranges - 1)
        hc = int(round(self.inflation_angle / o.angular_resolution / self.oculus_c_skip))
        hr = int(round(self.inflation_range / o.range_resolution / self.oculus_r_skip))
        hits = np.c_[r // self.oculus_r_skip, c // self.oculus_c_skip].astype(np.int32)
        return hits, hr, hc

    def _measure(self, slot, geom, hits, hr, hc):
        if hr >= 0:
            kernel = gaussian_kernel(2 * hr + 1).dot(gaussian_kernel(2 * hc + 1).T)
            ktab = np.ascontiguousarray(kernel.astype(np.float32).ravel())
            div = kernel[hr, hc] / self.hit_prob
        else:
            hits, ktab, div = np.zeros((0, 2), np.int32), np.zeros(1, np.float32), 1.0
        hits = np.ascontiguousarray(hits, np.int32)
        hit32, miss32 = np.float32(self.hit_prob), np.float32(self.miss_prob)
        arr = lambda v, t: np.ascontiguousarray(np.array(v, t))
        self._check(self._lib.sfe_map_measure(
            self._h, 1, _L.ptr(arr([slot], np.int32), C.c_int32), _L.ptr(arr([geom], np.int32), C.c_int32),
            _L.ptr(arr([0, len(hits)], np.int32), C.c_int32), _L.ptr(hits if len(hits) else arr([0, 0], np.int32), C.c_int32),
            _L.ptr(arr([hr, hc], np.int32), C.c_int32), _L.ptr(arr([0], np.int32), C.c_int32), _L.ptr(ktab, C.c_float),
            len(ktab), _L.ptr(arr([div], np.float64), C.c_double), float(miss32), float(logit(miss32)), float(hit32),
            float(logit(hit32))))

    def measure_stages(self):
        """(hit mask, image before logit, first hits) of the last add_keyframe's measurement (for tests)"""
        shape = self.oculus_image_size
        hits = np.zeros(shape, np.uint8)
        prob = np.zeros(shape, np.float32)
        fh = np.zeros(shape[1], np.int32)
        self._check(self._lib.sfe_map_measure_stages(self._h, 0, _L.ptr(hits, C.c_uint8), _L.ptr(prob, C.c_float),
                                                     _L.ptr(fh, C.c_int32)))
        return hits, prob, fh

    def add_keyframe(self, key, pose, ping, points):
        self._check_supported()
        kf = self._new_keyframe(pose, ping)
        hits, hr, hc = self._hits(np.asarray(points) if len(points) else points)
        self._measure(kf._slot, kf.geom, hits, hr, hc)
        if self.pub_occupancy2:
            self.point_cloud = points
        self._fit([kf], dec=False)
        self._append(key, kf)

    def add_keyframe_logodds(self, key, pose, ping, logodds):
        """add_keyframe with a ready polar log-odds image (float32, the downsampled image's shape) instead of points"""
        self._check_supported()
        kf = self._new_keyframe(pose, ping)
        lo = np.ascontiguousarray(logodds, np.float32).ravel()
        if lo.size != int(np.prod(self.oculus_image_size)):
            raise ValueError("add_keyframe_logodds: %d values for a %r image" % (lo.size, self.oculus_image_size))
        self._check(self._lib.sfe_map_set_logodds(self._h, kf._slot, kf.geom, _L.ptr(lo, C.c_float)))
        self._fit([kf], dec=False)
        self._append(key, kf)

    def _append(self, key, kf):
        while len(self.keyframes) < key:
            self.keyframes.append(None)
        # the slot was taken as len(keyframes) before the missed keys were filled in: keep it with the keyframe
        self.keyframes.append(kf)

    def update_pose(self, key, new_pose):
        self.update_poses([key], [new_pose])

    def update_poses(self, keys, poses):
        """for k, p in zip(keys, poses): update_pose(k, p) -- the same bits, with the fit batched over keyframes"""
        group = []
        for key, new_pose in zip(keys, poses):
            assert key < len(self.keyframes)
            kf = self.keyframes[key]
            if not kf:
                continue
            if not self.pose_changed(kf.pose, new_pose):
                continue
            if kf in group:         # a slot is refitted at most once per device call (at the pose it had then)
                self._fit(group, dec=True)
                group = []
            kf.pose = new_pose
            group.append(kf)
        if group:
            self._fit(group, dec=True)

    def _fit(self, group, dec):
        """fit_grid + adjust_bounds + dec_grid / inc_grid of `group` in order (mapping.py:466-582)"""
        n = len(group)
        slots = np.array([kf._slot for kf in group], np.int32)
        pose4 = np.zeros((n, 4), np.float64)
        for i, kf in enumerate(group):
            yaw = kf.pose.theta()
            pose4[i] = np.cos(yaw), np.sin(yaw), kf.pose.x(), kf.pose.y()
        origin = np.zeros((n, 2), np.float64)
        origin[:] = self.y0, self.x0
        mm = self._bounds(slots, pose4, origin)
        shift = np.zeros((n, 2), np.int64)
        grow = [0, 0, 0, 0]       # top, bottom, left, right (cells)
        for i in range(n):
            r0, r1, c0, c1 = (int(v) for v in mm[i])
            top = left = 0
            # adjust_bounds: while the cells leave the grid, grow by inc on that side
            while not r0 >= 0:
                r0 += self.inc_r
                r1 += self.inc_r
                top += self.inc_r
                self.rmin += self.inc_r
                self.rmax += self.inc_r
                self.rows += self.inc_r
                self.y0 -= self.inc_r * self.resolution
                self.height += self.inc_r * self.resolution
            while not r1 < self.rows:
                self.rows += self.inc_r
                self.height += self.inc_r * self.resolution
                grow[1] += self.inc_r
            while not c0 >= 0:
                c0 += self.inc_c
                c1 += self.inc_c
                left += self.inc_c
                self.cmin += self.inc_c
                self.cmax += self.inc_c
                self.cols += self.inc_c
                self.x0 -= self.inc_c * self.resolution
                self.width += self.inc_c * self.resolution
            while not c1 < self.cols:
                self.cols += self.inc_c
                self.width += self.inc_c * self.resolution
                grow[3] += self.inc_c
            grow[0] += top
            grow[2] += left
            shift[i] = top, left
            # cells of the keyframes fitted so far move with the grid
            shift[:i, 0] += top
            shift[:i, 1] += left
            # inc_grid's box
            self.rmin, self.rmax = min(self.rmin, r0), max(self.rmax, r1)
            self.cmin, self.cmax = min(self.cmin, c0), max(self.cmax, c1)
            if (top or left) and i + 1 < n:
                # the keyframes after this one are fitted at the new origin
                origin[i + 1:] = self.y0, self.x0
                mm[i + 1:] = self._bounds(slots[i + 1:], pose4[i + 1:], origin[i + 1:])
        self._check(self._lib.sfe_map_grow(self._h, grow[0], grow[1], grow[2], grow[3]))
        self._grow[0] += grow[0]
        self._grow[1] += grow[2]
        mm32 = np.ascontiguousarray(mm, np.int32)
        shift32 = np.ascontiguousarray(shift, np.int32)
        decs = np.full(n, 1 if dec else 0, np.uint8)
        self._check(self._lib.sfe_map_refit(self._h, n, _L.ptr(slots, C.c_int32), _L.ptr(pose4, C.c_double),
                                            _L.ptr(origin, C.c_double), float(self.resolution), _L.ptr(mm32, C.c_int32),
                                            _L.ptr(shift32, C.c_int32), _L.ptr(decs, C.c_uint8)))
        for i, kf in enumerate(group):
            r0, r1, c0, c1 = (int(v) for v in mm[i])
            sr, sc = int(shift[i, 0]), int(shift[i, 1])
            kf.box = (r0 + sr, r1 + sr, c0 + sc, c1 + sc)
            kf.base = tuple(self._grow)

    def _bounds(self, slots, pose4, origin):
        n = len(slots)
        mm = np.zeros((n, 4), np.int32)
        self._check(self._lib.sfe_map_fit_bounds(self._h, n, _L.ptr(np.ascontiguousarray(slots), C.c_int32),
                                                 _L.ptr(np.ascontiguousarray(pose4), C.c_double),
                                                 _L.ptr(np.ascontiguousarray(origin), C.c_double), float(self.resolution),
                                                 _L.ptr(mm, C.c_int32)))
        return mm.astype(np.int64)

    @property
    def logodds_grid(self):
        if self._h is None:
            return None
        out = np.zeros((self.rows, self.cols), np.float32)
        self._check(self._lib.sfe_map_read_grid(self._h, 0, _L.ptr(out, C.c_float), out.size))
        return out

    def frames_grid(self):
        """the grid of the last get_occupancy_grid1(frames=...) call"""
        out = np.zeros((self.rows, self.cols), np.float32)
        self._check(self._lib.sfe_map_read_grid(self._h, 1, _L.ptr(out, C.c_float), out.size))
        return out

    def _check_supported(self):
        if self.pub_intensity:
            raise NotImplementedError("Mapping.add_keyframe: pub_intensity=True (the intensity grid) is not implemented")

    def get_intensity_grid(self):
        raise NotImplementedError("Mapping.get_intensity_grid: the intensity grid is not implemented")

    def get_occupancy_grid2(self, frames=None, resolution=None):
        raise NotImplementedError("Mapping.get_occupancy_grid2: method 2 (point projection + dilation) is not implemented")

    def get_occupancy_grid(self, frames=None, resolution=None):
        if self.pub_occupancy1:
            return self.get_occupancy_grid1(frames, resolution)
        elif self.pub_occupancy2:
            return self.get_occupancy_grid2(frames, resolution)

    def get_occupancy_grid1(self, frames=None, resolution=None):
        occ_msg = OccupancyGrid()
        occ_msg.header.frame_id = "map"
        which = 0
        if frames is None:
            rmin, rmax, cmin, cmax = self.rmin, self.rmax, self.cmin, self.cmax
        else:
            which = 1
            rmin, rmax, cmin, cmax = self.rmax, self.rmin, self.cmax, self.cmin
            slots = []
            for k in frames:
                if k >= len(self.keyframes) or self.keyframes[k] is None:
                    continue
                kf = self.keyframes[k]
                slots.append(kf._slot)
                r0, r1, c0, c1 = kf.cell_box()
                rmin, rmax = min(rmin, r0), max(rmax, r1)
                cmin, cmax = min(cmin, c0), max(cmax, c1)
            slots = np.array(slots, np.int32)
            self._check(self._lib.sfe_map_frames(self._h, len(slots), _L.ptr(slots, C.c_int32)))
        h, w = max(0, rmax - rmin + 1), max(0, cmax - cmin + 1)
        resize = 0
        inv = 1.0
        if resolution is not None and resolution > 0 and abs(resolution - self.resolution) > self.resolution * 1e-1:
            assert resolution >= self.resolution
            ratio = self.resolution / resolution
            # cv2.resize(probs, None, None, ratio, ratio, INTER_NEAREST): size cvRound(n * ratio), source floor(i / ratio)
            oh, ow = int(np.rint(h * ratio)), int(np.rint(w * ratio))
            inv, resize = 1.0 / ratio, 1
            resolution = self.resolution / ratio
        else:
            oh, ow = h, w
            resolution = self.resolution
        occ = np.zeros((oh, ow), np.int8)
        if oh * ow:
            self._check(self._lib.sfe_map_render(self._h, which, int(rmin), int(rmax), int(cmin), int(cmax), oh, ow,
                                                 float(inv), resize, occ.ctypes.data_as(C.POINTER(C.c_int8))))
        occ_msg.info.origin.position.x = self.x0 + cmin * resolution
        occ_msg.info.origin.position.y = self.y0 + rmin * resolution
        occ_msg.info.origin.orientation.x = 0
        occ_msg.info.origin.orientation.y = 0
        occ_msg.info.origin.orientation.z = 0
        occ_msg.info.origin.orientation.w = 1
        occ_msg.info.width = occ.shape[1]
        occ_msg.info.height = occ.shape[0]
        occ_msg.info.resolution = resolution
        occ_msg.data = list(occ.ravel())
        occ_msg.occ = occ
        return occ_msg
