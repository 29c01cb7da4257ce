"""bruce_slam's occupancy map (bruce_slam/mapping.py: the log-odds grid, method 1, and the point-projection map, method 2)
with the per-pixel work on the device.

``Mapping`` keeps the reference's attributes, defaults and control flow; the polar measurement image, the fit of every
pixel of a keyframe to grid cells with its deduplication, the ordered add / subtract of the cells on the float32 grid, growth
and rendering run in HIP kernels (csrc/sfe_map.hip, one ``sfe_map`` per Mapping).  What stays here is small or carries
rounding the device cannot reproduce bit for bit: the OculusProperty subset (ranges, bearings, the cubic b2c, ra2ro), the
skips, sonar_xy (once per geometry), the outlier filter (pcl.remove_outlier), the hit indices, the Gaussian kernel, the
per-keyframe cos / sin of the pose, pose_changed and the growth decisions of adjust_bounds.

Extensions: ``update_poses(keys, poses)`` (the loop of update_pose calls, batched: the same bits) and
``add_keyframe_logodds(key, pose, ping, logodds)`` (a ready polar log-odds image instead of points) and
``add_keyframe_store(key, pose, ping, store, handle)`` (the cloud taken from a ``store.CloudStore`` where it lies on the
device: the same map, bit for bit, without the cloud crossing to the host).

Method 2 (``get_occupancy_grid2``): the selection of the cloud by ``frames`` and the known region (the union of the listed
keyframes' cell boxes) are taken here; marking the free cells from the keyframes' cell lists, the outlier filter, the
projection, the inflation by the ellipse element and the resize run in one device call (sfe_map_render2), bit for bit the
reference's int8 image.  With ``pub_occupancy1`` off a keyframe takes no measurement, as in the reference, and
``get_occupancy_grid`` serves method 2.

The intensity mosaic (``pub_intensity``, ``get_intensity_grid``) is opt-in: the reference's line for it names two variables
that exist nowhere (mapping.py:242), so ``pub_intensity=True`` alone is refused as before; with ``intensity_skips="oculus"``
the ping is subsampled by the map's own skips and the mosaic is built on the device next to the log-odds grid: the same cell
lists carry the ping's byte, the same applies update a uint32 sum grid and a uint16 counter grid.  The ping's image is
``ping.ping`` or the keyword ``image=``.  INTEGRATION.md lists the deviations.
"""
import contextlib
import ctypes as C
import functools
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


class DeviceImage(object):
    """a uint8 [rows x cols] ping that lies on the device: ``ptr`` (a ctypes.c_void_p, or an address) of its first byte,
    ``stride`` bytes from one row to the next (``cols`` by default).  What ``MapBatch``'s ``images=`` takes in a list."""

    def __init__(self, ptr, rows, cols, stride=None):
        self.ptr = ptr if isinstance(ptr, C.c_void_p) else C.c_void_p(int(ptr))
        self.shape = (int(rows), int(cols))
        self.stride = int(cols if stride is None else stride)
        if self.stride < self.shape[1]:
            raise ValueError("DeviceImage: a row stride of %d bytes for %d columns" % (self.stride, self.shape[1]))


def intensity_setting(what, pub_intensity, intensity_skips):
    """-> whether the intensity mosaic is on.  ``intensity_skips``: None (the reference as it stands: ``pub_intensity`` cannot
    run) or "oculus" (its ``r_skip`` / ``c_skip`` are the map's ``oculus_r_skip`` / ``oculus_c_skip``)."""
    if intensity_skips is not None and intensity_skips != "oculus":
        raise ValueError("%s: intensity_skips must be None or \"oculus\", got %r" % (what, intensity_skips))
    if pub_intensity and intensity_skips is None:
        raise NotImplementedError(
            "%s: pub_intensity=True (the intensity grid) is not implemented as the reference writes it: its mapping.py:242 "
            "subsamples the ping by r_skip and c_skip, names that are defined nowhere, so its first add_keyframe ends in "
            "NameError.  Set intensity_skips=\"oculus\" to subsample by the map's own oculus_r_skip / oculus_c_skip, the only "
            "values under which the pixels match sonar_xy" % what)
    return bool(pub_intensity)


def ping_image(what, ping, image, oculus):
    """the full-size image of an add with the mosaic on: ``image`` or ``ping.ping`` -> uint8 [num_ranges x num_bearings],
    contiguous (the stand-in for the reference's r2n(ping.ping))"""
    src = image if image is not None else getattr(ping, "ping", None)
    if src is None:
        raise ValueError("%s: pub_intensity is on, so the add needs the ping's image: ping.ping or image=" % what)
    img = np.asarray(src)
    want = (int(oculus.num_ranges), int(oculus.num_bearings))
    if img.dtype != np.uint8 or img.shape != want:
        raise ValueError("%s: the ping's image is %s %r, the ping's geometry says uint8 %r (num_ranges x num_bearings)"
                         % (what, img.dtype, img.shape, want))
    return np.ascontiguousarray(img)


class Submap(object):
    """one keyframe: ``k`` and ``pose`` live on the host; ``r``, ``c``, ``l``, ``logodds`` and, with the intensity mosaic,
    ``i`` and ``intensity`` are read back from the device"""

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
        return m._read_cells(self._slot, int(np.prod(m._geom_shape[self.geom])))

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
        return m._read_logodds(self._slot, int(np.prod(m._geom_shape[self.geom])))

    @property
    def intensity(self):
        """the subsampled ping, raveled (mapping.py:243); None without the mosaic"""
        m = self._m
        return m._read_slot_intensity(self._slot, int(np.prod(m._geom_shape[self.geom])), True) if m._intensity else None

    @property
    def i(self):
        """intensity[sel] of the current cell list (mapping.py:499); None without the mosaic"""
        m = self._m
        return m._read_slot_intensity(self._slot, int(np.prod(m._geom_shape[self.geom])), False) if m._intensity else None

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

        # method 1: log-odds update rule
        self.pub_intensity = False
        self.intensity_skips = None   # None: pub_intensity is refused (mapping.py:242 cannot run); "oculus": the map's skips
        self._intensity = False       # the mosaic is on (configure)
        self.pub_occupancy1 = True
        self.hit_prob = 0.8
        self.miss_prob = 0.3
        self.inflation_angle = 0.05
        self.inflation_range = 0.5
        # method 2: point projection
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
        self._geom_shape = {}         # geometry id -> image shape
        self._grow = [0, 0]           # rows grown on top, columns grown on the left (sfe_map_shape)
        self._hit_key = None          # what _hit_indices reads of the current geometry (the key of its device hit table)
        self._hit_tabs = {}
        # the store feed since configure(): points fed, points the device left to the host, calls
        self.feed_stats = {"points": 0, "undecided": 0, "calls": 0}

    @property
    def intensity_grid(self):
        """uint32 [rows x cols], read back; None without the mosaic, as in the reference"""
        return self._read_intensity()[0] if self._intensity and self._live() else None

    @property
    def counter_grid(self):
        """uint16 [rows x cols], read back; None without the mosaic"""
        return self._read_intensity()[1] if self._intensity and self._live() else None

    def _live(self):
        return getattr(self, "_h", None) is not None

    @property
    def point_cloud(self):
        """the cloud of the last keyframe (the ``pub_occupancy2`` bookkeeping).  After a store-fed add it is read from the
        store when asked for: the handle must still be live then (not dropped by ``store.truncate``)."""
        if self._cloud_ref is not None:
            store, handle = self._cloud_ref
            return store.read(handle)
        return self._point_cloud

    @point_cloud.setter
    def point_cloud(self, points):
        self._point_cloud, self._cloud_ref = points, None

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
        self._configure_host()
        self.close()
        if self.ctx is None:
            self.ctx = _L.default_context()
        self._lib = self.ctx.lib
        h = C.c_void_p()
        self._check(self._lib.sfe_map_create(self.ctx.handle, self.rows, self.cols, C.byref(h)))
        self._h = h
        if self._intensity:
            self._check(self._lib.sfe_map_enable_intensity(self._h))
        self._hit_tabs = {}
        self.feed_stats = {"points": 0, "undecided": 0, "calls": 0}

    def _configure_host(self):
        self._intensity = intensity_setting("Mapping.configure", self.pub_intensity, self.intensity_skips)
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
        self._grow = [0, 0]
        self._geom = -1
        self._geom_shape = {}
        self._hit_key = None
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

    # ---- the device calls of one map (MapBatch's per-session views answer these from the shared map set) -------------
    def _new_slot(self):
        # the slot of a keyframe is its index in self.keyframes (missed keys leave their slot unused)
        return len(self.keyframes)

    def _register_geometry(self, sonar_xy, shape):
        self._hit_key = self._new_hit_key()
        gid = C.c_int(0)
        self._check(self._lib.sfe_map_geometry(self._h, _L.ptr(sonar_xy, C.c_float), shape[0], shape[1], C.byref(gid)))
        return gid.value

    def _new_hit_key(self):
        o = self.oculus
        return (o.num_ranges, o.range_resolution, o.bearings.tobytes(), int(self.oculus_r_skip), int(self.oculus_c_skip))

    def _geometry_state(self):
        return (dict(vars(self.oculus)), self.oculus_image_size, self.oculus_r_skip, self.oculus_c_skip, self._geom,
                self._hit_key, dict(self._geom_shape))

    def _restore_geometry(self, state):
        ocu, self.oculus_image_size, self.oculus_r_skip, self.oculus_c_skip, self._geom, self._hit_key, shapes = state
        vars(self.oculus).clear()
        vars(self.oculus).update(ocu)
        self._geom_shape = shapes

    @contextlib.contextmanager
    def _geometry_guard(self):
        """a refused add leaves the geometry state (sonar settings, skips, image size, geometry id) as it found it:
        _new_keyframe takes a ping's geometry before the device can refuse the image, the slot or the cloud"""
        state = self._geometry_state()
        try:
            yield
        except BaseException:
            self._restore_geometry(state)
            raise

    def _bound(self, name):
        """the device call sfe_map_`name` with this map's handle bound (a MapBatch session binds the set's call of that name,
        its handle and the session): what the reads below go through"""
        return functools.partial(getattr(self._lib, "sfe_map_" + name), self._h)

    def _read_cells(self, slot, n):
        r, c, l = np.zeros(n, np.uint16), np.zeros(n, np.uint16), np.zeros(n, np.float32)
        got = C.c_int(0)
        self._check(self._bound("cells")(slot, r.ctypes.data_as(C.POINTER(C.c_uint16)), c.ctypes.data_as(C.POINTER(C.c_uint16)),
                                         _L.ptr(l, C.c_float), n, C.byref(got)))
        k = got.value
        return r[:k].copy(), c[:k].copy(), l[:k].copy()

    def _read_logodds(self, slot, n):
        out = np.zeros(n, np.float32)
        self._check(self._bound("logodds")(slot, _L.ptr(out, C.c_float), n))
        return out

    def _read_intensity(self):
        inten, count = np.zeros((self.rows, self.cols), np.uint32), np.zeros((self.rows, self.cols), np.uint16)
        self._check(self._bound("read_intensity")(inten.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  count.ctypes.data_as(C.POINTER(C.c_uint16)), inten.size))
        return inten, count

    def _read_slot_intensity(self, slot, n, image):
        out = np.zeros(n, np.uint8)
        if image:
            self._check(self._bound("slot_intensity")(slot, _L.ptr(out, C.c_uint8), n, None, 0, None))
            return out
        got = C.c_int(0)
        self._check(self._bound("slot_intensity")(slot, None, 0, _L.ptr(out, C.c_uint8), n, C.byref(got)))
        return out[:got.value].copy()

    def _read_grid(self, which):
        out = np.zeros((self.rows, self.cols), np.float32)
        self._check(self._bound("read_grid")(which, _L.ptr(out, C.c_float), out.size))
        return out

    # ---- the reference's methods -----------------------------------------------------------------------------------
    def pose_changed(self, pose, new_pose):
        dp = pose.between(new_pose)
        dt = np.linalg.norm(np.array([dp.x(), dp.y()]))
        dr = abs(dp.theta())
        return dt > self.min_translation or dr > self.min_rotation

    def _new_keyframe(self, pose, ping):
        kf = Submap(self, self._new_slot())
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
            self._geom = self._register_geometry(kf.sonar_xy, X.shape)
            self._geom_shape[self._geom] = X.shape
        kf.geom = self._geom
        return kf

    def _hits(self, points):
        """-> (hits [n x 2] int32 of the downsampled image, hr, hc); None for no points (mapping.py:172-205).  With
        pub_occupancy1 off the reference takes no measurement (mapping.py:170; `points` is then the SLAM cloud, kept for
        method 2): the slot gets the all-miss image, which nothing reads, and its cell list is what the fit makes of it"""
        if not self.pub_occupancy1 or not len(points):
            return None, -1, 0
        if self.outlier_filter_min_points > 1:
            points = pcl.remove_outlier(points[:, :2], self.outlier_filter_radius, self.outlier_filter_min_points,
                                        ctx=self.ctx)
        return self._hit_indices(points)

    def _hit_indices(self, points):
        """the hits of filtered points: elementwise in the points, so many clouds of one geometry may go through at once"""
        o = self.oculus
        c = o.b2c(np.arctan2(points[:, 1], points[:, 0]))
        c = np.clip(np.int32(np.round(c)), 0, o.num_bearings - 1)
        r = o.ra2ro(np.linalg.norm(points[:, :2], axis=1))
        r = np.clip(np.int32(np.round(r)), 0, o.num_ranges - 1)
        hr, hc = self._hit_halves()
        hits = np.c_[r // self.oculus_r_skip, c // self.oculus_c_skip].astype(np.int32)
        return hits, hr, hc

    def _hit_halves(self):
        """(hr, hc): the half sizes of the inflation kernel in pixels of the downsampled image"""
        o = self.oculus
        hc = int(round(self.inflation_angle / o.angular_resolution / self.oculus_c_skip))
        hr = int(round(self.inflation_range / o.range_resolution / self.oculus_r_skip))
        return hr, hc

    def _measure_args(self, hits, hr, hc):
        """-> (hits int32 [n x 2], the float32 kernel table, div) of one keyframe's measurement"""
        if hr >= 0:
            kernel = gaussian_kernel(2 * hr + 1).dot(gaussian_kernel(2 * hc + 1).T)
            ktab = np.ascontiguousarray(kernel.astype(np.float32).ravel())
            div = kernel[hr, hc] / self.hit_prob
        else:
            hits, ktab, div = np.zeros((0, 2), np.int32), np.zeros(1, np.float32), 1.0
        return np.ascontiguousarray(hits, np.int32), ktab, div

    def _measure(self, slot, geom, hits, hr, hc):
        hits = _hits32(hits, hr)
        self._check(self._lib.sfe_map_measure(self._h, 1, _i32p(slot), _i32p(geom), _i32p(0, len(hits)),
                                              _L.ptr(hits, C.c_int32) if len(hits) else _i32p(0, 0),
                                              *kernel_tables(self, [self], [(hr, hc)])))

    def measure_stages(self):
        """(hit mask, image before logit, first hits) of the last add_keyframe's measurement (for tests)"""
        shape = self.oculus_image_size
        hits = np.zeros(shape, np.uint8)
        prob = np.zeros(shape, np.float32)
        fh = np.zeros(shape[1], np.int32)
        self._check(self._lib.sfe_map_measure_stages(self._h, 0, _L.ptr(hits, C.c_uint8), _L.ptr(prob, C.c_float),
                                                     _L.ptr(fh, C.c_int32)))
        return hits, prob, fh

    def _image_guard(self, what, image):
        """what an add runs its geometry and measurement steps under: with the mosaic, ``_geometry_guard`` (a missing or
        misshapen image leaves the map as it was); without it nothing, and ``image=`` is refused"""
        if self._intensity:
            return self._geometry_guard()
        if image is not None:
            raise ValueError("%s: image= without the intensity mosaic (pub_intensity with intensity_skips)" % what)
        return contextlib.nullcontext()

    def _set_image(self, kf, img):
        self._check(self._lib.sfe_map_set_intensity(self._h, kf._slot, kf.geom, img.shape[0], img.shape[1],
                                                    int(self.oculus_r_skip), int(self.oculus_c_skip), _L.ptr(img, C.c_uint8)))

    def add_keyframe(self, key, pose, ping, points, image=None):
        self._check_supported()
        with self._image_guard("Mapping.add_keyframe", image):
            kf = self._new_keyframe(pose, ping)
            img = ping_image("Mapping.add_keyframe", ping, image, self.oculus) if self._intensity else None
            hits, hr, hc = self._hits(np.asarray(points) if len(points) else points)
            self._measure(kf._slot, kf.geom, hits, hr, hc)
            if img is not None:
                self._set_image(kf, img)
        if self.pub_occupancy2:
            self.point_cloud = points
        self._fit([kf], dec=False)
        self._append(key, kf)

    def add_keyframe_store(self, key, pose, ping, store, handle, image=None):
        """``add_keyframe(key, pose, ping, store.read(handle))``, bit for bit, without the cloud leaving the device: the
        outlier filter, the hit cells and the measurement run from the store's pool (``store``: a CloudStore of this map's
        context).  In mapping_node.py's flow: ``handle, n, _ = fe.callback_store(ping, store)`` in place of the feature
        cloud, then this call in place of ``add_keyframe``.

        The device decides a point's bearing column only outside a guard band (``guard_margin``); the few points it leaves
        undecided come back and go through ``_hit_indices`` here (``feed_stats`` counts them).  With ``pub_occupancy2``,
        ``point_cloud`` is read from the store on access: the handle must still be live then.  A dead handle, or an image
        or a slot the map cannot hold, raises and leaves the map as it was."""
        self._check_supported()
        if self._h is None:
            raise RuntimeError("Mapping.add_keyframe_store: configure() first")
        if getattr(store, "ctx", None) is not self.ctx:
            raise ValueError("Mapping.add_keyframe_store: the store belongs to another context")
        handle = int(handle)
        if image is not None and not self._intensity:
            self._image_guard("Mapping.add_keyframe_store", image)
        with self._geometry_guard():
            kf = self._new_keyframe(pose, ping)
            img = ping_image("Mapping.add_keyframe_store", ping, image, self.oculus) if self._intensity else None
            self._measure_store(kf, store, handle)
            if img is not None:
                self._set_image(kf, img)
        if self.pub_occupancy2:
            self._cloud_ref = (store, handle)
        self._fit([kf], dec=False)
        self._append(key, kf)

    def _hit_table(self):
        return device_hit_table(self, self._hit_tabs, lambda *a: self._lib.sfe_map_hit_table(self._h, *a))

    def _measure_store(self, kf, store, handle):
        head = (store.handle, 1, _i32p(kf._slot), _i32p(kf.geom), _i32p(handle), _i32p(self._hit_table()),
                float(self.outlier_filter_radius), int(self.outlier_filter_min_points))
        measure_store(self, [self], functools.partial(self._lib.sfe_map_measure_store, self._h, *head),
                      functools.partial(self._lib.sfe_map_measure_store_undecided, self._h),
                      functools.partial(self._lib.sfe_map_measure_store_finish, self._h))

    def add_keyframe_logodds(self, key, pose, ping, logodds, image=None):
        """add_keyframe with a ready polar log-odds image (float32, the downsampled image's shape) instead of points"""
        self._check_supported()
        with self._image_guard("Mapping.add_keyframe_logodds", image):
            kf = self._new_keyframe(pose, ping)
            img = ping_image("Mapping.add_keyframe_logodds", ping, image, self.oculus) if self._intensity else None
            lo = np.ascontiguousarray(logodds, np.float32).ravel()
            if lo.size != int(np.prod(self.oculus_image_size)):
                raise ValueError("add_keyframe_logodds: %d values for a %r image" % (lo.size, self.oculus_image_size))
            self._check(self._lib.sfe_map_set_logodds(self._h, kf._slot, kf.geom, _L.ptr(lo, C.c_float)))
            if img is not None:
                self._set_image(kf, img)
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

    def _adjust(self, mm, shift, grow, origin, start):
        """adjust_bounds and inc_grid's box for keyframes start.. of a fit group, from their bounds `mm`; fills shift / grow.
        -> the index of the first keyframe whose bounds must be taken again (the origin moved: origin[i:] is updated), or n"""
        n = len(mm)
        for i in range(start, n):
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
                origin[i + 1:] = self.y0, self.x0
                return i + 1
        return n

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
        i = self._adjust(mm, shift, grow, origin, 0)
        while i < n:
            # the keyframes after a growth that moved the origin are fitted at the new origin
            mm[i:] = self._bounds(slots[i:], pose4[i:], origin[i:])
            i = self._adjust(mm, shift, grow, origin, i)
        self._check(self._lib.sfe_map_grow(self._h, grow[0], grow[1], grow[2], grow[3]))
        self._grow[0] += grow[0]
        self._grow[1] += grow[2]
        mm32 = np.ascontiguousarray(mm, np.int32)
        shift32 = np.ascontiguousarray(shift, np.int32)
        decs = np.full(n, 1 if dec else 0, np.uint8)
        self._check(self._lib.sfe_map_refit(self._h, n, _L.ptr(slots, C.c_int32), _L.ptr(pose4, C.c_double),
                                            _L.ptr(origin, C.c_double), float(self.resolution), _L.ptr(mm32, C.c_int32),
                                            _L.ptr(shift32, C.c_int32), _L.ptr(decs, C.c_uint8)))
        self._fitted(group, mm, shift)

    def _fitted(self, group, mm, shift):
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
        return None if self._h is None else self._read_grid(0)

    def frames_grid(self):
        """the grid of the last get_occupancy_grid1(frames=...) call"""
        return self._read_grid(1)

    def _check_supported(self):
        if self.pub_intensity and not self._intensity:
            raise NotImplementedError("Mapping.add_keyframe: pub_intensity=True (the intensity grid) was set after configure(): "
                                      "the map was configured without it")

    def _intensity_box(self, what):
        """what get_intensity_grid needs, named when it is missing -> the box it renders"""
        if not (self._intensity and self._live()):
            raise NotImplementedError("%s: get_intensity_grid is not implemented for a map without the intensity grid: "
                                      "configure() with pub_intensity=True and intensity_skips=\"oculus\"" % what)
        if not any(kf is not None for kf in self.keyframes):
            raise RuntimeError("%s: no keyframe yet, so there is no box to publish" % what)
        return int(self.rmin), int(self.rmax), int(self.cmin), int(self.cmax)

    def get_intensity_grid(self):
        """mapping.py:272-298: the box of the mosaic, -1 where nothing was counted, else the mean intensity in percent"""
        box = self._intensity_box("Mapping.get_intensity_grid")
        occ = np.zeros((box[1] - box[0] + 1, box[3] - box[2] + 1), np.int8)
        self._check(self._lib.sfe_map_render_intensity(self._h, box[0], box[1], box[2], box[3],
                                                       occ.ctypes.data_as(C.POINTER(C.c_int8))))
        return self._grid_msg(box, self.resolution, occ)

    def _check_method2(self, what, cloud):
        """what method 2 needs, named when it is missing.  (Before configure() the answer stays NotImplementedError, a
        RuntimeError like the other entry points' "configure() first".)"""
        if self.rows is None:
            raise NotImplementedError("%s: get_occupancy_grid2 is not implemented for a map that was never configured: "
                                      "configure() first" % what)
        if not self.pub_occupancy2:
            raise RuntimeError("%s: the map was configured with pub_occupancy2=False, so it has no dilate_size" % what)
        if cloud is None:
            raise RuntimeError("%s: no point_cloud yet: add a keyframe, or set point_cloud to the SLAM cloud "
                               "(x, y, z, key)" % what)
        if self.dilate_size < 1 or self.dilate_size % 2 == 0:
            raise ValueError("%s: dilate_size = %r; the ellipse element is built for odd sizes (2 * dilate_hs + 1, as "
                             "configure() sets it)" % (what, self.dilate_size))

    def get_occupancy_grid2(self, frames=None, resolution=None):
        """mapping.py:357-439: unknown -1, the listed keyframes' cells 0 (all keyframes by default), the cells under the
        inflated projection of ``point_cloud`` 100 (with ``frames``: of its rows whose column 3 is a listed key)"""
        cloud = self.point_cloud if self.rows is not None and self.pub_occupancy2 else None
        self._check_method2("Mapping.get_occupancy_grid2", cloud)
        points = select_points(np.asarray(cloud), frames)
        slots, box, origin, (oh, ow), inv, resize, resolution = self._render2_plan(frames, resolution)
        xy = np.ascontiguousarray(points, np.float64)
        occ = np.zeros((oh, ow), np.int8)
        self._check(self._lib.sfe_map_render2(
            self._h, len(slots), _L.ptr(slots, C.c_int32), box[0], box[1], box[2], box[3],
            _L.ptr(xy if len(xy) else np.zeros(2), C.c_double), len(xy), int(self.outlier_filter_min_points > 1),
            float(self.outlier_filter_radius), int(self.outlier_filter_min_points), self.dilate_size // 2, origin[0], origin[1],
            float(self.resolution), oh, ow, inv, resize, occ.ctypes.data_as(C.POINTER(C.c_int8))))
        return self._grid_msg(box, resolution, occ, origin)

    def get_occupancy_grid2_store(self, store, handle, frames=None, resolution=None):
        """``get_occupancy_grid2(frames, resolution)`` with ``point_cloud = np.c_[store.read(handle), 0,
        store.read_keys(handle)].astype(np.float32)``, without the cloud leaving the device: the selection by ``frames``
        (``select_points``' multiset), the outlier filter and the projection read cloud ``handle`` of ``store`` (a CloudStore
        of this map's context) where it lies.  The cloud is a keyed one -- ``FrontEnd.slam_cloud()``,
        ``store.get_points_keys(...)`` or ``store.put_keys(...)`` -- or, with ``frames=None``, any cloud.  ``point_cloud`` is
        neither read nor set.  A dead handle, or a frame list for a cloud without keys, raises SonarFEError; nothing
        changes then."""
        what = "Mapping.get_occupancy_grid2_store"
        self._check_method2(what, ())
        if getattr(store, "ctx", None) is not self.ctx:
            raise ValueError("%s: the store belongs to another context" % what)
        slots, box, origin, (oh, ow), inv, resize, resolution = self._render2_plan(frames, resolution)
        listed = frame_list(frames)
        occ = np.zeros((oh, ow), np.int8)
        self._check(self._lib.sfe_map_render2_store(
            self._h, store.handle, len(slots), _L.ptr(slots, C.c_int32), box[0], box[1], box[2], box[3], int(handle), int(frames is None),
            _L.ptr(listed if len(listed) else np.zeros(1, np.int32), C.c_int32), len(listed),
            int(self.outlier_filter_min_points > 1), float(self.outlier_filter_radius), int(self.outlier_filter_min_points),
            self.dilate_size // 2, origin[0], origin[1], float(self.resolution), oh, ow, inv, resize,
            occ.ctypes.data_as(C.POINTER(C.c_int8))))
        return self._grid_msg(box, resolution, occ, origin)

    def get_occupancy_grid(self, frames=None, resolution=None):
        if self.pub_occupancy1:
            return self.get_occupancy_grid1(frames, resolution)
        elif self.pub_occupancy2:
            return self.get_occupancy_grid2(frames, resolution)

    def _render_plan(self, frames, resolution):
        """-> (which, slots of `frames`, (rmin, rmax, cmin, cmax), (oh, ow), inv, resize, resolution)"""
        which, slots = 0, None
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
        h, w = max(0, rmax - rmin + 1), max(0, cmax - cmin + 1)
        (oh, ow), inv, resize, resolution = self._resize_plan(h, w, resolution)
        return which, slots, (int(rmin), int(rmax), int(cmin), int(cmax)), (oh, ow), inv, resize, resolution

    def _resize_plan(self, h, w, resolution):
        """the resize both methods end with -> ((oh, ow), inv, resize, the resolution published)"""
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
        return (oh, ow), float(inv), resize, resolution

    def _render2_plan(self, frames, resolution):
        """method 2's known region and sizes -> (slots of `frames`, (rmin, rmax, cmin, cmax), (y0, x0) of its corner,
        (oh, ow), inv, resize, resolution).  The region is the tight box of the cells marked free, which is the union of the
        listed keyframes' cell boxes; its corner is taken with the map's resolution, also when the image is resized
        (mapping.py:401-402).  Nothing marked: the reference's IndexError (mapping.py:384)."""
        slots, boxes = [], []
        for k in (range(len(self.keyframes)) if frames is None else frames):
            if k >= len(self.keyframes) or self.keyframes[k] is None:
                continue
            slots.append(self.keyframes[k]._slot)
            boxes.append(self.keyframes[k].cell_box())
        if not slots:
            raise IndexError("get_occupancy_grid2: no keyframe of frames=%r has cells, so there is no known region"
                             % (None if frames is None else list(frames),))
        rmin, cmin = min(b[0] for b in boxes), min(b[2] for b in boxes)
        rmax, cmax = max(b[1] for b in boxes), max(b[3] for b in boxes)
        x0 = self.x0 + cmin * self.resolution
        y0 = self.y0 + rmin * self.resolution
        size, inv, resize, resolution = self._resize_plan(rmax - rmin + 1, cmax - cmin + 1, resolution)
        return (np.array(slots, np.int32), (int(rmin), int(rmax), int(cmin), int(cmax)), (float(y0), float(x0)), size, inv,
                resize, resolution)

    def _grid_msg(self, box, resolution, occ, origin=None):
        """the message of an image of `box`; its origin as method 1 takes it (with the published resolution), or `origin` =
        (y, x) as given (method 2)"""
        rmin, cmin = box[0], box[2]
        occ_msg = OccupancyGrid()
        occ_msg.header.frame_id = "map"
        occ_msg.info.origin.position.x = self.x0 + cmin * resolution if origin is None else origin[1]
        occ_msg.info.origin.position.y = self.y0 + rmin * resolution if origin is None else origin[0]
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

    def get_occupancy_grid1(self, frames=None, resolution=None):
        which, slots, box, (oh, ow), inv, resize, resolution = self._render_plan(frames, resolution)
        if which:
            self._check(self._lib.sfe_map_frames(self._h, len(slots), _L.ptr(slots, C.c_int32)))
        occ = np.zeros((oh, ow), np.int8)
        if oh * ow:
            self._check(self._lib.sfe_map_render(self._h, which, box[0], box[1], box[2], box[3], oh, ow, inv, resize,
                                                 occ.ctypes.data_as(C.POINTER(C.c_int8))))
        return self._grid_msg(box, resolution, occ)


# ---- method 2's cloud -----------------------------------------------------------------------------------------------------
def select_points(point_cloud, frames):
    """the points get_occupancy_grid2 projects (mapping.py:365-372), as written there: columns x, y of the whole cloud, or
    with `frames` the rows whose column 3 is k, for every k in list order (a key listed twice gives its rows twice; a key
    without a keyframe still gives its rows), behind np.zeros((0, 2)): float64"""
    points = point_cloud[:, :2]
    if frames is not None:
        points = [np.zeros((0, 2))]
        keys = np.uint32(point_cloud[:, 3])
        for k in frames:
            points.append(point_cloud[keys == k, :2])
        points = np.concatenate(points)
    return points


def frame_list(frames):
    """`frames` as the device's selection reads it: int32, in list order, repeats kept.  The stored keys are integers in
    [0, 2^31), so an entry that is none (negative, too large, not a whole number) selects nothing, as in select_points'
    comparison; it becomes -1, which no key equals."""
    out = []
    for k in (() if frames is None else frames):
        whole = isinstance(k, (int, np.integer)) or (isinstance(k, (float, np.floating)) and np.isfinite(k) and k == int(k))
        out.append(int(k) if whole and 0 <= int(k) < 2 ** 31 else -1)
    return np.array(out, np.int32)


# ---- what Mapping and MapBatch hand the measurement ------------------------------------------------------------------------
def _i32p(*values):
    return _L.ptr(np.ascontiguousarray(np.array(values, np.int32).reshape(-1)), C.c_int32)


def _hits32(hits, hr):
    """a keyframe's hits as the device takes them: int32 [n x 2]; none for a keyframe without points (hr < 0)"""
    return np.ascontiguousarray(hits, np.int32).reshape(-1, 2) if hr >= 0 else np.zeros((0, 2), np.int32)


def kernel_tables(owner, views, halves=None):
    """The inflation kernels of a measurement call with one keyframe per map view in ``views``; ``halves[i]`` = its (hr, hc),
    by default what its sonar geometry gives.  -> the arguments every measure call ends its inputs with: hrhc, k_off, ktab (the
    distinct float32 kernels back to back), n_ktab, div, and ``owner``'s miss / hit probabilities in float32 with their
    logits"""
    halves = [v._hit_halves() for v in views] if halves is None else halves
    k_off, div, ktabs, at, n_k = [], [], [], {}, 0
    for v, (hr, hc) in zip(views, halves):
        _, ktab, d = v._measure_args(np.zeros((0, 2), np.int32), hr, hc)
        if (hr, hc) not in at:
            at[(hr, hc)] = n_k
            ktabs.append(ktab)
            n_k += len(ktab)
        k_off.append(at[(hr, hc)])
        div.append(d)
    ktab = np.ascontiguousarray(np.concatenate(ktabs), np.float32)
    hit32, miss32 = np.float32(owner.hit_prob), np.float32(owner.miss_prob)
    return (_i32p(halves), _i32p(k_off), _L.ptr(ktab, C.c_float), len(ktab),
            _L.ptr(np.ascontiguousarray(np.array(div, np.float64)), C.c_double), float(miss32), float(logit(miss32)),
            float(hit32), float(logit(hit32)))


def measure_store(owner, views, phase_one, undecided, finish):
    """A store-fed measurement of one keyframe per map view in ``views``, the whole protocol.  The three calls are the
    owner's sfe_map(set)_measure_store (with everything before the kernel tables bound), _undecided and _finish (with the
    handle bound).  Phase two, for the few points the device left undecided: they come back, go through ``_hit_indices``
    once per sonar geometry, and their cells go back before the measurement runs.  Counts into ``owner.feed_stats``."""
    n_pts, n_und = np.zeros(len(views), np.int32), np.zeros(len(views), np.int32)
    with owner.ctx.lock:        # the store's slot table and the context's pinned staging
        owner._check(phase_one(*kernel_tables(owner, views), _L.ptr(n_pts, C.c_int32), _L.ptr(n_und, C.c_int32)))
        total = int(n_und.sum())
        if total:
            xy, pos = np.zeros((total, 2), np.float32), np.zeros(total, np.int32)
            owner._check(undecided(_L.ptr(xy, C.c_float), _L.ptr(pos, C.c_int32), total))
            job = np.searchsorted(np.cumsum(n_pts), pos, side="right")
            cells = np.zeros((total, 2), np.int32)
            groups = {}
            for i, j in enumerate(job):
                groups.setdefault(views[j]._hit_key, []).append(i)
            for idx in groups.values():
                cells[idx] = views[job[idx[0]]]._hit_indices(xy[idx])[0]
            owner._check(finish(total, _L.ptr(pos, C.c_int32), _L.ptr(np.ascontiguousarray(cells), C.c_int32)))
    owner.feed_stats["points"] += int(n_pts.sum())
    owner.feed_stats["undecided"] += total
    owner.feed_stats["calls"] += 1


# ---- the hit cells on the device (the store feed) ------------------------------------------------------------------------
def spline_table(oculus):
    """``oculus.b2c`` as one cubic per knot interval, in double -> (breaks [n + 1], coef [n x 4]): on
    [breaks[k], breaks[k + 1]) the column is polyval(coef[k], angle - breaks[k]).  (The not-a-knot spline has no knot at
    the second and the second to last bearing, so there are two intervals fewer than bearing gaps.)"""
    from scipy.interpolate import PPoly
    sp = oculus.b2c._spline
    pp = PPoly.from_spline((np.asarray(sp.t, np.float64), np.asarray(sp.c, np.float64).reshape(-1), sp.k))
    live = np.nonzero(np.diff(pp.x) > 0)[0]
    breaks = np.ascontiguousarray(np.r_[pp.x[live], pp.x[live[-1] + 1]], np.float64)
    return breaks, np.ascontiguousarray(pp.c[:, live].T, np.float64)


def guard_margin(oculus, breaks, coef):
    """How far, in columns, a column value computed from a double atan2 must stay from a rounding boundary x.5 (and, in
    radians, its angle from the ends of the bearing table) for numpy's float32 route to round it the same way:
    2 * ulp_float32(max(1, largest |bearing|)) * max(1, largest |column slope| of the table) + 1e-9.  numpy's atan2f is
    within one such ulp of the angle; the factor 2 and the 1e-9 cover the last bits of the two spline evaluations."""
    h = np.diff(breaks)
    a, b, c = 3 * coef[:, 0], 2 * coef[:, 1], coef[:, 2]            # the slope on interval k: a d^2 + b d + c, 0 <= d <= h
    slope = max(np.abs(c).max(), np.abs((a * h + b) * h + c).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(a != 0, -b / (2 * a), -1.0)
    inside = (d > 0) & (d < h)
    if inside.any():
        slope = max(slope, np.abs((a * d + b) * d + c)[inside].max())
    ulp = float(np.spacing(np.float32(max(1.0, float(np.abs(oculus.bearings).max())))))
    return 2.0 * ulp * max(1.0, float(slope)) + 1e-9


def decide_columns(oculus, points, breaks, coef, margin):
    """The device rule of the store feed (csrc/sfe_map.hip: feed_hit_cells_kernel), restated for tests: float32 points
    -> (columns before the skip, decided).  Undecided points carry column -1."""
    a = np.arctan2(points[:, 1].astype(np.float64), points[:, 0].astype(np.float64))
    first, last = float(oculus.bearings[0]), float(oculus.bearings[-1])
    outside = (a < first - margin) | (a > last + margin)
    inside = (a > first + margin) & (a < last - margin)
    k = np.clip(np.searchsorted(breaks, a, side="right") - 1, 0, len(coef) - 1)
    d = a - breaks[k]
    v = ((coef[k, 0] * d + coef[k, 1]) * d + coef[k, 2]) * d + coef[k, 3]
    safe = inside & (np.abs(v - np.floor(v) - 0.5) > margin)
    col = np.full(len(points), -1, np.int64)
    col[safe] = np.clip(np.rint(v[safe]), 0, oculus.num_bearings - 1).astype(np.int64)
    col[outside] = 0
    return col, safe | outside


def hit_table_args(v):
    """what the device's hit table holds of map ``v``'s sonar geometry and skips: the arguments of sfe_map_hit_table /
    sfe_mapset_hit_table after the handle, without id_out -> (bearings, num_bearings, breaks, coef, n_intervals, margin,
    num_ranges, range_resolution, range_in_double, r_skip, c_skip)"""
    o = v.oculus
    breaks, coef = spline_table(o)
    bearings = np.ascontiguousarray(o.bearings, np.float32)
    wide = np.result_type(np.float32, o.range_resolution) == np.float64     # ra / res of float32 ranges
    return (bearings, len(bearings), breaks, coef, len(coef), guard_margin(o, breaks, coef), int(o.num_ranges),
            float(o.range_resolution), int(wide), int(v.oculus_r_skip), int(v.oculus_c_skip))


def device_hit_table(v, tabs, register):
    """the id of the device's copy of what _hit_indices reads of map ``v``'s sonar geometry, stored once per geometry in
    ``tabs`` (keyed by ``v._hit_key``); ``register(*ctypes arguments)`` is the owner's sfe_map(set)_hit_table call"""
    key = v._hit_key
    if key not in tabs:
        bearings, nb, breaks, coef, n_iv, margin, num_ranges, res, wide, r_skip, c_skip = hit_table_args(v)
        tid = C.c_int(0)
        v._check(register(_L.ptr(bearings, C.c_float), nb, _L.ptr(breaks, C.c_double), _L.ptr(coef, C.c_double), n_iv, margin,
                          num_ranges, res, wide, r_skip, c_skip, C.byref(tid)))
        tabs[key] = tid.value
    return tabs[key]


# ---- S maps in lock-step ---------------------------------------------------------------------------------------------
SETTINGS = ("x0", "y0", "width", "height", "inc", "resolution", "pub_intensity", "intensity_skips", "pub_occupancy1", "hit_prob", "miss_prob",
            "inflation_angle", "inflation_range", "pub_occupancy2", "inflation_radius", "outlier_filter_radius",
            "outlier_filter_min_points", "min_translation", "min_rotation")


def plan_updates(keyframes, pose_changed, sessions, keys, poses):
    """Mapping.update_poses' rules for flat (session, key, pose) lists -> waves of fit groups.

    ``keyframes[s]`` is session s's keyframe list (None for a missed key), ``pose_changed[s](old, new)`` its gate.  Per
    session, in list order: a missed key and an unchanged pose drop out; an accepted keyframe takes its new pose at once (so a
    later entry for the same key is gated against it); a keyframe listed again closes the session's open group, because a slot
    is refitted at most once per device call.  -> [wave][(session, [(keyframe, pose) in order])]: wave w holds the w-th group of
    every session that has one, sessions in order of first appearance; a group is fitted at the poses listed in it (a keyframe
    listed again has moved on by the time its first group is fitted)."""
    if not (len(sessions) == len(keys) == len(poses)):
        raise ValueError("update_poses: %d sessions, %d keys, %d poses" % (len(sessions), len(keys), len(poses)))
    groups, order = {}, []
    for s, key, new_pose in zip(sessions, keys, poses):
        s = int(s)
        kfs = keyframes[s]
        assert key < len(kfs)
        kf = kfs[key]
        if not kf:
            continue
        if not pose_changed[s](kf.pose, new_pose):
            continue
        if s not in groups:
            groups[s] = [[]]
            order.append(s)
        if any(kf is g for g, _ in groups[s][-1]):
            groups[s].append([])
        kf.pose = new_pose
        groups[s][-1].append((kf, new_pose))
    waves = []
    for s in order:
        for w, g in enumerate(groups[s]):
            while len(waves) <= w:
                waves.append([])
            waves[w].append((s, g))
    return waves


class _SessionMap(Mapping):
    """``MapBatch.maps[s]``: Mapping's attributes and read surface for one session of a MapBatch.  Its state on the device
    lives in the batch's map set; its own add_keyframe / update_poses calls are batch calls for this one session."""

    def __init__(self, batch, s):
        Mapping.__init__(self, batch.ctx)
        self._b, self._s = batch, s
        self._n_slots = 0
        self._meas_job = -1

    def configure(self):
        raise RuntimeError("a MapBatch session is configured through MapBatch.configure")

    def load_yaml(self, path):
        raise RuntimeError("a MapBatch session is configured through MapBatch.load_yaml")

    def close(self):
        pass

    def _check(self, rc):
        return self._b.ctx._check(rc)

    def _new_slot(self):
        return self._n_slots        # slots are handed out densely: max_keyframes counts keyframes, not keys

    def _register_geometry(self, sonar_xy, shape):
        self._hit_key = self._new_hit_key()
        return self._b._geometry(sonar_xy, shape)

    def _bound(self, name):
        b = self._b
        return functools.partial(getattr(b._lib, "sfe_mapset_" + name), b._h, self._s)

    def _live(self):
        return getattr(self._b, "_h", None) is not None

    @property
    def logodds_grid(self):
        return self._read_grid(0)       # (its own _h stays None: the handle is the batch's)

    def device_shape(self):
        """(rows, cols, rows grown on top, columns grown on the left) as the device holds them"""
        out = np.zeros(4, np.int32)
        self._check(self._bound("shape")(_L.ptr(out, C.c_int32)))
        return tuple(int(v) for v in out)

    def measure_stages(self):
        b = self._b
        if self._meas_job < 0:
            raise RuntimeError("measure_stages: session %d took no part in the batch's last add_keyframes call" % self._s)
        shape = self.oculus_image_size
        hits, prob, fh = np.zeros(shape, np.uint8), np.zeros(shape, np.float32), np.zeros(shape[1], np.int32)
        self._check(b._lib.sfe_mapset_measure_stages(b._h, self._meas_job, _L.ptr(hits, C.c_uint8), _L.ptr(prob, C.c_float),
                                                     _L.ptr(fh, C.c_int32)))
        return hits, prob, fh

    def _images1(self, ping, image):
        """the batch's images= for this one session"""
        if image is None and self._intensity:
            image = getattr(ping, "ping", None)
        return None if image is None else [image]

    def add_keyframe(self, key, pose, ping, points, image=None):
        self._b.add_keyframes([self._s], [key], [pose], ping, [points], images=self._images1(ping, image))

    def add_keyframe_logodds(self, key, pose, ping, logodds, image=None):
        self._b.add_keyframes_logodds([self._s], [key], [pose], ping, [logodds], images=self._images1(ping, image))

    def get_intensity_grid(self):
        return self._b.get_intensity_grid([self._s])[0]

    def update_poses(self, keys, poses):
        self._b.update_poses([self._s] * len(keys), keys, poses)

    def get_occupancy_grid1(self, frames=None, resolution=None):
        return self._b._render([self._s], frames, resolution)[0]

    def get_occupancy_grid2(self, frames=None, resolution=None):
        return self._b.get_occupancy_grid2([self._s], frames, resolution)[0]

    def get_occupancy_grid2_store(self, store, handle, frames=None, resolution=None):
        return self._b.get_occupancy_grid2_store(store, [handle], [self._s], frames, resolution)[0]


class MapBatch(object):
    """S occupancy maps that advance together: every stage of Mapping as one device call over the listed sessions
    (csrc/sfe_map.hip: sfe_mapset).  ``maps[s]`` is, bit for bit, the Mapping that was given session s's calls.

    The settings are Mapping's attributes (keyword arguments, or set afterwards; then ``configure()`` or ``load_yaml()``, as
    with Mapping).  The device arena is sized here and never grows: ``max_keyframes`` keyframes per session of up to
    ``max_pixels`` polar pixels each (the default holds a 1024 x 512 ping at the shipped skips), 20 bytes per pixel (23 with
    the intensity mosaic); one keyframe more, or a larger image, raises.

    With the mosaic on (``pub_intensity=True, intensity_skips="oculus"``) every add takes ``images=``: the listed sessions'
    full-size pings as one host ``uint8 [n x num_ranges x num_bearings]`` array (or a list of such images), or a list of
    ``DeviceImage`` views of pings that already lie on the device, which are sampled in place."""

    def __init__(self, ctx=None, n_sessions=1, max_keyframes=256, max_pixels=1 << 17, **settings):
        if int(n_sessions) < 1 or int(max_keyframes) < 1 or int(max_pixels) < 1:
            raise ValueError("MapBatch: n_sessions, max_keyframes and max_pixels must be positive, got %r, %r, %r"
                             % (n_sessions, max_keyframes, max_pixels))
        self.ctx, self.S = ctx, int(n_sessions)
        self.max_keyframes, self.max_pixels = int(max_keyframes), int(max_pixels)
        proto = Mapping()
        for name in SETTINGS:
            setattr(self, name, getattr(proto, name))
        for name, v in settings.items():
            if name not in SETTINGS:
                raise TypeError("MapBatch: unknown setting %r (Mapping's settings: %s)" % (name, ", ".join(SETTINGS)))
            setattr(self, name, v)
        self.maps = []
        self._h = None
        self._intensity = False         # the intensity mosaic is on (configure)
        self.last_apply_rounds = 0     # apply launches of the last add / update_poses call, as the device counted them

    load_yaml = Mapping.load_yaml

    def configure(self):
        self._intensity = intensity_setting("MapBatch.configure", self.pub_intensity, self.intensity_skips)
        self.close()
        maps = []
        for s in range(self.S):
            v = _SessionMap(self, s)
            for name in SETTINGS:
                setattr(v, name, getattr(self, name))
            v._configure_host()
            maps.append(v)
        if self.ctx is None:
            self.ctx = _L.default_context()
            for v in maps:
                v.ctx = self.ctx
        self._lib = self.ctx.lib
        h = C.c_void_p()
        self.ctx._check(self._lib.sfe_mapset_create(self.ctx.handle, self.S, maps[0].rows, maps[0].cols, self.max_keyframes,
                                                    self.max_pixels, C.byref(h)))
        self._h = h
        if self._intensity:
            self.ctx._check(self._lib.sfe_mapset_enable_intensity(self._h))
        self.maps = maps
        self._geoms = {}
        self._hit_tabs = {}
        # the store feed since configure() / reset(): points fed, points the device left to the host, calls
        self.feed_stats = {"points": 0, "undecided": 0, "calls": 0}

    reset = configure

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._lib.sfe_mapset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_intensity_grid(self, sessions=None):
        """maps[s].get_intensity_grid() for the listed sessions (all by default) -> list of OccupancyGrid, rendered in one
        device call"""
        what = "MapBatch.get_intensity_grid"
        if getattr(self, "_h", None) is None or not getattr(self, "_intensity", False):
            raise NotImplementedError("%s: get_intensity_grid is not implemented for a batch without the intensity grid: "
                                      "configure() with pub_intensity=True and intensity_skips=\"oculus\"" % what)
        sessions = self._listed("get_intensity_grid", range(self.S) if sessions is None else sessions)
        boxes = [self.maps[s]._intensity_box("%s (session %d)" % (what, s)) for s in sessions]
        shapes = [(b[1] - b[0] + 1, b[3] - b[2] + 1) for b in boxes]
        out_off = np.zeros(len(sessions) + 1, np.int64)
        out_off[1:] = np.cumsum([h * w for h, w in shapes])
        occ = np.zeros(max(1, int(out_off[-1])), np.int8)
        i32 = lambda a: np.ascontiguousarray(np.array(a, np.int32).reshape(-1))
        self._check(self._lib.sfe_mapset_render_intensity(
            self._h, len(sessions), _L.ptr(i32(sessions), C.c_int32), _L.ptr(i32(boxes), C.c_int32),
            out_off.ctypes.data_as(C.POINTER(C.c_longlong)), int(out_off[-1]), occ.ctypes.data_as(C.POINTER(C.c_int8))))
        return [self.maps[s]._grid_msg(b, self.maps[s].resolution, occ[out_off[j]:out_off[j + 1]].reshape(shp).copy())
                for j, (s, b, shp) in enumerate(zip(sessions, boxes, shapes))]

    def get_occupancy_grid2(self, sessions=None, frames=None, resolution=None, point_clouds=None):
        """maps[s].get_occupancy_grid2(frames, resolution) for the listed sessions (all by default) -> list of OccupancyGrid,
        rendered in one device call.  ``point_clouds[i]`` replaces the stored cloud of ``sessions[i]`` for this call."""
        if self._h is None:
            raise NotImplementedError("MapBatch.get_occupancy_grid2: get_occupancy_grid2 is not implemented for a batch that "
                                      "was never configured: configure() first")
        sessions = self._listed("get_occupancy_grid2", range(self.S) if sessions is None else sessions,
                                *(() if point_clouds is None else (point_clouds,)))
        views = [self.maps[s] for s in sessions]
        clouds = [v.point_cloud if self.pub_occupancy2 else None for v in views] if point_clouds is None else point_clouds
        for s, v, cloud in zip(sessions, views, clouds):
            v._check_method2("MapBatch.get_occupancy_grid2 (session %d)" % s, cloud)
        points = [np.ascontiguousarray(select_points(np.asarray(c), frames), np.float64) for c in clouds]
        plans = [v._render2_plan(frames, resolution) for v in views]
        i32 = lambda a: np.ascontiguousarray(np.array(a, np.int32).reshape(-1))
        f64 = lambda a: np.ascontiguousarray(np.array(a, np.float64).reshape(-1))
        off = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        slots = np.concatenate([p[0] for p in plans]).astype(np.int32)
        xy = np.concatenate(points) if sum(len(p) for p in points) else np.zeros((1, 2))
        out_off = np.zeros(len(sessions) + 1, np.int64)
        out_off[1:] = np.cumsum([p[3][0] * p[3][1] for p in plans])
        occ = np.zeros(max(1, int(out_off[-1])), np.int8)
        n = len(sessions)
        self._check(self._lib.sfe_mapset_render2(
            self._h, n, _L.ptr(i32(sessions), C.c_int32), _L.ptr(off([len(p[0]) for p in plans]), C.c_int32),
            _L.ptr(slots, C.c_int32), _L.ptr(i32([p[1] for p in plans]), C.c_int32),
            _L.ptr(off([len(p) for p in points]), C.c_int32), _L.ptr(np.ascontiguousarray(xy), C.c_double),
            _L.ptr(i32([v.outlier_filter_min_points > 1 for v in views]), C.c_int32),
            _L.ptr(f64([v.outlier_filter_radius for v in views]), C.c_double),
            _L.ptr(i32([v.outlier_filter_min_points for v in views]), C.c_int32),
            _L.ptr(i32([v.dilate_size // 2 for v in views]), C.c_int32), _L.ptr(f64([p[2] for p in plans]), C.c_double),
            _L.ptr(f64([v.resolution for v in views]), C.c_double), _L.ptr(i32([p[3] for p in plans]), C.c_int32),
            _L.ptr(f64([p[4] for p in plans]), C.c_double), _L.ptr(i32([p[5] for p in plans]), C.c_int32),
            out_off.ctypes.data_as(C.POINTER(C.c_longlong)), occ.ctypes.data_as(C.POINTER(C.c_int8)), int(out_off[-1])))
        return [v._grid_msg(p[1], p[6], occ[out_off[j]:out_off[j + 1]].reshape(p[3]).copy(), p[2])
                for j, (v, p) in enumerate(zip(views, plans))]

    def get_occupancy_grid2_store(self, store, handles, sessions=None, frames=None, resolution=None):
        """maps[s].get_occupancy_grid2_store(store, handles[i], frames, resolution) for s = sessions[i] (all sessions by
        default) -> list of OccupancyGrid, rendered in one device call from the clouds where they lie in ``store`` (a
        CloudStore of this batch's context): ``SessionBatch.slam_clouds()``' handles, or any keyed clouds."""
        what = "get_occupancy_grid2_store"
        if self._h is None:
            raise NotImplementedError("MapBatch.%s: get_occupancy_grid2 is not implemented for a batch that was never "
                                      "configured: configure() first" % what)
        handles = [int(h) for h in np.asarray(handles).reshape(-1)]
        sessions = self._listed(what, range(self.S) if sessions is None else sessions, handles)
        views = [self.maps[s] for s in sessions]
        for s, v in zip(sessions, views):
            v._check_method2("MapBatch.%s (session %d)" % (what, s), ())
        if getattr(store, "ctx", None) is not self.ctx:
            raise ValueError("MapBatch.%s: the store belongs to another context" % what)
        plans = [v._render2_plan(frames, resolution) for v in views]
        i32 = lambda a: np.ascontiguousarray(np.array(a, np.int32).reshape(-1))
        f64 = lambda a: np.ascontiguousarray(np.array(a, np.float64).reshape(-1))
        off = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        slots = np.concatenate([p[0] for p in plans]).astype(np.int32)
        listed = frame_list(frames)
        n = len(sessions)
        lists = np.ascontiguousarray(np.tile(listed, n)) if len(listed) else np.zeros(1, np.int32)
        out_off = np.zeros(n + 1, np.int64)
        out_off[1:] = np.cumsum([p[3][0] * p[3][1] for p in plans])
        occ = np.zeros(max(1, int(out_off[-1])), np.int8)
        self._check(self._lib.sfe_mapset_render2_store(
            self._h, store.handle, n, _L.ptr(i32(sessions), C.c_int32), _L.ptr(off([len(p[0]) for p in plans]), C.c_int32),
            _L.ptr(slots, C.c_int32), _L.ptr(i32([p[1] for p in plans]), C.c_int32), _L.ptr(i32(handles), C.c_int32),
            _L.ptr(i32([frames is None] * n), C.c_int32), _L.ptr(off([len(listed)] * n), C.c_int32), _L.ptr(lists, C.c_int32),
            _L.ptr(i32([v.outlier_filter_min_points > 1 for v in views]), C.c_int32),
            _L.ptr(f64([v.outlier_filter_radius for v in views]), C.c_double),
            _L.ptr(i32([v.outlier_filter_min_points for v in views]), C.c_int32),
            _L.ptr(i32([v.dilate_size // 2 for v in views]), C.c_int32), _L.ptr(f64([p[2] for p in plans]), C.c_double),
            _L.ptr(f64([v.resolution for v in views]), C.c_double), _L.ptr(i32([p[3] for p in plans]), C.c_int32),
            _L.ptr(f64([p[4] for p in plans]), C.c_double), _L.ptr(i32([p[5] for p in plans]), C.c_int32),
            out_off.ctypes.data_as(C.POINTER(C.c_longlong)), occ.ctypes.data_as(C.POINTER(C.c_int8)), int(out_off[-1])))
        return [v._grid_msg(p[1], p[6], occ[out_off[j]:out_off[j + 1]].reshape(p[3]).copy(), p[2])
                for j, (v, p) in enumerate(zip(views, plans))]

    # ---- helpers -----------------------------------------------------------------------------------------------------
    def _check(self, rc):
        return self.ctx._check(rc)

    def _geometry(self, sonar_xy, shape):
        """equal sonar_xy tables are stored once"""
        import hashlib
        key = (tuple(shape), hashlib.sha256(sonar_xy.tobytes()).digest())
        if key not in self._geoms:
            gid = C.c_int(0)
            self._check(self._lib.sfe_mapset_geometry(self._h, _L.ptr(sonar_xy, C.c_float), shape[0], shape[1], C.byref(gid)))
            self._geoms[key] = gid.value
        return self._geoms[key]

    def _listed(self, what, sessions, *per_session):
        if self._h is None:
            raise RuntimeError("MapBatch.%s: configure() first" % what)
        sessions = [int(s) for s in sessions]
        for a in per_session:
            if len(a) != len(sessions):
                raise ValueError("MapBatch.%s: %d sessions but a list of %d" % (what, len(sessions), len(a)))
        if len(set(sessions)) != len(sessions):
            raise ValueError("MapBatch.%s: a session is listed twice" % what)
        for s in sessions:
            if not 0 <= s < self.S:
                raise IndexError("MapBatch.%s: session %d of %d" % (what, s, self.S))
        return sessions

    def _begin(self, what, sessions, keys, poses, pings, data, images=None):
        """the checks of an add call, before anything changes -> (sessions, pings, new keyframes)"""
        sessions = self._listed(what, sessions, keys, poses, data)
        if self._intensity and images is None:
            raise ValueError("MapBatch.%s: pub_intensity is on, so the add needs images= (the listed sessions' pings)" % what)
        if not self._intensity and images is not None:
            raise ValueError("MapBatch.%s: images= without the intensity mosaic (pub_intensity with intensity_skips)" % what)
        if images is not None and len(images) != len(sessions):
            raise ValueError("MapBatch.%s: %d sessions but %d images" % (what, len(sessions), len(images)))
        if isinstance(pings, (list, tuple)):
            if len(pings) != len(sessions):
                raise ValueError("MapBatch.%s: %d sessions but %d pings" % (what, len(sessions), len(pings)))
        else:
            pings = [pings] * len(sessions)
        for s in sessions:
            self.maps[s]._check_supported()
            if self.maps[s]._n_slots >= self.max_keyframes:
                raise _L.SonarFEError("MapBatch.%s: session %d already holds max_keyframes = %d keyframes"
                                      % (what, s, self.max_keyframes))
        return sessions, pings

    @contextlib.contextmanager
    def _geometry_guard(self, sessions):
        """a refused add leaves the listed sessions' geometry state (sonar settings, skips, image size, geometry id) as it
        found it: _new_keyframe takes a ping's geometry before the device can refuse the image or the slot"""
        keep = [(self.maps[s], self.maps[s]._geometry_state()) for s in sessions]
        try:
            yield
        except BaseException:
            for v, state in keep:
                v._restore_geometry(state)
            raise

    def _images(self, what, sessions, pings, images):
        """the checks of an add's images=, after the listed sessions took their pings' geometry -> what _set_images takes:
        None (mosaic off), ("dev", views) or ("host", contiguous uint8 images)"""
        if not self._intensity:
            return None
        if all(isinstance(im, DeviceImage) for im in images):
            for s, im in zip(sessions, images):
                o = self.maps[s].oculus
                if im.shape != (int(o.num_ranges), int(o.num_bearings)):
                    raise ValueError("MapBatch.%s: session %d's device image is %r, its ping's geometry says %r (num_ranges x "
                                     "num_bearings)" % (what, s, im.shape, (int(o.num_ranges), int(o.num_bearings))))
            return "dev", list(images)
        if any(isinstance(im, DeviceImage) for im in images):
            raise ValueError("MapBatch.%s: images= mixes device views and host images" % what)
        return "host", [ping_image("MapBatch.%s (session %d)" % (what, s), ping, im, self.maps[s].oculus)
                        for s, ping, im in zip(sessions, pings, images)]

    def _set_images(self, sessions, kfs, images):
        if images is None:
            return
        kind, imgs = images
        i32 = lambda a: np.ascontiguousarray(np.array(a, np.int32).reshape(-1))
        views = [self.maps[s] for s in sessions]
        shape4 = i32([[im.shape[0], im.shape[1], int(v.oculus_r_skip), int(v.oculus_c_skip)] for v, im in zip(views, imgs)])
        head = (self._h, len(sessions), _L.ptr(i32(sessions), C.c_int32), _L.ptr(i32([kf._slot for kf in kfs]), C.c_int32),
                _L.ptr(i32([kf.geom for kf in kfs]), C.c_int32), _L.ptr(shape4, C.c_int32))
        if kind == "dev":
            ptrs = (C.c_void_p * len(imgs))(*[im.ptr.value for im in imgs])
            strides = np.array([im.stride for im in imgs], np.int64)
            self._check(self._lib.sfe_mapset_set_intensity_dev(*head, ptrs, strides.ctypes.data_as(C.POINTER(C.c_longlong))))
        else:
            flat = np.ascontiguousarray(np.concatenate([im.ravel() for im in imgs]))
            with self.ctx.lock:        # the context's pinned staging
                self._check(self._lib.sfe_mapset_set_intensity(*head, _L.ptr(flat, C.c_uint8)))

    def _end(self, sessions, keys, kfs):
        before = self._apply_launches()
        self._fit_many([(s, [(kf, kf.pose)]) for s, kf in zip(sessions, kfs)], dec=False)
        self.last_apply_rounds = self._apply_launches() - before
        for s, key, kf in zip(sessions, keys, kfs):
            v = self.maps[s]
            v._append(key, kf)
            v._n_slots += 1

    # ---- the stages --------------------------------------------------------------------------------------------------
    def add_keyframes(self, sessions, keys, poses, pings, points, images=None):
        """Mapping.add_keyframe for each listed session: ``pings`` one ping for all or one per session, ``points[i]`` the
        cloud of ``sessions[i]``, ``images[i]`` its ping's image (with the intensity mosaic, and only then)"""
        sessions, pings = self._begin("add_keyframes", sessions, keys, poses, pings, points, images)
        with self._geometry_guard(sessions):
            kfs = [self.maps[s]._new_keyframe(pose, ping) for s, pose, ping in zip(sessions, poses, pings)]
            images = self._images("add_keyframes", sessions, pings, images)
            self._measure_many(sessions, kfs, points)
            self._set_images(sessions, kfs, images)
        for v in self.maps:
            v._meas_job = -1
        for j, (s, p) in enumerate(zip(sessions, points)):
            self.maps[s]._meas_job = j
            if self.pub_occupancy2:
                self.maps[s].point_cloud = p
        self._end(sessions, keys, kfs)

    def _measure_many(self, sessions, kfs, points):
        clouds = [np.asarray(p) if len(p) else p for p in points]
        hits = self._hits_many(sessions, clouds)
        all_hits = [_hits32(h, hr) for h, hr, _ in hits]
        hit_off = np.cumsum([0] + [len(h) for h in all_hits])
        hits_all = np.ascontiguousarray(np.concatenate(all_hits)) if hit_off[-1] else np.zeros(2, np.int32)
        self._check(self._lib.sfe_mapset_measure(
            self._h, len(sessions), _i32p(sessions), _i32p([kf._slot for kf in kfs]), _i32p([kf.geom for kf in kfs]),
            _i32p(hit_off), _L.ptr(hits_all, C.c_int32),
            *kernel_tables(self, [self.maps[s] for s in sessions], [(hr, hc) for _, hr, hc in hits])))

    def add_keyframes_store(self, sessions, keys, poses, pings, store, handles, images=None):
        """``add_keyframes(sessions, keys, poses, pings, store.read_many(handles))``, bit for bit, without the clouds
        leaving the device: the outlier filter, the hit cells and the measurement of every listed session run from the
        store's pool (``store``: a CloudStore of this batch's context, ``handles[i]`` the cloud of ``sessions[i]``).

        The device decides a point's bearing column only inside a guard band (``guard_margin``); the few points it leaves
        undecided come back and go through ``_hit_indices`` here (``feed_stats`` counts them).  With ``pub_occupancy2``,
        ``maps[s].point_cloud`` is read from the store on access: the handle must still be live then."""
        handles = [int(h) for h in np.asarray(handles).reshape(-1)]
        sessions, pings = self._begin("add_keyframes_store", sessions, keys, poses, pings, handles, images)
        if getattr(store, "ctx", None) is not self.ctx:
            raise ValueError("MapBatch.add_keyframes_store: the store belongs to another context")
        with self._geometry_guard(sessions):
            kfs = [self.maps[s]._new_keyframe(pose, ping) for s, pose, ping in zip(sessions, poses, pings)]
            images = self._images("add_keyframes_store", sessions, pings, images)
            self._measure_store(sessions, kfs, store, handles)
            self._set_images(sessions, kfs, images)
        for v in self.maps:
            v._meas_job = -1
        for j, (s, h) in enumerate(zip(sessions, handles)):
            self.maps[s]._meas_job = j
            if self.pub_occupancy2:
                self.maps[s]._cloud_ref = (store, h)
        self._end(sessions, keys, kfs)

    def _hit_table(self, v):
        """the device's copy of what _hit_indices reads of session map v's sonar geometry, stored once per geometry"""
        return device_hit_table(v, self._hit_tabs, lambda *a: self._lib.sfe_mapset_hit_table(self._h, *a))

    def _measure_store(self, sessions, kfs, store, handles):
        views = [self.maps[s] for s in sessions]
        head = (store.handle, len(sessions), _i32p(sessions), _i32p([kf._slot for kf in kfs]), _i32p([kf.geom for kf in kfs]),
                _i32p(handles), _i32p([self._hit_table(v) for v in views]), float(self.outlier_filter_radius),
                int(self.outlier_filter_min_points))
        measure_store(self, views, functools.partial(self._lib.sfe_mapset_measure_store, self._h, *head),
                      functools.partial(self._lib.sfe_mapset_measure_store_undecided, self._h),
                      functools.partial(self._lib.sfe_mapset_measure_store_finish, self._h))

    def add_keyframes_logodds(self, sessions, keys, poses, pings, logodds, images=None):
        """Mapping.add_keyframe_logodds for each listed session"""
        sessions, pings = self._begin("add_keyframes_logodds", sessions, keys, poses, pings, logodds, images)
        with self._geometry_guard(sessions):
            kfs = [self.maps[s]._new_keyframe(pose, ping) for s, pose, ping in zip(sessions, poses, pings)]
            images = self._images("add_keyframes_logodds", sessions, pings, images)
            los = []
            for s, lo in zip(sessions, logodds):
                lo = np.ascontiguousarray(lo, np.float32).ravel()
                size = self.maps[s].oculus_image_size
                if lo.size != int(np.prod(size)):
                    raise ValueError("add_keyframes_logodds: %d values for session %d's %r image" % (lo.size, s, size))
                los.append(lo)
            i32 = lambda a: np.ascontiguousarray(np.array(a, np.int32))
            self._check(self._lib.sfe_mapset_set_logodds(
                self._h, len(sessions), _L.ptr(i32(sessions), C.c_int32), _L.ptr(i32([kf._slot for kf in kfs]), C.c_int32),
                _L.ptr(i32([kf.geom for kf in kfs]), C.c_int32), _L.ptr(np.ascontiguousarray(np.concatenate(los)), C.c_float)))
            self._set_images(sessions, kfs, images)
        self._end(sessions, keys, kfs)

    def _hits_many(self, sessions, clouds):
        """Mapping._hits for every listed session: the outlier filter of all clouds in one device call, then the hit indices
        (elementwise in the points) once per group of sessions that share a sonar geometry -> [(hits, hr, hc)]"""
        out = [None] * len(sessions)
        live = [i for i, c in enumerate(clouds) if len(c)] if self.pub_occupancy1 else []     # (Mapping._hits)
        for i in range(len(sessions)):
            if i not in live:
                out[i] = (None, -1, 0)
        pts = {i: clouds[i] for i in live}
        if live and self.outlier_filter_min_points > 1:
            pts = {i: pcl._cloud(clouds[i][:, :2], "add_keyframes(points)") for i in live}
            off = np.zeros(len(live) + 1, np.int32)
            off[1:] = np.cumsum([len(pts[i]) for i in live])
            cat = np.ascontiguousarray(np.concatenate([pts[i] for i in live]))
            keep = np.zeros(len(cat), np.uint8)
            with self.ctx.lock:        # the context's shared scratch, as pcl.remove_outlier
                self._check(self._lib.sfe_remove_outlier_many(
                    self.ctx.handle, _L.ptr(cat, C.c_float), _L.ptr(off, C.c_int32), len(live),
                    float(self.outlier_filter_radius), int(self.outlier_filter_min_points), _L.ptr(keep, C.c_uint8)))
            keep = keep.astype(bool)
            pts = {i: cat[off[j]:off[j + 1]][keep[off[j]:off[j + 1]]] for j, i in enumerate(live)}
        groups = {}
        for i in live:
            groups.setdefault((self.maps[sessions[i]]._hit_key, pts[i].dtype.str, pts[i].shape[1]), []).append(i)
        for idx in groups.values():
            v = self.maps[sessions[idx[0]]]
            hits, hr, hc = v._hit_indices(np.concatenate([pts[i] for i in idx]) if len(idx) > 1 else pts[idx[0]])
            at = 0
            for i in idx:
                out[i] = (hits[at:at + len(pts[i])], hr, hc)
                at += len(pts[i])
        return out

    def update_poses(self, sessions, keys, poses):
        """for s, k, p in zip(sessions, keys, poses): maps[s].update_pose(k, p) -- the same bits; the fits of all sessions in
        one pass, their ordered applies in rounds"""
        if self._h is None:
            raise RuntimeError("MapBatch.update_poses: configure() first")
        for s in sessions:
            if not 0 <= int(s) < self.S:
                raise IndexError("MapBatch.update_poses: session %d of %d" % (s, self.S))
        waves = plan_updates([v.keyframes for v in self.maps], [v.pose_changed for v in self.maps], sessions, keys, poses)
        before = self._apply_launches()
        for wave in waves:
            self._fit_many(wave, dec=True)
        self.last_apply_rounds = self._apply_launches() - before

    def _bounds(self, maps, slots, pose4, origin):
        n = len(slots)
        mm = np.zeros((n, 4), np.int32)
        self._check(self._lib.sfe_mapset_fit_bounds(self._h, n, _L.ptr(np.ascontiguousarray(maps), C.c_int32),
                                                    _L.ptr(np.ascontiguousarray(slots), C.c_int32),
                                                    _L.ptr(np.ascontiguousarray(pose4), C.c_double),
                                                    _L.ptr(np.ascontiguousarray(origin), C.c_double), float(self.resolution),
                                                    _L.ptr(mm, C.c_int32)))
        return mm.astype(np.int64)

    def _apply_launches(self):
        n = C.c_longlong(0)
        self._check(self._lib.sfe_mapset_apply_launches(self._h, C.byref(n)))
        return n.value

    def _fit_many(self, wave, dec):
        """Mapping._fit for one group per session: [(session, [(keyframe, pose) in order])], every session at most once"""
        wave = [(s, g) for s, g in wave if g]
        if not wave:
            return
        n = sum(len(g) for _, g in wave)
        maps, slots = np.zeros(n, np.int32), np.zeros(n, np.int32)
        pose4, origin = np.zeros((n, 4), np.float64), np.zeros((n, 2), np.float64)
        spans, a = [], 0
        for s, group in wave:
            v = self.maps[s]
            for i, (kf, pose) in enumerate(group):
                yaw = pose.theta()
                maps[a + i], slots[a + i] = s, kf._slot
                pose4[a + i] = np.cos(yaw), np.sin(yaw), pose.x(), pose.y()
            origin[a:a + len(group)] = v.y0, v.x0
            spans.append((a, a + len(group)))
            a += len(group)
        mm = self._bounds(maps, slots, pose4, origin)
        shift = np.zeros((n, 2), np.int64)
        grows = [[0, 0, 0, 0] for _ in wave]
        # adjust_bounds per session; the sessions whose origin moved in the middle of their group take their remaining bounds
        # again, all of them in one call per pass
        at = [lo for lo, _ in spans]
        while True:
            again = []
            for w, ((s, _), (lo, hi)) in enumerate(zip(wave, spans)):
                if at[w] < hi:
                    at[w] = lo + self.maps[s]._adjust(mm[lo:hi], shift[lo:hi], grows[w], origin[lo:hi], at[w] - lo)
                    if at[w] < hi:
                        again.append(np.arange(at[w], hi))
            if not again:
                break
            idx = np.concatenate(again)
            mm[idx] = self._bounds(maps[idx], slots[idx], pose4[idx], origin[idx])
        grown = [w for w, g in enumerate(grows) if any(g)]
        if grown:
            self._check(self._lib.sfe_mapset_grow(
                self._h, len(grown), _L.ptr(np.array([wave[w][0] for w in grown], np.int32), C.c_int32),
                _L.ptr(np.ascontiguousarray(np.array([grows[w] for w in grown], np.int32)), C.c_int32)))
            for w in grown:
                v = self.maps[wave[w][0]]
                v._grow[0] += grows[w][0]
                v._grow[1] += grows[w][2]
        mm32 = np.ascontiguousarray(mm, np.int32)
        shift32 = np.ascontiguousarray(shift, np.int32)
        decs = np.full(n, 1 if dec else 0, np.uint8)
        self._check(self._lib.sfe_mapset_refit(self._h, n, _L.ptr(maps, C.c_int32), _L.ptr(slots, C.c_int32),
                                               _L.ptr(pose4, C.c_double), _L.ptr(origin, C.c_double), float(self.resolution),
                                               _L.ptr(mm32, C.c_int32), _L.ptr(shift32, C.c_int32), _L.ptr(decs, C.c_uint8)))
        for (s, group), (lo, hi) in zip(wave, spans):
            self.maps[s]._fitted([kf for kf, _ in group], mm[lo:hi], shift[lo:hi])

    def get_occupancy_grids(self, sessions=None, frames=None, resolution=None):
        """maps[s].get_occupancy_grid(frames, resolution) for the listed sessions (all by default) -> list of OccupancyGrid,
        rendered in one device call"""
        if self.pub_occupancy1:
            return self._render(range(self.S) if sessions is None else sessions, frames, resolution)
        if self.pub_occupancy2:
            return self.get_occupancy_grid2(sessions, frames, resolution)
        return [None] * (self.S if sessions is None else len(sessions))

    def _render(self, sessions, frames, resolution):
        sessions = self._listed("get_occupancy_grids", sessions)
        plans = [self.maps[s]._render_plan(frames, resolution) for s in sessions]
        i32 = lambda a: np.ascontiguousarray(np.array(a, np.int32))
        if frames is not None:
            off = np.zeros(len(sessions) + 1, np.int32)
            off[1:] = np.cumsum([len(p[1]) for p in plans])
            slots = np.ascontiguousarray(np.concatenate([p[1] for p in plans]), np.int32) if off[-1] else i32([0])
            self._check(self._lib.sfe_mapset_frames(self._h, len(sessions), _L.ptr(i32(sessions), C.c_int32),
                                                    _L.ptr(off, C.c_int32), _L.ptr(slots, C.c_int32)))
        sizes = [p[3][0] * p[3][1] for p in plans]
        out_off = np.zeros(len(sessions) + 1, np.int64)
        out_off[1:] = np.cumsum(sizes)
        occ = np.zeros(int(out_off[-1]), np.int8)
        if len(occ):
            self._check(self._lib.sfe_mapset_render(
                self._h, len(sessions), _L.ptr(i32(sessions), C.c_int32), _L.ptr(i32([p[0] for p in plans]), C.c_int32),
                _L.ptr(i32([p[2] for p in plans]), C.c_int32), _L.ptr(i32([p[3] for p in plans]), C.c_int32),
                _L.ptr(np.ascontiguousarray(np.array([p[4] for p in plans], np.float64)), C.c_double),
                _L.ptr(i32([p[5] for p in plans]), C.c_int32), out_off.ctypes.data_as(C.POINTER(C.c_longlong)),
                occ.ctypes.data_as(C.POINTER(C.c_int8)), len(occ)))
        return [self.maps[s]._grid_msg(p[2], p[6], occ[out_off[j]:out_off[j + 1]].reshape(p[3]).copy())
                for j, (s, p) in enumerate(zip(sessions, plans))]
