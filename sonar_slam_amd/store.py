"""Device-resident keyframe clouds (``sfe_cloud_store``, include/sonarfe.h): SURVEY 8 row f4.

The reference moves every feature cloud through a ROS topic and rebuilds the scan matcher's inputs in
numpy (feature_extraction.py:175-193 -> slam_ros.py:169-170 -> slam.py:229-292, slam_objects.py:178-198).
Here the clouds stay in HBM from the feature extractor to the scan matcher: a cloud is named by an
integer handle; ``get_points`` (transform + concatenate + pcl.downsample), ``icp`` and ``overlap`` take
handles; the host sees sizes (a few bytes per cloud) and results, and the points only when it asks
(``read``: the PointCloud2 for rviz / the mapping node).

``CloudStore3`` (``sfe_cloud_store3``) is the same for the N x 3 clouds a keyframe carries (``Keyframe.points3D``,
slam_objects.py:101-106, 200-223): ``put``, ``get_points``, ``icp`` and ``overlap`` over handles, with 4 x 4 transforms, and
the keyed clouds of the loop-closure search (``get_points_keys``, ``fov_select``, ``compact_selected``, ``match_keys``).
"""
import ctypes as _C

import numpy as np

from . import _lib as _L
from . import icp_config as _cfg

NEGATE_Y = 1        # SFE_STORE_NEGATE_Y: store (x, -y), what slam_ros.py:170 makes of the feature message
F32_POINTS = 2      # SFE_STORE_F32_POINTS: transform like numpy does for float32 keyframe clouds (sgemm)


def pose_T6(pose_or_matrix):
    """The six float32 numbers Keyframe.transform_points reads from ``pose.matrix().astype(np.float32)``
    (slam_objects.py:192-195): T00 T01 T02 T10 T11 T12."""
    M = pose_or_matrix.matrix() if hasattr(pose_or_matrix, "matrix") else pose_or_matrix
    return np.asarray(M, np.float64).astype(np.float32)[:2, :3].reshape(6)


class CloudStore(object):
    def __init__(self, ctx=None, capacity_points=1 << 22, max_clouds=1 << 16):
        self.ctx = ctx or _L.default_context()
        h = _C.c_void_p()
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_create(self.ctx.handle, int(capacity_points), int(max_clouds),
                                                                _C.byref(h)))
        self.handle = h
        self.capacity_points, self.max_clouds = int(capacity_points), int(max_clouds)

    # -- filling --
    def put(self, points, stamp=0):
        """one host cloud (N x 2, rounded to float32 like the pybind boundary) -> handle"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        h = _C.c_int32(-1)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_put(self.ctx.handle, self.handle, int(stamp),
                                                             _L.ptr(pts, _C.c_float), len(pts), _C.byref(h)))
        return h.value

    def put_keys(self, points, keys, stamp=0):
        """``put`` with a key per point (integers in [0, 2^31)): a keyed cloud, as ``get_points_keys`` leaves one -> handle.
        For a cloud that arrives already keyed, such as the SLAM cloud a mapping node receives: ``put_keys(cloud[:, :2],
        cloud[:, 3])``; ``read_keys`` reads the keys back."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        wide = np.asarray(keys).reshape(-1)
        if len(wide) != len(pts):
            raise ValueError("CloudStore.put_keys: %d points but %d keys" % (len(pts), len(wide)))
        if len(wide) and not (np.all(wide >= 0) and np.all(wide < 2 ** 31) and np.all(wide == np.floor(wide))):
            raise ValueError("CloudStore.put_keys: keys must be integers in [0, 2^31)")
        ks = np.ascontiguousarray(wide, np.int32)
        h = _C.c_int32(-1)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_put_keys(self.ctx.handle, self.handle, int(stamp),
                                                                  _L.ptr(pts, _C.c_float), _L.ptr(ks, _C.c_int32), len(pts),
                                                                  _C.byref(h)))
        return h.value

    def put_batch_dev(self, d_clouds, d_counts, n_frames, cap, stamps=None, flags=0):
        """n_frames clouds straight from the resident cloud filter's outputs (device buffers) -> handles"""
        handles = np.zeros(n_frames, np.int32)
        st = None if stamps is None else np.ascontiguousarray(stamps, np.int64)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_put_batch_dev(
                self.ctx.handle, self.handle, None if st is None else _L.ptr(st, _C.c_int64), d_clouds.ptr, d_counts.ptr,
                int(n_frames), int(cap), int(flags), _L.ptr(handles, _C.c_int32)))
        return handles

    # -- bookkeeping --
    def __len__(self):
        return int(self.ctx.lib.sfe_cloud_store_count(self.handle))

    def meta(self, first=0, n=None):
        """-> (stamps int64, offsets int64, counts int32) of clouds first .. first + n - 1"""
        n = len(self) - first if n is None else int(n)
        st, off, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_meta(self.ctx.handle, self.handle, int(first), n,
                                                              _L.ptr(st, _C.c_int64), _L.ptr(off, _C.c_int64),
                                                              _L.ptr(cnt, _C.c_int32)))
        return st, off, cnt

    def counts(self, handles):
        handles = np.asarray(handles, np.int64).reshape(-1)
        if len(handles) == 0:
            return np.zeros(0, np.int32)
        lo, hi = int(handles.min()), int(handles.max())
        return self.meta(lo, hi - lo + 1)[2][handles - lo]

    def read(self, handle):
        """the points of one cloud (N x 2 float32), copied to the host"""
        n = int(self.counts([handle])[0])
        out = np.zeros((max(n, 0), 2), np.float32)
        m = _C.c_int(0)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_read(self.ctx.handle, self.handle, int(handle),
                                                              _L.ptr(out, _C.c_float), len(out), _C.byref(m)))
        if m.value < 0:
            raise _L.SonarFEError("cloud %d was not stored (count %d: -1 octree too deep, -3 pool full)" % (handle, m.value))
        return out

    def read_many(self, handles):
        """the points of many clouds in one call (a copy per cloud, one final synchronisation) -> list of N x 2 float32 arrays"""
        handles = np.ascontiguousarray(handles, np.int32).reshape(-1)
        counts = self.counts(handles)
        bad = np.nonzero(counts < 0)[0]
        if len(bad):
            raise _L.SonarFEError("cloud %d was not stored (count %d: -1 octree too deep, -3 pool full)"
                                  % (handles[bad[0]], counts[bad[0]]))
        out = np.zeros((int(counts.sum()), 2), np.float32)
        got = np.zeros(len(handles), np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_read_many(self.ctx.handle, self.handle, _L.ptr(handles, _C.c_int32),
                                                                   len(handles), _L.ptr(out, _C.c_float), len(out),
                                                                   _L.ptr(got, _C.c_int32)))
        ends = np.cumsum(got)
        return [out[e - c:e].copy() for e, c in zip(ends, got)]

    def truncate(self, n_slots):
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_truncate(self.ctx.handle, self.handle, int(n_slots)))

    # -- the SLAM node's three uses of a keyframe cloud --
    def get_points(self, handles, T6, resolution, flags=0, stamps=None):
        """SLAM.get_points(frames, ref_frame) for many targets at once: handles [n_jobs x m] (-1 = unused),
        T6 [n_jobs x m x 6] (``pose_T6`` of ref_pose.between(pose)) -> new handles [n_jobs]"""
        handles = np.ascontiguousarray(handles, np.int32)
        if handles.ndim == 1:
            handles = handles[None, :]
        n_jobs, m = handles.shape
        T6 = np.ascontiguousarray(T6, np.float32).reshape(n_jobs, m, 6)
        out = np.zeros(n_jobs, np.int32)
        st = None if stamps is None else np.ascontiguousarray(stamps, np.int64)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_get_points(
                self.ctx.handle, self.handle, _L.ptr(handles, _C.c_int32), _L.ptr(T6, _C.c_float), n_jobs, m,
                float(resolution), int(flags), None if st is None else _L.ptr(st, _C.c_int64), _L.ptr(out, _C.c_int32)))
        return out

    def icp(self, params_or_chain, pairs, guesses):
        """SLAM.compute_icp over handles: pairs [n x 2] = (source, target), guesses [n x 3 x 3]
        -> (T [n x 3 x 3] float32, status [n], iterations [n]).

        ``params_or_chain``: an ``IcpParams``, or an ``icp_config.IcpChain`` -- its data-point filters then run on the
        stored clouds in place (every distinct handle of a side once per call) and its outlier filters / checker inside
        the ICP loop, bit for bit what ``pcl.ICP`` with ``setChain`` computes on the same clouds (statuses 7, 8 and 9
        included).  A chain with neither is its ``params``."""
        chain = None
        if isinstance(params_or_chain, _cfg.IcpChain):
            chain, params = params_or_chain, params_or_chain.params
        else:
            params = params_or_chain
        if not isinstance(params, _L.IcpParams):
            raise TypeError("CloudStore.icp: expected an IcpParams or an icp_config.IcpChain, got %s"
                            % type(params_or_chain).__name__)
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        g = np.ascontiguousarray(np.asarray(guesses, np.float32).reshape(n, 9))
        T, st, it = np.zeros((n, 3, 3), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        with self.ctx.lock:
            if chain is None or not chain.has_modules():
                self.ctx._check(self.ctx.lib.sfe_icp_store_compute(
                    self.ctx.handle, _C.byref(params), self.handle, _L.ptr(pairs, _C.c_int32), _L.ptr(g, _C.c_float), n,
                    _L.ptr(T, _C.c_float), _L.ptr(st, _C.c_int32), _L.ptr(it, _C.c_int32)))
            else:
                rd, n_rd = chain.device_stages(chain.reading)
                rf, n_rf = chain.device_stages(chain.reference)
                ox = _C.byref(chain.outliers) if chain.outliers.any() else None
                self.ctx._check(self.ctx.lib.sfe_icp_store_compute_chain_ext(
                    self.ctx.handle, _C.byref(params), ox, rd, n_rd, rf, n_rf, self.handle, _L.ptr(pairs, _C.c_int32),
                    _L.ptr(g, _C.c_float), n, _L.ptr(T, _C.c_float), _L.ptr(st, _C.c_int32), _L.ptr(it, _C.c_int32)))
        return T, st, it

    def overlap(self, pairs, T6, max_dist, flags=0):
        """SLAM.get_overlap for many (source, target) pairs -> matched source points per pair"""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        T6 = np.ascontiguousarray(T6, np.float32).reshape(n, 6)
        out = np.zeros(n, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_overlap(
                self.ctx.handle, self.handle, _L.ptr(pairs, _C.c_int32), _L.ptr(T6, _C.c_float), n, float(max_dist),
                int(flags), _L.ptr(out, _C.c_int32)))
        return out

    # -- the loop-closure search (slam.py:839-1001) --
    def bbox(self, handles):
        """-> [n x 4] float32 (min x, min y, max x, max y) of the named clouds"""
        h = np.ascontiguousarray(handles, np.int32).reshape(-1)
        out = np.zeros((len(h), 4), np.float32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_bbox(self.ctx.handle, self.handle, _L.ptr(h, _C.c_int32), len(h),
                                                              _L.ptr(out, _C.c_float)))
        return out

    def get_points_keys(self, handles, T6, keys, resolution, flags=0, stamp=0):
        """SLAM.get_points(frames, None, return_keys=True) (slam.py:873): cloud k under T6[k] (its pose's matrix) tagged
        keys[k]; the descriptor overload of pcl.downsample.  Any size.  -> the new handle (its keys: ``read_keys``)"""
        handles = np.ascontiguousarray(handles, np.int32).reshape(-1)
        m = len(handles)
        T6 = np.ascontiguousarray(T6, np.float32).reshape(m, 6)
        keys = np.ascontiguousarray(keys, np.int32).reshape(m)
        out = _C.c_int32(-1)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_get_points_keys(
                self.ctx.handle, self.handle, _L.ptr(handles, _C.c_int32), _L.ptr(T6, _C.c_float), _L.ptr(keys, _C.c_int32), m,
                float(resolution), int(flags), int(stamp), _C.byref(out)))
        return out.value

    def read_keys(self, handle):
        n = int(self.counts([handle])[0])
        out = np.zeros(max(n, 0), np.int32)
        m = _C.c_int(0)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_read_keys(self.ctx.handle, self.handle, int(handle),
                                                                   _L.ptr(out, _C.c_int32), len(out), _C.byref(m)))
        return out

    def fov_select(self, handle, Tinv6, range_bounds, bearing_bounds, n_keys):
        """the field-of-view gate of slam.py:875-899 on a keyed cloud -> (per-key counts of the selected points [n_keys],
        number selected, number the device could not decide: then ``set_selection``)"""
        Tinv6 = np.ascontiguousarray(Tinv6, np.float32).reshape(-1, 6)
        rb = np.ascontiguousarray(range_bounds, np.float64).reshape(-1)
        bb = np.ascontiguousarray(bearing_bounds, np.float64).reshape(-1)
        assert len(rb) == len(bb) == len(Tinv6)
        hist = np.zeros(int(n_keys), np.int32)
        n_sel, n_amb = _C.c_int32(0), _C.c_int32(0)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_fov_select(
                self.ctx.handle, self.handle, int(handle), _L.ptr(Tinv6, _C.c_float), _L.ptr(rb, _C.c_double),
                _L.ptr(bb, _C.c_double), len(Tinv6), int(n_keys), _L.ptr(hist, _C.c_int32), _C.byref(n_sel), _C.byref(n_amb)))
        return hist, n_sel.value, n_amb.value

    def set_selection(self, handle, sel):
        sel = np.ascontiguousarray(sel, np.uint8).reshape(-1)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_set_selection(self.ctx.handle, self.handle, int(handle),
                                                                       _L.ptr(sel, _C.c_uint8), len(sel)))

    def compact_selected(self, handle, stamp=0):
        """target_points[sel], target_keys[sel] (slam.py:898-899) -> new keyed handle"""
        out = _C.c_int32(-1)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_compact_selected(self.ctx.handle, self.handle, int(handle), int(stamp),
                                                                          _C.byref(out)))
        return out.value

    def match_keys(self, source, T6, target, max_dist, n_keys, flags=0):
        """slam.py:977-985 -> (per-key counts of the matched targets [n_keys], overlap)"""
        T6 = np.ascontiguousarray(T6, np.float32).reshape(6)
        hist = np.zeros(int(n_keys), np.int32)
        ov = _C.c_int32(0)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_match_keys(
                self.ctx.handle, self.handle, int(source), _L.ptr(T6, _C.c_float), int(target), float(max_dist), int(flags),
                int(n_keys), _L.ptr(hist, _C.c_int32), _C.byref(ov)))
        return hist, ov.value

    # -- the same for many clouds at once (chained.SessionBatch: the search of every session in lock-step) --
    def get_points_keys_many(self, handles, T6, keys, resolution, flags=0, stamps=None):
        """``get_points_keys`` for n_jobs keyed targets in one call: handles / T6 / keys are lists (one entry per job) of
        what ``get_points_keys`` takes -> new handles [n_jobs]"""
        n_jobs = len(handles)
        m = np.array([len(h) for h in handles], np.int32)
        off = np.ascontiguousarray(np.r_[0, np.cumsum(m)], np.int32)
        hs = np.ascontiguousarray(np.concatenate([np.asarray(h, np.int32).reshape(-1) for h in handles]) if n_jobs else
                                  np.zeros(0), np.int32)
        T = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float32).reshape(-1, 6) for t in T6]) if n_jobs else
                                 np.zeros((0, 6)), np.float32).reshape(-1, 6)
        ks = np.ascontiguousarray(np.concatenate([np.asarray(k, np.int32).reshape(-1) for k in keys]) if n_jobs else
                                  np.zeros(0), np.int32)
        assert len(hs) == len(T) == len(ks) == off[-1]
        st = None if stamps is None else np.ascontiguousarray(stamps, np.int64).reshape(n_jobs)
        out = np.full(n_jobs, -1, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_get_points_keys_many(
                self.ctx.handle, self.handle, _L.ptr(hs, _C.c_int32), _L.ptr(T, _C.c_float), _L.ptr(ks, _C.c_int32),
                _L.ptr(off, _C.c_int32), n_jobs, float(resolution), int(flags), None if st is None else _L.ptr(st, _C.c_int64),
                _L.ptr(out, _C.c_int32)))
        return out

    def fov_select_many(self, handles, Tinv6, range_bounds, bearing_bounds, n_keys):
        """``fov_select`` for n_jobs keyed clouds in one launch: Tinv6 / range_bounds / bearing_bounds are lists (one entry per
        job, any number of frames each) -> (per-key counts [n_jobs x n_keys], selected [n_jobs], undecided [n_jobs])"""
        h = np.ascontiguousarray(handles, np.int32).reshape(-1)
        n_jobs = len(h)
        nf = np.array([len(np.asarray(r).reshape(-1)) for r in range_bounds], np.int32)
        off = np.ascontiguousarray(np.r_[0, np.cumsum(nf)], np.int32)
        cat = (lambda xs, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1, w) for x in xs]) if n_jobs else
                                                     np.zeros((0, w)), dt))
        T, rb, bb = cat(Tinv6, np.float32, 6), cat(range_bounds, np.float64, 1), cat(bearing_bounds, np.float64, 1)
        assert len(T) == len(rb) == len(bb) == off[-1] and len(nf) == n_jobs
        hist = np.zeros((n_jobs, int(n_keys)), np.int32)
        n_sel, n_amb = np.zeros(n_jobs, np.int32), np.zeros(n_jobs, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_fov_select_many(
                self.ctx.handle, self.handle, _L.ptr(h, _C.c_int32), n_jobs, _L.ptr(T, _C.c_float), _L.ptr(rb, _C.c_double),
                _L.ptr(bb, _C.c_double), _L.ptr(off, _C.c_int32), int(n_keys), _L.ptr(hist, _C.c_int32),
                _L.ptr(n_sel, _C.c_int32), _L.ptr(n_amb, _C.c_int32)))
        return hist, n_sel, n_amb

    def compact_selected_many(self, handles, stamps=None):
        """``compact_selected`` for n_jobs clouds in one launch -> new keyed handles [n_jobs]"""
        h = np.ascontiguousarray(handles, np.int32).reshape(-1)
        st = None if stamps is None else np.ascontiguousarray(stamps, np.int64).reshape(len(h))
        out = np.full(len(h), -1, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_compact_selected_many(
                self.ctx.handle, self.handle, _L.ptr(h, _C.c_int32), len(h), None if st is None else _L.ptr(st, _C.c_int64),
                _L.ptr(out, _C.c_int32)))
        return out

    def match_keys_many(self, sources, T6, targets, max_dist, n_keys, flags=0):
        """``match_keys`` for n_jobs (source, T6 [6], keyed target) triples in one launch -> (per-key counts [n_jobs x n_keys],
        overlaps [n_jobs])"""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        tgt = np.ascontiguousarray(targets, np.int32).reshape(-1)
        n_jobs = len(src)
        assert len(tgt) == n_jobs
        T6 = np.ascontiguousarray(T6, np.float32).reshape(n_jobs, 6)
        hist = np.zeros((n_jobs, int(n_keys)), np.int32)
        ov = np.zeros(n_jobs, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store_match_keys_many(
                self.ctx.handle, self.handle, _L.ptr(src, _C.c_int32), _L.ptr(T6, _C.c_float), _L.ptr(tgt, _C.c_int32), n_jobs,
                float(max_dist), int(flags), int(n_keys), _L.ptr(hist, _C.c_int32), _L.ptr(ov, _C.c_int32)))
        return hist, ov

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            self.ctx.lib.sfe_cloud_store_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pose_H12(matrix):
    """The twelve float32 numbers Keyframe.transform_points_3D reads from a 4 x 4 matrix H (slam_objects.py:200-223,
    ``points.dot(H[:3, :3].T) + H[:3, 3]``): rows 0..2, row-major."""
    H = np.asarray(matrix, np.float32)
    if H.shape != (4, 4):
        raise TypeError("CloudStore3: a transform must be 4 x 4, got %r" % (H.shape,))
    return H[:3, :].reshape(12)


def fov3_numpy(points, Hinv, range_bound, bearing_bound):
    """One frame of the field-of-view gate of slam.py:891-894 on an N x 3 float32 cloud, in plain numpy: the points moved
    into the frame by ``Keyframe.transform_points_3D``'s product, the range over all three columns, the bearing over x and y
    (no elevation gate: the reference has none) -> bool [N]"""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    H = np.asarray(Hinv, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        local_points = points.dot(H[:3, :3].T) + H[:3, 3]
        ranges = np.linalg.norm(local_points, axis=1)
        bearings = np.arctan2(local_points[:, 1], local_points[:, 0])
        return (ranges < range_bound) & (abs(bearings) < bearing_bound)


class CloudStore3(object):
    """``sfe_cloud_store3``: the keyframe store for N x 3 float32 clouds (``Keyframe.points3D``).  Clouds live in HBM under
    integer handles; ``get_points`` (transform + concatenate + the 3-D ``pcl.downsample``), ``icp`` (the 3-D point-to-point
    ICP of ``pcl.ICP``) and ``overlap`` take handles and return, bit for bit, what the host-pointer ``pcl`` calls return on
    the same clouds moved by numpy's float32 ``points.dot(H[:3, :3].T) + H[:3, 3]``.  A call that does not fit the pool or the
    slot table raises (SFE_ERR_CAP) and leaves the store as it was.

    Keyed clouds (a keyframe index per point): ``put_keys`` / ``get_points_keys`` make them -- the SLAM cloud of
    slam_ros.py:317-359 -- and ``fov_select``, ``compact_selected`` and ``match_keys`` run the candidate selection of the
    loop-closure search (slam.py:873-902, :977-997) on them, many clouds per call.  No device-to-device producer (clouds
    come in through ``put`` / ``put_keys``) and no ``FrontEnd`` / ``SessionBatch`` wiring in 3-D."""

    def __init__(self, ctx=None, capacity_points=1 << 22, max_clouds=1 << 16):
        self.ctx = ctx or _L.default_context()
        h = _C.c_void_p()
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_create(self.ctx.handle, int(capacity_points), int(max_clouds),
                                                                 _C.byref(h)))
        self.handle = h
        self.capacity_points, self.max_clouds = int(capacity_points), int(max_clouds)

    def put(self, points, stamp=0):
        """one host cloud (N x 3, rounded to float32 like the pybind boundary; N may be 0) -> handle"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        h = _C.c_int32(-1)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_put(self.ctx.handle, self.handle, int(stamp),
                                                              _L.ptr(pts, _C.c_float), len(pts), _C.byref(h)))
        return h.value

    def __len__(self):
        return int(self.ctx.lib.sfe_cloud_store3_count(self.handle))

    def meta(self, first=0, n=None):
        """-> (stamps int64, offsets int64, counts int32) of clouds first .. first + n - 1"""
        n = len(self) - first if n is None else int(n)
        st, off, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_meta(self.ctx.handle, self.handle, int(first), n,
                                                               _L.ptr(st, _C.c_int64), _L.ptr(off, _C.c_int64),
                                                               _L.ptr(cnt, _C.c_int32)))
        return st, off, cnt

    def counts(self, handles):
        handles = np.asarray(handles, np.int64).reshape(-1)
        if len(handles) == 0:
            return np.zeros(0, np.int32)
        lo, hi = int(handles.min()), int(handles.max())
        return self.meta(lo, hi - lo + 1)[2][handles - lo]

    def read(self, handle):
        """the points of one cloud (N x 3 float32), copied to the host"""
        n = int(self.counts([handle])[0])
        out = np.zeros((n, 3), np.float32)
        m = _C.c_int(0)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_read(self.ctx.handle, self.handle, int(handle),
                                                               _L.ptr(out, _C.c_float), len(out), _C.byref(m)))
        return out

    def truncate(self, n_slots):
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_truncate(self.ctx.handle, self.handle, int(n_slots)))

    def get_points(self, handle_lists, transforms, resolution, stamps=None):
        """SLAM.get_points on 3-D clouds for many targets at once.  ``handle_lists``: one list of handles per target (-1 =
        unused; the lists may differ in length); ``transforms``: per target one 4 x 4 matrix per listed handle (cloud k is
        moved by ``points.dot(H[:3, :3].T) + H[:3, 3]`` in float32).  The clouds of a target are concatenated in list order
        and downsampled like ``pcl.downsample(points, resolution)`` (``resolution <= 0``: not at all).
        -> new handles int32 [n_targets]"""
        n_jobs = len(handle_lists)
        if len(transforms) != n_jobs:
            raise ValueError("CloudStore3.get_points: %d handle lists but %d transform lists" % (n_jobs, len(transforms)))
        m = max([len(h) for h in handle_lists] + [1])
        handles = np.full((n_jobs, m), -1, np.int32)
        H12 = np.zeros((n_jobs, m, 12), np.float32)
        for j, (hs, Hs) in enumerate(zip(handle_lists, transforms)):
            if len(hs) != len(Hs):
                raise ValueError("CloudStore3.get_points: target %d lists %d handles but %d transforms" % (j, len(hs), len(Hs)))
            for k, (h, H) in enumerate(zip(hs, Hs)):
                handles[j, k] = int(h)
                H12[j, k] = pose_H12(H)
        out = np.full(n_jobs, -1, np.int32)
        st = None if stamps is None else np.ascontiguousarray(stamps, np.int64).reshape(n_jobs)
        with self.ctx.lock:
            # float(resolution) through c_float: the rounding pcl.downsample applies at the same boundary
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_get_points(
                self.ctx.handle, self.handle, _L.ptr(handles, _C.c_int32), _L.ptr(H12, _C.c_float), n_jobs, m,
                float(resolution), None if st is None else _L.ptr(st, _C.c_int64), _L.ptr(out, _C.c_int32)))
        return out

    def icp(self, pairs, guesses, params):
        """The 3-D scan match over handles: pairs [n x 2] = (source, target), guesses [n x 4 x 4]
        -> (status int32 [n], T [n x 4 x 4] float32, iterations int32 [n]), bit for bit ``pcl.ICP.compute_jobs`` on the same
        clouds.  ``params``: an ``IcpParams`` or an ``icp_config.IcpChain``; what ``pcl.ICP`` refuses on N x 3 input
        (data-point filters, the MinDist / MedianDist / Bound modules, the 2-D point-to-plane form) is refused here in the
        same words; ``minimizer = 2`` (PointToPlaneErrorMinimizer {force2D: 0}) and ``minimizer = 3`` ({force4DOF: 1}: yaw
        and translation only) run, pairs on one target handle sharing its normals.  A chain written for N x 3 clouds (``IcpChain.dims == 3``) runs whole: its reading filters once on every
        distinct source handle of the call, its reference filters once on every distinct target handle, into context
        scratch (the store is left as it was), its MinDist / MedianDist / Bound modules inside the loop; a job whose
        filters leave no point reports status 7."""
        from . import pcl as _pcl
        icp = _pcl.ICP(self.ctx)
        if isinstance(params, _cfg.IcpChain):
            icp.setChain(params)
        elif isinstance(params, _L.IcpParams):
            icp.setParams(params)
        else:
            raise TypeError("CloudStore3.icp: expected an IcpParams or an icp_config.IcpChain, got %s" % type(params).__name__)
        p = icp._chain3("CloudStore3.icp")
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        g = np.ascontiguousarray(np.asarray(guesses, np.float32).reshape(n, 16))
        T, st, it = np.zeros((n, 4, 4), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        ext = icp._ext3()
        if ext is not None:
            with self.ctx.lock:
                self.ctx._check(self.ctx.lib.sfe_icp3_store_compute_chain_ext(
                    self.ctx.handle, _C.byref(p), *(ext + (
                        self.handle, _L.ptr(pairs, _C.c_int32), _L.ptr(g, _C.c_float), n, _L.ptr(T, _C.c_float),
                        _L.ptr(st, _C.c_int32), _L.ptr(it, _C.c_int32)))))
            return st, T, it
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_icp3_store_compute(
                self.ctx.handle, _C.byref(p), self.handle, _L.ptr(pairs, _C.c_int32), _L.ptr(g, _C.c_float), n,
                _L.ptr(T, _C.c_float), _L.ptr(st, _C.c_int32), _L.ptr(it, _C.c_int32)))
        return st, T, it

    def overlap(self, pairs, transforms, max_dist):
        """SLAM.get_overlap in 3-D for many (source, target) pairs: the source moved by its 4 x 4 transform, the points of
        it with a target point within ``max_dist`` (``pcl.match(target, moved, 1, max_dist)``, ids != -1) -> int32 [n]"""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        if len(transforms) != n:
            raise ValueError("CloudStore3.overlap: %d pairs but %d transforms" % (n, len(transforms)))
        H12 = np.ascontiguousarray(np.stack([pose_H12(H) for H in transforms]) if n else np.zeros((0, 12)), np.float32)
        out = np.zeros(n, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_overlap(
                self.ctx.handle, self.handle, _L.ptr(pairs, _C.c_int32), _L.ptr(H12, _C.c_float), n, float(max_dist),
                _L.ptr(out, _C.c_int32)))
        return out

    # -- keyed clouds: the SLAM cloud and the candidate selection of the loop-closure search (slam.py:873-902, :977-997) --
    @staticmethod
    def _keys(keys, n, what):
        wide = np.asarray(keys).reshape(-1)
        if len(wide) != n:
            raise ValueError("%s: %d keys for %d %s" % (what[0], len(wide), n, what[1]))
        if len(wide) and not (np.all(wide >= 0) and np.all(wide < 2 ** 31) and np.all(wide == np.floor(wide))):
            raise ValueError("%s: keys must be integers in [0, 2^31)" % what[0])
        return np.ascontiguousarray(wide, np.int32)

    @staticmethod
    def _points3(points, what):
        pts = np.asarray(points)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError("%s: points must be N x 3, got %r" % (what, pts.shape))
        return np.ascontiguousarray(pts, np.float32)

    def put_keys(self, points, keys, stamp=0):
        """``put`` with a key per point (integers in [0, 2^31)): a keyed cloud, as ``get_points_keys`` leaves one -> handle"""
        pts = self._points3(points, "CloudStore3.put_keys")
        ks = self._keys(keys, len(pts), ("CloudStore3.put_keys", "points"))
        h = _C.c_int32(-1)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_put_keys(self.ctx.handle, self.handle, int(stamp),
                                                                   _L.ptr(pts, _C.c_float), _L.ptr(ks, _C.c_int32), len(pts),
                                                                   _C.byref(h)))
        return h.value

    def is_keyed(self, handle):
        r = int(self.ctx.lib.sfe_cloud_store3_keyed(self.handle, int(handle)))
        if r < 0:
            raise ValueError("CloudStore3.is_keyed: no cloud %d" % int(handle))
        return bool(r)

    def get_points_keys(self, handle_lists, transform_lists, key_lists, resolution, stamps=None):
        """``SLAM.get_points(frames, ref, return_keys=True)`` on 3-D clouds for many targets at once: per target a list of
        handles (-1 = unused), one 4 x 4 matrix and one key per listed handle.  Cloud k is moved by its matrix, every point of
        it tagged with its key, the clouds concatenated in list order and downsampled like ``pcl.downsample(points, keys,
        resolution)`` (``resolution <= 0``: not at all).  The points are those of ``get_points`` for the same inputs.
        -> new keyed handles int32 [n_targets] (their keys: ``read_keys``)"""
        n_jobs = len(handle_lists)
        if len(transform_lists) != n_jobs or len(key_lists) != n_jobs:
            raise ValueError("CloudStore3.get_points_keys: %d handle lists but %d transform lists and %d key lists"
                             % (n_jobs, len(transform_lists), len(key_lists)))
        hs, Hs, ks, off = [], [], [], [0]
        for j, (h, H, k) in enumerate(zip(handle_lists, transform_lists, key_lists)):
            if len(H) != len(h):
                raise ValueError("CloudStore3.get_points_keys: target %d lists %d handles but %d transforms" % (j, len(h), len(H)))
            ks.append(self._keys(k, len(h), ("CloudStore3.get_points_keys: target %d" % j, "handles")))
            hs.extend(int(x) for x in h)
            Hs.extend(pose_H12(x) for x in H)
            off.append(len(hs))
        handles = np.ascontiguousarray(hs, np.int32).reshape(-1)
        H12 = np.ascontiguousarray(np.stack(Hs) if Hs else np.zeros((0, 12)), np.float32)
        keys = np.ascontiguousarray(np.concatenate(ks) if ks else np.zeros(0), np.int32)
        job_off = np.ascontiguousarray(off, np.int32)
        out = np.full(n_jobs, -1, np.int32)
        st = None if stamps is None else np.ascontiguousarray(stamps, np.int64).reshape(n_jobs)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_get_points_keys(
                self.ctx.handle, self.handle, _L.ptr(handles, _C.c_int32), _L.ptr(H12, _C.c_float), _L.ptr(keys, _C.c_int32),
                _L.ptr(job_off, _C.c_int32), n_jobs, float(resolution), None if st is None else _L.ptr(st, _C.c_int64),
                _L.ptr(out, _C.c_int32)))
        return out

    def read_keys(self, handle):
        """the keys of one keyed cloud (int32 [N]), copied to the host"""
        n = int(self.counts([handle])[0])
        out = np.zeros(n, np.int32)
        m = _C.c_int(0)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_read_keys(self.ctx.handle, self.handle, int(handle),
                                                                    _L.ptr(out, _C.c_int32), len(out), _C.byref(m)))
        return out

    def fov_select(self, handles, Hinv_lists, range_bounds, bearing_bounds, n_keys, resolve=True):
        """The field-of-view gate of slam.py:875-899 on keyed 3-D clouds, many at once: cloud ``handles[j]`` against the
        frames of ``Hinv_lists[j]`` (4 x 4 matrices, ``pose.inverse()``) with ``range_bounds[j]`` / ``bearing_bounds[j]`` (one
        float64 per frame).  A point is selected iff some frame sees it (``fov3_numpy``); the selection stays on the device
        for ``compact_selected``.  -> (per-key counts of the selected points int32 [n x n_keys], selected int32 [n],
        undecided int32 [n]).  With ``resolve`` a cloud the device could not decide (a bearing within 1e-6 of its bound) is read
        back, gated by ``fov3_numpy`` and written with ``set_selection``, so the caller always gets numpy's selection and
        the third array is zero; without it the three arrays are the device's own."""
        h = np.ascontiguousarray(handles, np.int32).reshape(-1)
        n_jobs = len(h)
        if not (len(Hinv_lists) == len(range_bounds) == len(bearing_bounds) == n_jobs):
            raise ValueError("CloudStore3.fov_select: %d handles but %d frame lists, %d range-bound lists and %d bearing-bound "
                             "lists" % (n_jobs, len(Hinv_lists), len(range_bounds), len(bearing_bounds)))
        n_keys = int(n_keys)
        if n_keys < 0:
            raise ValueError("CloudStore3.fov_select: n_keys must be >= 0")
        Hs, rbs, bbs, off = [], [], [], [0]
        for j in range(n_jobs):
            rb = np.asarray(range_bounds[j], np.float64).reshape(-1)
            bb = np.asarray(bearing_bounds[j], np.float64).reshape(-1)
            if not (len(Hinv_lists[j]) == len(rb) == len(bb)):
                raise ValueError("CloudStore3.fov_select: cloud %d has %d frames but %d range bounds and %d bearing bounds"
                                 % (j, len(Hinv_lists[j]), len(rb), len(bb)))
            Hs.extend(pose_H12(H) for H in Hinv_lists[j])
            rbs.append(rb)
            bbs.append(bb)
            off.append(len(Hs))
        H12 = np.ascontiguousarray(np.stack(Hs) if Hs else np.zeros((0, 12)), np.float32)
        rb = np.ascontiguousarray(np.concatenate(rbs) if rbs else np.zeros(0), np.float64)
        bb = np.ascontiguousarray(np.concatenate(bbs) if bbs else np.zeros(0), np.float64)
        frame_off = np.ascontiguousarray(off, np.int32)
        hist = np.zeros((n_jobs, n_keys), np.int32)
        n_sel, n_amb = np.zeros(n_jobs, np.int32), np.zeros(n_jobs, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_fov_select(
                self.ctx.handle, self.handle, _L.ptr(h, _C.c_int32), n_jobs, _L.ptr(H12, _C.c_float), _L.ptr(rb, _C.c_double),
                _L.ptr(bb, _C.c_double), _L.ptr(frame_off, _C.c_int32), n_keys, _L.ptr(hist, _C.c_int32),
                _L.ptr(n_sel, _C.c_int32), _L.ptr(n_amb, _C.c_int32)))
        if resolve:
            for j in np.nonzero(n_amb)[0]:
                pts, keys = self.read(int(h[j])), self.read_keys(int(h[j]))
                sel = np.zeros(len(pts), bool)
                for H, r, b in zip(Hinv_lists[j], rbs[j], bbs[j]):
                    sel |= fov3_numpy(pts, H, r, b)
                self.set_selection(int(h[j]), sel)
                picked = keys[sel]
                hist[j] = np.bincount(picked[picked < n_keys], minlength=n_keys)[:n_keys]
                n_sel[j], n_amb[j] = int(sel.sum()), 0
        return hist, n_sel, n_amb

    def set_selection(self, handle, sel):
        """the host's selection (one value per point, non-zero = selected) replaces the device's"""
        sel = np.ascontiguousarray(np.asarray(sel).reshape(-1) != 0, np.uint8)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_set_selection(self.ctx.handle, self.handle, int(handle),
                                                                        _L.ptr(sel, _C.c_uint8), len(sel)))

    def compact_selected(self, handles, stamps=None):
        """``points[sel]``, ``keys[sel]`` (slam.py:898-899) of many keyed clouds, order kept -> new keyed handles int32 [n]"""
        h = np.ascontiguousarray(handles, np.int32).reshape(-1)
        st = None if stamps is None else np.ascontiguousarray(stamps, np.int64).reshape(len(h))
        out = np.full(len(h), -1, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_compact_selected(
                self.ctx.handle, self.handle, _L.ptr(h, _C.c_int32), len(h), None if st is None else _L.ptr(st, _C.c_int64),
                _L.ptr(out, _C.c_int32)))
        return out

    def match_keys(self, pairs, transforms, max_dist, n_keys):
        """slam.py:977-985 for many (source, keyed target) pairs: the source moved by its 4 x 4 transform, every moved point
        matched like ``pcl.match(target, moved, 1, max_dist)`` -> (per-key counts of the matched targets int32 [n x n_keys],
        overlaps int32 [n] = ``overlap`` of the same pairs)"""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        if len(transforms) != n:
            raise ValueError("CloudStore3.match_keys: %d pairs but %d transforms" % (n, len(transforms)))
        n_keys = int(n_keys)
        if n_keys < 0:
            raise ValueError("CloudStore3.match_keys: n_keys must be >= 0")
        H12 = np.ascontiguousarray(np.stack([pose_H12(H) for H in transforms]) if n else np.zeros((0, 12)), np.float32)
        hist = np.zeros((n, n_keys), np.int32)
        ov = np.zeros(n, np.int32)
        with self.ctx.lock:
            self.ctx._check(self.ctx.lib.sfe_cloud_store3_match_keys(
                self.ctx.handle, self.handle, _L.ptr(pairs, _C.c_int32), _L.ptr(H12, _C.c_float), n, float(max_dist), n_keys,
                _L.ptr(hist, _C.c_int32), _L.ptr(ov, _C.c_int32)))
        return hist, ov

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            self.ctx.lib.sfe_cloud_store3_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
