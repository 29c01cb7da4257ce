"""Many independent SLAM sessions advanced in lock-step, every cloud device-resident.

One session is what ``replay.FrontEnd`` runs: ping -> FeatureExtraction.callback -> keyframe test -> target cloud
= get_points(last 3 keyframes) -> ICP(source, target, odometry guess) -> sanity checks + overlap -> pose
(slam_ros.py:157-213, slam.py:716-832).  Inside a session the keyframes are strictly sequential -- keyframe k's
target cloud needs the poses the scan matches of k-1, k-2, k-3 produced -- so the batch axis is the SESSION: S
trajectories (robots, bags, replays) step together, step k = keyframe k of every session:

    CFAR + gate -> remap + nonzero + px->m -> downsample -> outlier filter      sfe_*_batch_dev, S pings
    -> append to the keyframe store (slam_ros.py:170 convention)                 sfe_cloud_store_put_batch_dev
    -> S target clouds: transform + concatenate + pcl.downsample                 sfe_cloud_store_get_points
    -> S scan matches over handles                                               sfe_icp_store_compute
    -> S overlap counts                                                          sfe_cloud_store_overlap

The host does what the SLAM node's Python does between those calls -- gtsam.Pose2 algebra in double, the
ssm_min_points / max translation / max rotation / overlap tests, the factor list -- on S sessions at a time, with
exactly the arithmetic of ``pose2.Pose2`` (so a session's records equal those of ``replay.FrontEnd`` on the same
pings bit for bit: tests/test_gpu_store.py).  Per step three small synchronisations (cloud sizes; scan-match
results; overlap counts); no cloud crosses PCIe.

``initialization=True`` adds the reference's default step in front of every scan match (slam.py:77, :665-716): the
global initialisation by ``scipy.optimize.shgo`` over the matching cost.  shgo itself is host Python per session (its
Delaunay / minimiser-pool bookkeeping: tens of milliseconds per call, far more than the scoring); what the device
takes is the cost function: the target grids of all S sessions are built in one launch, shgo's sampling points -- the
same Sobol set for every session, since the bounds are the odometry sigmas -- are scored for all sessions in one more
(``matching_cost.batch_store``), and each session's shgo then runs on that table; the handful of further points its
local minimiser asks for (finite-difference neighbours) are scored one call each.

``nssm_enable=True`` (off by default here; FrontEnd's other ``nssm_*`` arguments and defaults) adds the loop-closure search
(slam.py:839-1087) of every session after its scan match, in ``FrontEnd._feed``'s order -- marginal covariance, append, search
-- and with FrontEnd's own host decisions (replay.fov_bounds, nssm_pose_bounds, initial_transforms, robust_covariance,
large_transformation).  Sessions leave it at different gates; each stage is one call over the sessions still searching:

    source clouds, refined targets, target moved to its keyframe                 sfe_cloud_store_get_points
    keyed global targets (own downsample each)                                    sfe_cloud_store_get_points_keys_many
    field-of-view gate / compaction                                               sfe_cloud_store_fov_select_many / compact_selected_many
    shgo(100, 5) candidates + finite-difference points of all sessions            sfe_costgrid_create_store + sfe_matching_cost_store
    target-key refinement                                                         sfe_cloud_store_match_keys_many
    <= 30 guesses per session / overlaps                                          sfe_icp_store_compute / sfe_cloud_store_overlap

On the host, per session: shgo_fast.replay_multi (scipy.optimize.shgo after a FALLBACK or with shgo_replay=False), the numpy
gate of a session whose device gate reports undecided points, MinCovDet.  ``rec["nssm"][s]`` is FrontEnd's ``rec["nssm"]``
bit for bit (None: no search), ``loops[s]`` its loop factors; every cloud of a step's searches is dropped at its end.
"""
import math

import numpy as np

from . import _lib as _L
from . import icp_config as _cfg
from . import store as _store


class Pose2Batch(object):
    """``pose2.Pose2`` for n poses at once: the same double-precision expressions, element by element (cos / sin /
    atan2 through ``math`` per element, so that no vector math library rounds differently from the scalar class)."""

    __slots__ = ("x", "y", "c", "s")

    def __init__(self, x, y, theta=None, cs=None):
        self.x, self.y = np.array(x, np.float64), np.array(y, np.float64)
        if cs is None:
            th = np.asarray(theta, np.float64)
            self.c = np.array([math.cos(t) for t in th])
            self.s = np.array([math.sin(t) for t in th])
        else:
            c, s = np.array(cs[0], np.float64), np.array(cs[1], np.float64)
            scale = c * c + s * s
            fix = np.abs(scale - 1.0) > 1e-10
            if fix.any():
                with np.errstate(invalid="ignore", divide="ignore"):
                    k = 1.0 / np.sqrt(scale)
                c, s = np.where(fix, c * k, c), np.where(fix, s * k, s)
            self.c, self.s = c, s

    def __len__(self):
        return len(self.x)

    def theta(self):
        return np.array([math.atan2(s, c) for s, c in zip(self.s, self.c)])

    def compose(self, o):
        return Pose2Batch(self.x + self.c * o.x - self.s * o.y, self.y + self.s * o.x + self.c * o.y,
                          cs=(self.c * o.c - self.s * o.s, self.s * o.c + self.c * o.s))

    def inverse(self):
        return Pose2Batch(-(self.c * self.x + self.s * self.y), -(-self.s * self.x + self.c * self.y),
                          cs=(self.c, -self.s))

    def between(self, o):
        return self.inverse().compose(o)

    def T6(self):
        """[n x 6] float32: T00 T01 T02 T10 T11 T12 of ``matrix().astype(np.float32)``"""
        return np.stack([self.c, -self.s, self.x, self.s, self.c, self.y], axis=1).astype(np.float32)

    def matrix32(self):
        """[n x 3 x 3] float32 = ``matrix()`` handed to pybind (the ICP guess, slam.py:316)"""
        M = np.zeros((len(self), 3, 3), np.float64)
        M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = self.c, -self.s, self.x
        M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = self.s, self.c, self.y
        M[:, 2, 2] = 1.0
        return M.astype(np.float32)

    def take(self, idx):
        return Pose2Batch(self.x[idx], self.y[idx], cs=(self.c[idx], self.s[idx]))

    def put(self, idx, o):
        self.x[idx], self.y[idx], self.c[idx], self.s[idx] = o.x, o.y, o.c, o.s

    def xytheta(self):
        return np.stack([self.x, self.y, self.theta()], axis=1)


def sample_transforms(lib, target, source, X):
    """T6 [n x len(X) x 6] float32 of target_i.between(source_i.compose(Pose2(*x))) for Pose2Batch target / source (n poses each)
    and deltas X [P x 3]: the cost function's sample transforms (slam.py:548-550) of n sessions at once.  The arithmetic is
    Pose2's, done by the library's host routine (sfe_pose2_sample_transforms); cos / sin of the deltas through ``math`` like Pose2."""
    import ctypes as _C
    X = np.asarray(X, np.float64).reshape(-1, 3)
    n, P = len(target), len(X)
    d4 = np.ascontiguousarray(np.stack([X[:, 0], X[:, 1], [math.cos(t) for t in X[:, 2]], [math.sin(t) for t in X[:, 2]]], axis=1)) \
        if P else np.zeros((0, 4))
    t4 = np.ascontiguousarray(np.stack([target.x, target.y, target.c, target.s], axis=1), np.float64)
    s4 = np.ascontiguousarray(np.stack([source.x, source.y, source.c, source.s], axis=1), np.float64)
    out = np.zeros((n, P, 6), np.float32)
    f64 = _C.POINTER(_C.c_double)
    rc = lib.sfe_pose2_sample_transforms(t4.ctypes.data_as(f64), s4.ctypes.data_as(f64), n, d4.ctypes.data_as(f64), P,
                                         out.ctypes.data_as(_C.POINTER(_C.c_float)))
    if rc != 0:
        raise _L.SonarFEError("sfe_pose2_sample_transforms: %d" % rc)
    return out


class _View(object):
    """a window into a DeviceBuffer (what KeyframeBatch reads as .ptr)"""

    def __init__(self, buf, offset):
        import ctypes as _C
        self.ptr = _C.c_void_p(buf.ptr.value + int(offset))


class SessionBatch(object):
    """S sessions x K pings, all pings resident in HBM.  ``step(k)`` advances every session by its k-th ping."""

    def __init__(self, ctx, geometry, cfar_params, alg, intensity_thr, icp_params, n_sessions, n_steps, dr_poses,
                 max_points=16384, resolution=0.5, outlier_radius=1.0, outlier_min_points=5, point_resolution=0.5,
                 point_noise=0.5, ssm_min_points=50, ssm_max_translation=3.0, ssm_max_rotation=np.deg2rad(30),
                 ssm_target_frames=3, store_points=None, initialization=False, initialization_params=(50, 1, 0.01),
                 odom_sigmas=(0.2, 0.2, 0.02), shgo_workers=1, shgo_replay=True, nssm_enable=False, nssm_initialization=True,
                 nssm_initialization_params=(100, 5, 0.01), nssm_min_st_sep=8, nssm_min_points=50, nssm_max_translation=10.0,
                 nssm_max_rotation=np.deg2rad(60), nssm_source_frames=5, nssm_cov_samples=30, oculus_max_range=30.0,
                 oculus_horizontal_aperture=np.radians(130.0), mcd_random_state=None, mapping=None):
        from .pipeline import KeyframeBatch
        from .replay import ChainBackend
        if mapping is not None:                                  # (checked before anything is allocated)
            mapping = dict(mapping)
            if "ping" not in mapping:
                raise ValueError("SessionBatch: mapping needs a `ping` (num_ranges, range_resolution, bearings)")
            if mapping.get("feed", "host") not in ("host", "store"):
                raise ValueError("SessionBatch: mapping feed must be \"host\" or \"store\", got %r" % (mapping["feed"],))
            if mapping.get("pub_intensity"):
                # the mosaic samples the batch's own resident frames: they must be the map ping's num_ranges x num_bearings
                want = (int(mapping["ping"].num_ranges), len(mapping["ping"].bearings))
                if (int(geometry.polar_rows), int(geometry.polar_cols)) != want:
                    raise ValueError("SessionBatch: mapping with pub_intensity: the batch's frames are %d x %d, the map ping's "
                                     "num_ranges x num_bearings is %d x %d"
                                     % (geometry.polar_rows, geometry.polar_cols, want[0], want[1]))
        self.ctx, self.S, self.K = ctx, int(n_sessions), int(n_steps)
        # loop-closure search (replay.FrontEnd's arguments of the same names, its defaults but for nssm_enable: off here, so that a
        # batch built without it runs, sizes and records exactly what it did before the search existed)
        assert nssm_source_frames < nssm_min_st_sep                                           # slam.py:158
        assert nssm_cov_samples == 0 or nssm_cov_samples < nssm_initialization_params[0] * nssm_initialization_params[1]
        self.nssm_enable, self.nssm_initialization = bool(nssm_enable), nssm_initialization
        self.nssm_initialization_params = tuple(nssm_initialization_params)
        self.nssm_min_st_sep, self.nssm_min_points = nssm_min_st_sep, nssm_min_points
        self.nssm_max_translation, self.nssm_max_rotation = nssm_max_translation, nssm_max_rotation
        self.nssm_source_frames, self.nssm_cov_samples = nssm_source_frames, nssm_cov_samples
        self.oculus_max_range, self.oculus_horizontal_aperture = oculus_max_range, oculus_horizontal_aperture
        self.mcd_random_state = mcd_random_state
        self.icp_odom_sigmas = np.array([0.1, 0.1, 0.01])        # slam.yaml: icp_odom_sigmas (replay.FrontEnd's)
        self._cov_backend = ChainBackend()                       # its marginal_covariance: what FrontEnd's keyframes get
        self.nssm_stats = {"searches": 0, "device_s": 0.0, "shgo_s": 0.0, "mcd_s": 0.0, "host_s": 0.0}
        self.icp_params = icp_params
        self.kb = KeyframeBatch(ctx, geometry, cfar_params, alg, intensity_thr, self._kb_params(), self.S,
                                max_points=max_points)
        self.frame_bytes = self.kb.rows * self.kb.cols
        self._kb_img = self.kb.d_img                     # (kept for free(): the batch's own frame buffer is unused)
        self.d_frames = ctx.alloc(self.K * self.S * self.frame_bytes)
        self.resolution, self.outlier_radius, self.outlier_min_points = resolution, outlier_radius, outlier_min_points
        self.point_resolution, self.point_noise = point_resolution, point_noise
        self.ssm_min_points, self.ssm_max_translation = ssm_min_points, ssm_max_translation
        self.ssm_max_rotation, self.ssm_target_frames = ssm_max_rotation, ssm_target_frames
        # keyframe clouds of K steps + the targets of one step (3 keyframes each before the downsample shrinks them); with the
        # loop-closure search also its scratch clouds of one step: the source (nssm_source_frames keyframes), the keyed global
        # target and its compaction (all older keyframes each), the compaction moved to the target and the refined target
        pts = store_points or int(self.S * (self.K + 4 + (self.nssm_source_frames + 4 * self.K if self.nssm_enable else 0)) * 2048)
        self.store = _store.CloudStore(ctx, capacity_points=pts,
                                       max_clouds=self.S * (self.K + 2 + (self.NSSM_CLOUDS if self.nssm_enable else 0)))
        dr = np.asarray(dr_poses, np.float64).reshape(self.S, self.K, 3)
        self.dr = [Pose2Batch(dr[:, k, 0], dr[:, k, 1], dr[:, k, 2]) for k in range(self.K)]
        self.max_raw = 0
        self.initialization, self.initialization_params = initialization, tuple(initialization_params)
        self.odom_sigmas = np.array(odom_sigmas, np.float64)
        self._sobol = None
        self.shgo_workers, self._shgo_pool = int(shgo_workers), None    # > 1: shgo_pool.ShgoPool (host processes)
        # shgo_replay: sonar_slam_amd/shgo_fast.py -- what shgo decides after its sampling stage, replayed for all sessions from
        # one table of costs; scipy.optimize.shgo itself only for the sessions the replay reports as undecidable
        self.shgo_replay, self._plan = bool(shgo_replay), None
        # mapping: None (no map: the batch allocates, runs and records what it did before maps existed), or a dict: `ping` (what
        # Mapping.add_keyframe reads of a ping: num_ranges, range_resolution, bearings), optionally `max_pixels`, and Mapping's
        # settings -> self.maps, a mapping.MapBatch that step(k) feeds keyframe k of every session; `feed`: "host" (the
        # default: the clouds are read back and handed to add_keyframes) or "store" (add_keyframes_store: the same maps, bit
        # for bit, from the clouds where they lie on the device)
        self.maps, self._map_ping, self._map_feed = None, None, "host"
        if mapping is not None:
            from .mapping import MapBatch
            self._map_ping = mapping.pop("ping")
            self._map_feed = mapping.pop("feed", "host")
            self.maps = MapBatch(ctx, self.S, self.K, **mapping)
            self.maps.configure()
        self.init_stats = {"shgo_s": 0.0, "cost_calls": 0, "table_hits": 0, "speculated": 0, "speculation_failed": 0,
                           "replayed": 0, "replay_fallbacks": 0, "transforms_s": 0.0, "table_s": 0.0, "grids_s": 0.0}
        self.reset()

    @property
    def icp_params(self):
        """the chain of the scan matches: an ``IcpParams`` or an ``icp_config.IcpChain`` (its data-point filters and
        outlier filters / checker run through ``store.icp``); assignable between runs"""
        return self._icp

    @icp_params.setter
    def icp_params(self, params_or_chain):
        if not isinstance(params_or_chain, (_L.IcpParams, _cfg.IcpChain)):
            raise TypeError("SessionBatch: icp_params must be an IcpParams or an icp_config.IcpChain, got %s"
                            % type(params_or_chain).__name__)
        self._icp = params_or_chain

    def _kb_params(self):
        """what KeyframeBatch takes: the IcpParams of the chain"""
        p = self._icp
        return p.params if isinstance(p, _cfg.IcpChain) else p

    def upload_frames(self, k, frames):
        """pings of step k: [S x rows x cols] uint8"""
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.shape == (self.S, self.kb.rows, self.kb.cols)
        self.d_frames.upload(frames, offset=k * self.S * self.frame_bytes)

    def fit_capacity(self):
        """After a first (untimed) run: size the per-ping point capacity by what the pings really hold.  The resident
        downsample's LDS is sized by the capacity -- 128 KB (one frame per CU) at 16 384 points, 64 KB (two per CU) at
        8 192 -- so sessions whose pings stay below 8 192 raw detections run their filters twice as dense."""
        from .pipeline import KeyframeBatch
        if self.max_raw <= 0 or self.max_raw > 7800 or self.kb.cap <= 8192:
            return self.kb.cap
        old = self.kb
        old.d_img = self._kb_img
        self.kb = KeyframeBatch(self.ctx, old.geom, (old.train_hs, old.guard_hs, old.tau), "SOCA", 0, self._kb_params(), self.S,
                                max_points=8192)
        self.kb.alg, self.kb.k, self.kb.intensity_thr = old.alg, old.k, old.intensity_thr
        self._kb_img = self.kb.d_img
        old.free()
        return self.kb.cap

    NSSM_CLOUDS = 5     # clouds one session's loop-closure search holds at once (source, keyed target, compaction, 2 targets)

    def reset(self):
        self.store.truncate(0)
        self.handles = np.full((self.S, self.K), -1, np.int32)      # keyframe k of session s -> store handle
        self.poses = [None] * self.K                                # Pose2Batch per step (every ping is a keyframe)
        self.records = []
        self.covs = [[None] * self.K for _ in range(self.S)]        # marginal covariance per keyframe (loop-closure search)
        self.loops = [[] for _ in range(self.S)]                    # ("loop", target_key, source_key, transform, cov) per session
        if self.maps is not None and any(len(v.keyframes) for v in self.maps.maps):
            self.maps.reset()

    def step(self, k):
        """-> dict of per-session arrays: status codes, sizes, transforms, overlaps, poses"""
        S, kb, store = self.S, self.kb, self.store
        kb.d_img = _View(self.d_frames, k * S * self.frame_bytes)
        kb.run_cfar()
        kb.run_extract()
        # (nothing between these two: run_filter reads the staging slots run_extract filled, and an octree stage of a
        #  chain's ICP rewrites them -- the scan matches below come after it)
        kb.run_filter(self.resolution, self.outlier_radius, self.outlier_min_points)
        src_h = kb.store_clouds(store, stamps=np.arange(S) * self.K + k)
        self.handles[:, k] = src_h
        rec = {"k": k, "status": np.full(S, PRIOR if k == 0 else SUCCESS, np.int8)}
        if k == 0:
            self.poses[0] = self.dr[0]                                      # add_prior (slam.py:426-442)
            rec["n_source"] = store.counts(src_h)
            self._check_raw(k)
            self._check_counts(rec["n_source"], k)
            rec["pose"] = self.poses[0].xytheta()
            self.records.append(rec)
            self._after_keyframe(k, rec)
            self._map_keyframe(k)
            return rec
        # frame.update(current_keyframe.pose.compose(dr_odom))              slam_ros.py:181-184
        prev = self.poses[k - 1]
        dr_odom = self.dr[k - 1].between(self.dr[k])
        pose = prev.compose(dr_odom)
        # target = get_points(last ssm_target_frames keyframes, target_key = k - 1)   slam.py:740-741
        frames = list(range(k))[-self.ssm_target_frames:]
        m = self.ssm_target_frames
        th = np.full((S, m), -1, np.int32)
        T6 = np.zeros((S, m, 6), np.float32)
        for j, key in enumerate(frames):
            th[:, j] = self.handles[:, key]
            T6[:, j] = prev.between(self.poses[key]).T6()
        n_keep = len(store)
        try:
            rec = self._scan_match_step(k, rec, src_h, th, T6, prev, pose)
        finally:
            store.truncate(n_keep)                                          # the targets are dropped, the keyframes stay
        self._after_keyframe(k, rec)
        self._map_keyframe(k)
        return rec

    def _map_keyframe(self, k):
        """keyframe k of every session into its occupancy map: the cloud stored for the ping, the pose just recorded (pose
        corrections are the caller's: ``self.maps.update_poses``)"""
        if self.maps is None:
            return
        poses = [self._pose(k, s) for s in range(self.S)]
        images = {"images": self._frame_images(k)} if self.maps.pub_intensity else {}
        if self._map_feed == "store":
            self.maps.add_keyframes_store(range(self.S), [k] * self.S, poses, self._map_ping, self.store, self.handles[:, k],
                                          **images)
            return
        clouds = self.store.read_many(self.handles[:, k])
        self.maps.add_keyframes(range(self.S), [k] * self.S, poses, self._map_ping, clouds, **images)

    def _frame_images(self, k):
        """the pings of step k where they lie in ``d_frames``, one view per session: the intensity mosaic samples them in
        place, no ping crosses to the host and back"""
        from .mapping import DeviceImage
        base = self.d_frames.ptr.value + k * self.S * self.frame_bytes
        return [DeviceImage(base + s * self.frame_bytes, self.kb.rows, self.kb.cols) for s in range(self.S)]

    def intensity_grids(self, sessions=None):
        """``maps.get_intensity_grid(sessions)``: the published intensity mosaics of the listed sessions (all by default).
        Needs ``mapping=dict(..., pub_intensity=True, intensity_skips="oculus")``."""
        if self.maps is None:
            raise RuntimeError("SessionBatch.intensity_grids: the batch owns no maps: construct it with mapping=dict(ping=...)")
        return self.maps.get_intensity_grid(sessions)

    def slam_clouds(self, sessions=None):
        """``FrontEnd.slam_cloud()`` for the listed sessions (all by default): the keyframes recorded so far under the batch's
        current poses, tagged with their keys and downsampled at ``point_resolution``, in one ``get_points_keys_many`` call ->
        handles of new keyed slots, one per listed session, which the caller drops with ``store.truncate``"""
        sessions = [int(s) for s in (range(self.S) if sessions is None else sessions)]
        for s in sessions:
            if not 0 <= s < self.S:
                raise IndexError("SessionBatch.slam_clouds: session %d of %d" % (s, self.S))
        n = 0
        while n < self.K and self.poses[n] is not None and np.all(self.handles[:, n] >= 0):
            n += 1
        frames = list(range(n))
        h = self.store.get_points_keys_many([self.handles[s, frames] for s in sessions],
                                            [[_store.pose_T6(self._pose(f, s)) for f in frames] for s in sessions],
                                            [frames] * len(sessions), self.point_resolution)
        self._made(h, n - 1, "SLAM")
        return h

    def occupancy_grids2(self, sessions=None, frames=None, resolution=None):
        """``FrontEnd.occupancy_grid2(frames, resolution)`` for the listed sessions (all by default) -> list of OccupancyGrid:
        their SLAM clouds are built in the store (``slam_clouds``), rendered from there in one device call
        (``MapBatch.get_occupancy_grid2_store``) and dropped again.  Needs ``mapping=dict(...)`` with ``pub_occupancy2``
        on."""
        if self.maps is None:
            raise RuntimeError("SessionBatch.occupancy_grids2: the batch owns no maps: construct it with mapping=dict(ping=...)")
        if not self.maps.pub_occupancy2:
            raise RuntimeError("SessionBatch.occupancy_grids2: the maps were configured with pub_occupancy2=False")
        sessions = list(range(self.S) if sessions is None else sessions)
        n_slots = len(self.store)
        try:
            clouds = self.slam_clouds(sessions)
            return self.maps.get_occupancy_grid2_store(self.store, clouds, sessions, frames, resolution)
        finally:
            self.store.truncate(n_slots)

    def _scan_match_step(self, k, rec, src_h, th, T6, prev, pose):
        S, store = self.S, self.store
        tgt_h = store.get_points(th, T6, self.point_resolution)
        counts = store.counts(np.concatenate([src_h, tgt_h]))
        n_src, n_tgt = counts[:S], counts[S:]
        self._check_raw(k)
        self._check_counts(n_src, k)
        self._check_counts(n_tgt, k)
        rec["n_source"], rec["n_target"] = n_src, n_tgt
        enough = (n_src >= self.ssm_min_points) & (n_tgt >= self.ssm_min_points)
        rec["status"][~enough] = NOT_ENOUGH_POINTS
        dr_between = prev.between(pose)
        initial = prev.between(pose)                                        # target_pose.between(keyframe.pose) slam.py:757
        idx = np.nonzero(enough)[0]
        T = np.zeros((S, 3, 3), np.float32)
        icp_status = np.full(S, -1, np.int32)
        iters = np.zeros(S, np.int32)
        overlap = np.full(S, -1, np.int32)
        est = Pose2Batch(dr_between.x.copy(), dr_between.y.copy(), cs=(dr_between.c.copy(), dr_between.s.copy()))
        if self.initialization and len(idx):
            # slam.py:665-716: ICP starts from the pose shgo found; a failed initialisation leaves the odometry factor
            ok_init, est_src, xs, fs = self._global_init(idx, src_h, tgt_h, pose, prev)
            rec["init_success"] = np.zeros(S, bool)
            rec["init_success"][idx] = ok_init
            rec["init_x"], rec["init_cost"] = np.zeros((S, 3)), np.zeros(S)
            rec["init_x"][idx], rec["init_cost"][idx] = xs, fs
            rec["status"][idx[~ok_init]] = INITIALIZATION_FAILURE
            initial.put(idx[ok_init], prev.take(idx[ok_init]).between(est_src.take(np.nonzero(ok_init)[0])))
            idx = idx[ok_init]
        if len(idx):
            pairs = np.stack([src_h[idx], tgt_h[idx]], axis=1)
            Ti, sti, iti = store.icp(self.icp_params, pairs, initial.take(idx).matrix32())
            T[idx], icp_status[idx], iters[idx] = Ti, sti, iti
            # x, y = T[:2, 2]; theta = np.arctan2(T[1, 0], T[0, 0]); gtsam.Pose2(x, y, theta)     slam.py:319-323
            theta32 = np.arctan2(Ti[:, 1, 0], Ti[:, 0, 0])
            e = Pose2Batch(Ti[:, 0, 2].astype(np.float64), Ti[:, 1, 2].astype(np.float64), theta32.astype(np.float64))
            est.put(idx, e)
            rec["status"][idx[sti != 0]] = NOT_CONVERGED
            delta = initial.take(idx).between(e)
            # (the reference: np.linalg.norm(delta.translation()) per scan match; hypot here, for all sessions at once -- the two can
            #  differ in the last bit, i.e. for a translation within 4e-16 m of the 3 m gate)
            large = (np.hypot(delta.x, delta.y) > self.ssm_max_translation) | (np.abs(delta.theta()) > self.ssm_max_rotation)
            rec["status"][idx[(sti == 0) & large]] = LARGE_TRANSFORMATION
            ok = idx[(sti == 0) & ~large]
            if len(ok):
                ov = store.overlap(np.stack([src_h[ok], tgt_h[ok]], axis=1), est.take(ok).T6(), self.point_noise)
                overlap[ok] = ov
                rec["status"][ok[ov < self.ssm_min_points]] = NOT_ENOUGH_OVERLAP
        good = rec["status"] == SUCCESS
        # keyframe.update(target_pose.compose(estimated))   slam.py:825-827; otherwise the dead-reckoned pose stays
        new_pose = Pose2Batch(pose.x.copy(), pose.y.copy(), cs=(pose.c.copy(), pose.s.copy()))
        gi = np.nonzero(good)[0]
        if len(gi):
            new_pose.put(gi, prev.take(gi).compose(est.take(gi)))
        self.poses[k] = new_pose
        rec.update(T=T, icp_status=icp_status, iters=iters, overlap=overlap, transform=est.xytheta(),
                   pose=new_pose.xytheta())
        self.records.append(rec)
        return rec

    # -- global initialisation (slam.py:665-716) for the sessions `idx` --
    def _sobol_points(self, pose_bounds):
        """the points shgo's first sampling stage evaluates for these bounds and parameters: the same for every session
        and every step, so they are asked for once (a dry run of shgo whose `workers` hook stops at the first pool)"""
        from scipy.optimize import shgo
        if self._sobol is None:
            class _Stop(Exception):
                pass
            got = []

            def pool(_fn, xs):
                got.extend(np.asarray(x, np.float64).copy() for x in xs)
                raise _Stop()
            try:
                shgo(func=lambda x: 0.0, bounds=pose_bounds, n=self.initialization_params[0], iters=self.initialization_params[1],
                     sampling_method="sobol", minimizer_kwargs={"options": {"ftol": self.initialization_params[2]}}, workers=pool)
            except _Stop:
                pass
            self._sobol = np.array(got, np.float64).reshape(-1, 3)
        return self._sobol

    def _replay_plan(self, pose_bounds):
        """shgo_fast.SobolPlan for these bounds, or None (replay switched off, more than one shgo iteration, or the replay does
        not reproduce the installed scipy: then every problem goes through scipy.optimize.shgo)"""
        from . import shgo_fast
        if not self.shgo_replay or self.initialization_params[1] != 1:
            return None
        if self._plan is None:
            self._plan = shgo_fast.plan_for(pose_bounds, self.initialization_params[0], self.initialization_params[2])
            if self._plan.checked is None:
                self._plan.self_check()
        return self._plan if self._plan.checked else None

    def warm_up(self):
        """Build and self-check the shgo replays NOW instead of inside the first steps (a few seconds of scipy.optimize.shgo on
        random step functions), and say in the log whether they are active for the installed scipy.  -> shgo_fast.status()"""
        from . import shgo_fast
        pose_stds = np.array([self.odom_sigmas]).T
        self._replay_plan(5.0 * np.c_[-pose_stds, pose_stds])
        if self.nssm_enable and self.nssm_initialization and self.shgo_replay and self.nssm_initialization_params[1] > 1:
            shgo_fast.multi_checked(*self.nssm_initialization_params)
        return shgo_fast.status()

    def _global_init(self, idx, src_h, tgt_h, pose, prev):
        """-> (success [n], estimated source poses Pose2Batch [n], result.x [n x 3], result.fun [n]) for sessions idx"""
        import time
        from scipy.optimize import shgo
        from . import matching_cost as mc
        from . import shgo_fast
        n = len(idx)
        pose_stds = np.array([self.odom_sigmas]).T
        pose_bounds = 5.0 * np.c_[-pose_stds, pose_stds]
        plan = self._replay_plan(pose_bounds)
        # the poses every session's shgo asks for first: the vertices of its sampling stage (+ with the replay the three
        # forward-difference points SLSQP adds per vertex)
        X0 = plan.points.reshape(-1, 3) if plan is not None else self._sobol_points(pose_bounds)
        src_pose, tgt_pose = pose.take(idx), prev.take(idx)

        def transforms(sel, X):
            """T6 [len(sel) x len(X) x 6] of target_pose.between(source_pose.compose(n2g(x))) (slam.py:548-550)"""
            return sample_transforms(self.ctx.lib, tgt_pose.take(sel), src_pose.take(sel), X)
        t_g = time.perf_counter()
        grids = mc._StoreGrids(self.store, tgt_h[idx], self.point_noise)
        self.init_stats["grids_s"] += time.perf_counter() - t_g
        try:
            t_a = time.perf_counter()
            d4 = np.stack([X0[:, 0], X0[:, 1], [math.cos(t) for t in X0[:, 2]], [math.sin(t) for t in X0[:, 2]]], axis=1)
            t4 = np.stack([tgt_pose.x, tgt_pose.y, tgt_pose.c, tgt_pose.s], axis=1)
            s4 = np.stack([src_pose.x, src_pose.y, src_pose.c, src_pose.s], axis=1)
            t_b = time.perf_counter()
            # [n x len(X0)]: one launch, the sample transforms target.between(source.compose(x)) computed on the device
            table = grids.cost_samples(src_h[idx], t4, s4, d4, f64_points=True)
            self.init_stats["transforms_s"] += t_b - t_a
            self.init_stats["table_s"] += time.perf_counter() - t_b
            self.init_stats["table_hits"] += n * len(X0)
            keys = [x.tobytes() for x in X0]
            ok, xs, fs = np.zeros(n, bool), np.zeros((n, 3)), np.zeros(n)
            t0 = time.perf_counter()
            todo = np.arange(n)
            if plan is not None:
                st, vx = plan.solve_many(self.ctx.lib, table.reshape(n, plan.V, 4))
                done = st != shgo_fast.FALLBACK
                good = st == shgo_fast.OK
                ok[good] = True
                xs[good] = plan.X[vx[good]]
                fs[good] = table.reshape(n, plan.V, 4)[np.nonzero(good)[0], vx[good], 0]
                todo = np.nonzero(~done)[0]
                self.init_stats["replayed"] += int(done.sum())
                self.init_stats["replay_fallbacks"] += len(todo)
            if self.shgo_workers > 1 and len(todo) > 1:
                # speculative runs on the host cores (shgo_pool.py), every assumed cost verified in one launch
                from . import shgo_pool
                if self._shgo_pool is None:
                    t_pool = time.perf_counter()
                    self._shgo_pool = shgo_pool.ShgoPool(self.shgo_workers)
                    t0 += time.perf_counter() - t_pool
                out = self._shgo_pool.map([(pose_bounds, self.initialization_params, X0, table[i].astype(np.int64)) for i in todo])
                who = np.concatenate([np.full(len(o[4]), i, np.int64) for i, o in zip(todo, out)])
                bad = np.zeros(n, bool)
                if len(who):
                    asked = np.concatenate([o[4] for o in out])
                    assumed = np.concatenate([o[5] for o in out])
                    T6 = np.zeros((len(who), 1, 6), np.float32)
                    d = Pose2Batch(asked[:, 0], asked[:, 1], asked[:, 2])
                    T6[:, 0] = tgt_pose.take(who).between(src_pose.take(who).compose(d)).T6()
                    true = grids.cost(src_h[idx[who]], T6, True, grid_index=who)[:, 0]
                    np.logical_or.at(bad, who, true != assumed)
                    self.init_stats["cost_calls"] += len(who)
                self.init_stats["speculated"] += len(todo)
                self.init_stats["speculation_failed"] += int(bad.sum())
                for i, o in zip(todo, out):
                    if not bad[i]:
                        ok[i] = o[0]
                        if o[0]:
                            xs[i], fs[i] = o[1], o[2]
                todo = np.nonzero(bad)[0]
            for i in todo:
                cache = dict(zip(keys, table[i]))

                def f(x, i=i, cache=cache):
                    x = np.asarray(x, np.float64)
                    v = cache.get(x.tobytes())
                    if v is None:
                        v = grids.cost(src_h[idx[i:i + 1]], transforms(np.array([i]), [x]), True, grid_index=[i])[0, 0]
                        cache[x.tobytes()] = v
                        self.init_stats["cost_calls"] += 1
                    else:
                        self.init_stats["table_hits"] += 1
                    return np.int64(v)
                res = shgo(func=f, bounds=pose_bounds, n=self.initialization_params[0], iters=self.initialization_params[1],
                           sampling_method="sobol", minimizer_kwargs={"options": {"ftol": self.initialization_params[2]}},
                           workers=lambda _fn, pts: [f(p) for p in pts])
                ok[i] = bool(res.success)
                if res.success:
                    xs[i], fs[i] = res.x, res.fun
            self.init_stats["shgo_s"] += time.perf_counter() - t0
        finally:
            grids.close()
        est = src_pose.compose(Pose2Batch(xs[:, 0], xs[:, 1], xs[:, 2]))
        return ok, est, xs, fs

    # -- loop-closure search (slam.py:839-1087) of every session, after its keyframe is appended (slam_ros.py:207) --
    def _pose(self, k, s):
        """keyframe k of session s as a pose2.Pose2 with the bits of the batch's pose (what FrontEnd's keyframe holds)"""
        from .pose2 import Pose2
        p = self.poses[k]
        return Pose2(float(p.x[s]), float(p.y[s]), _cs=(float(p.c[s]), float(p.s[s])))

    def _after_keyframe(self, k, rec):
        """FrontEnd._feed after the scan match: the keyframe's marginal covariance (ChainBackend.marginal_covariance, kind from
        the scan match's status), then the search -> rec["nssm"] = [S entries: FrontEnd's rec["nssm"], or None: no search]"""
        if not self.nssm_enable:
            return
        import time
        for s in range(self.S):
            kind = "prior" if k == 0 else ("icp" if rec["status"][s] == SUCCESS else "odometry")
            self.covs[s][k] = self._cov_backend.marginal_covariance(k, self.covs[s][k - 1] if k else None, kind)
        rec["nssm"] = [None] * self.S
        if k == 0 or k + 1 < self.nssm_min_st_sep:              # (FrontEnd: current_frame is None / shorter than the exclusion zone)
            return
        n_keep = len(self.store)
        t0 = time.perf_counter()
        try:
            rec["nssm"] = self._nssm_search(k)
        finally:
            self.store.truncate(n_keep)                         # every cloud the searches built is dropped again
        self.nssm_stats["searches"] += self.S
        self.nssm_stats["host_s"] += time.perf_counter() - t0

    def _made(self, handles, k, what):
        """counts of clouds the search just built; a store too small for them fails here (-3: pool full), never silently"""
        n = self.store.counts(handles)
        bad = np.nonzero(n < 0)[0]
        if len(bad):
            raise _L.SonarFEError("step %d: the loop-closure search's %s cloud was not stored (count %d: -1 octree deeper than 24 "
                                  "levels, -3 store full: raise store_points)" % (k, what, int(n[bad[0]])))
        return n

    def _nssm_search(self, k):
        """FrontEnd._nssm for every session at keyframe k, one device call per stage over the sessions still searching; the
        host decisions are FrontEnd's own functions"""
        import time
        from . import pcl
        from .replay import FrontEnd, fov_bounds, icp_result, large_transformation, robust_covariance
        S, store, P, st = self.S, self.store, self._pose, self.nssm_stats
        F32 = _store.F32_POINTS
        K, source_key = k + 1, k
        recs = [{"source_key": source_key} for _ in range(S)]
        source_frames = list(range(source_key, source_key - self.nssm_source_frames, -1))
        target_frames = list(range(K - self.nssm_min_st_sep))
        source_pose = [P(k - 1, s) for s in range(S)]               # slam.py:854: the frame of the PREVIOUS callback

        def done(s, status):
            recs[s]["status"] = status

        t = time.perf_counter()
        # source = get_points(source_frames, source_key)
        T6 = np.array([[_store.pose_T6(P(k, s).between(P(f, s))) for f in source_frames] for s in range(S)], np.float32)
        src_h = store.get_points(self.handles[:, source_frames], T6, self.point_resolution)
        n_src = self._made(src_h, k, "source")
        act = []
        for s in range(S):
            recs[s]["n_source"] = int(n_src[s])
            if n_src[s] < self.nssm_min_points:
                done(s, "NOT_ENOUGH_POINTS")
            else:
                act.append(s)
        # keyed global target, field-of-view gate (slam.py:873-904)
        G = store.get_points_keys_many([self.handles[s, target_frames] for s in act],
                                       [[_store.pose_T6(P(f, s)) for f in target_frames] for s in act],
                                       [target_frames] * len(act), self.point_resolution)
        self._made(G, k, "keyed target")
        bounds = [fov_bounds([P(f, s) for f in source_frames], [self.covs[s][f] for f in source_frames], self.oculus_max_range,
                             self.oculus_horizontal_aperture) for s in act]
        hist, n_sel, n_amb = store.fov_select_many(G, [[_store.pose_T6(p) for p in b[0]] for b in bounds], [b[1] for b in bounds],
                                                   [b[2] for b in bounds], K)
        st["device_s"] += time.perf_counter() - t
        gate = []
        for j, s in enumerate(act):
            h, ns = hist[j], int(n_sel[j])
            if n_amb[j]:        # a bearing within float32 rounding of its bound: numpy decides, for this session alone
                Tinv, rb, bb = bounds[j]
                sel = FrontEnd._fov_numpy(store.read(G[j]), Tinv, rb, bb)
                store.set_selection(G[j], sel)
                h = np.bincount(store.read_keys(G[j])[sel], minlength=K).astype(np.int32)
                ns = int(sel.sum())
            r = recs[s]
            r["fov_ambiguous"] = int(n_amb[j])
            frames1 = np.nonzero(h)[0].astype(np.int32)
            counts = h[frames1]
            r["n_target_global"] = ns
            frames1, counts = frames1[counts > 10], counts[counts > 10]
            if len(frames1) == 0 or ns < self.nssm_min_points:
                done(s, "NOT_ENOUGH_POINTS")
                continue
            r["target_key_fov"] = int(frames1[np.argmax(counts)])
            gate.append((j, s, ns))
        if not gate:
            return recs
        t = time.perf_counter()
        # target_points[sel] moved to the target keyframe (slam.py:898-905)
        C = store.compact_selected_many([G[j] for j, _, _ in gate])
        self._made(C, k, "compacted target")
        tkey = {s: recs[s]["target_key_fov"] for _, s, _ in gate}
        tl = store.get_points(C[:, None], np.array([[_store.pose_T6(P(tkey[s], s).inverse())] for _, s, _ in gate], np.float32),
                              0.0, flags=F32)
        self._made(tl, k, "target")
        st["device_s"] += time.perf_counter() - t
        cur = [dict(s=s, C=int(C[i]), tl=int(tl[i]), n=ns, target_key=tkey[s], target_pose=P(tkey[s], s),
                    est=source_pose[s], samples=None) for i, (_, s, ns) in enumerate(gate)]
        if self.nssm_initialization:
            cur = self._nssm_init(k, cur, recs, src_h, K, target_frames)
        for c in cur:
            recs[c["s"]]["target_key"], recs[c["s"]]["n_target"] = c["target_key"], c["n"]
        # ICPResult (slam_objects.py:247-300): the guesses of every session in one store.icp call
        pairs, guesses, owner = [], [], []
        with_cov = self.nssm_initialization and self.nssm_cov_samples > 0
        for i, c in enumerate(cur):
            c["initial"] = c["target_pose"].between(c["est"])
            if with_cov:
                g = FrontEnd.initial_transforms(c["samples"], c["target_pose"], limit=self.nssm_cov_samples)
                recs[c["s"]]["n_guesses"] = len(g)
            else:
                g = [c["initial"]]
            pairs += [(src_h[c["s"]], c["tl"])] * len(g)
            guesses += [pcl.ICP._guess(x.matrix()) for x in g]
            owner += [i] * len(g)
        t = time.perf_counter()
        if pairs:
            Ts, sts, _ = store.icp(self.icp_params, pairs, guesses)
        st["device_s"] += time.perf_counter() - t
        owner = np.array(owner, np.int64)
        ok_cur = []
        for i, c in enumerate(cur):
            r, mine = recs[c["s"]], np.nonzero(owner == i)[0]
            if with_cov:
                t = time.perf_counter()
                if len(mine):
                    message, odom, cov_icp, samples = robust_covariance(Ts[mine], sts[mine] == 0, self.mcd_random_state,
                                                                        self.icp_odom_sigmas)
                else:
                    message = "Too few samples for covariance computation"
                st["mcd_s"] += time.perf_counter() - t
                r["icp"] = message
                if message != "success":
                    done(c["s"], "NOT_CONVERGED")
                    continue
                r["n_converged"], r["sample_transforms"], r["cov"] = len(samples), samples, cov_icp
            else:
                message, odom = icp_result(Ts[mine[0]], sts[mine[0]])
                cov_icp = None
                r["icp"] = message
                if message != "success":
                    done(c["s"], "NOT_CONVERGED")
                    continue
            r["transform"] = (odom.x(), odom.y(), odom.theta())
            if large_transformation(c["initial"], odom, self.nssm_max_translation, self.nssm_max_rotation):   # slam.py:1066-1077
                done(c["s"], "LARGE_TRANSFORMATION")
                continue
            c["odom"], c["cov"] = odom, cov_icp
            ok_cur.append(c)
        t = time.perf_counter()
        ov = store.overlap([(src_h[c["s"]], c["tl"]) for c in ok_cur], [_store.pose_T6(c["odom"]) for c in ok_cur],
                           self.point_noise, flags=F32) if ok_cur else []
        st["device_s"] += time.perf_counter() - t
        for c, o in zip(ok_cur, ov):
            r = recs[c["s"]]
            r["overlap"] = int(o)
            if o < self.nssm_min_points:
                done(c["s"], "NOT_ENOUGH_OVERLAP")
                continue
            done(c["s"], "SUCCESS")
            self.loops[c["s"]].append(("loop", c["target_key"], source_key, c["odom"], c["cov"]))   # -> PCM + ISAM2: back end
        return recs

    def _nssm_init(self, k, cur, recs, src_h, K, target_frames):
        """slam.py:922-999 for the sessions `cur`: shgo over the matching cost (the candidates of every session and their
        finite-difference points scored in one launch, shgo_fast.replay_multi per session; scipy.optimize.shgo itself where the
        replay is off or reports FALLBACK), then the target key refined by the matches (one launch) and the refined targets
        (one get_points call) -> the sessions still searching"""
        import time
        from . import matching_cost as mc
        from . import shgo_fast
        from .pose2 import Pose2
        from .replay import FrontEnd, nssm_pose_bounds
        store, P, st, params = self.store, self._pose, self.nssm_stats, self.nssm_initialization_params
        source_frames_last = k - self.nssm_source_frames + 1
        for c in cur:
            c["bounds"] = nssm_pose_bounds(self.covs[c["s"]][source_frames_last])
            np.linalg.inv(self.covs[c["s"]][k])                  # slam.py:529 (the subroutine inverts the source's covariance)
        multi = self.shgo_replay and params[1] > 1 and shgo_fast.multi_checked(params[0], params[1], params[2])
        results = [None] * len(cur)
        if multi:
            t = time.perf_counter()
            grids = mc._StoreGrids(store, [c["tl"] for c in cur], self.point_noise)
            try:
                cands, T6 = [], []
                for c in cur:
                    draws, cand, fd = shgo_fast.multi_candidates(c["bounds"], params[0], params[1])
                    cands.append((draws, cand, fd))
                    T6.append(mc._sample_poses(self.ctx.lib, c["est"], c["target_pose"], np.concatenate([cand, fd.reshape(-1, 3)]))[0])
                costs = grids.cost([src_h[c["s"]] for c in cur], np.array(T6), f64_points=False).astype(np.int64)
            finally:
                grids.close()
            st["device_s"] += time.perf_counter() - t
            t = time.perf_counter()
            for i, c in enumerate(cur):
                draws, cand, fd = cands[i]
                M = len(cand)
                cost, fd_cost = costs[i, :M], costs[i, M:].reshape(M, 3)
                sta, x, fun, vertices, minimised = self._replay_multi(c["bounds"], params[0], params[1], draws, cand, cost, fd_cost)
                if sta == shgo_fast.FALLBACK:
                    continue
                X = np.concatenate([cand[vertices], cand[minimised], fd[minimised].reshape(-1, 3)])
                _, poses = mc._sample_poses(self.ctx.lib, c["est"], c["target_pose"], X)
                c["samples"] = list(np.c_[poses, np.concatenate([cost[vertices], cost[minimised],
                                                                  fd_cost[minimised].reshape(-1)]).astype(np.float64)])
                results[i] = (sta == shgo_fast.OK, x, np.int64(fun), True,
                              None if sta == shgo_fast.OK else "Failed to find a feasible minimizer point. Lowest sampling point = %s" % fun)
            st["shgo_s"] += time.perf_counter() - t
        t = time.perf_counter()
        for i, c in enumerate(cur):
            if results[i] is not None:
                continue
            # FrontEnd's own call on this session alone, over its handles: after a FALLBACK of the replay scipy.optimize.shgo
            # (where FrontEnd.shgo goes then), otherwise what FrontEnd.shgo does with these parameters
            sub, samples = mc.get_matching_cost_subroutine1_store(store, int(src_h[c["s"]]), c["est"], c["tl"], c["target_pose"],
                                                                  self.covs[c["s"]][k], point_noise=self.point_noise, f64_points=False)
            try:
                res = FrontEnd.shgo(sub, c["bounds"], params, replay=self.shgo_replay and not multi)
            finally:
                sub.grid.close()
            c["samples"] = samples
            results[i] = (bool(res.success), res.x, res.fun, bool(res.get("replayed", False)), str(res.message))
        st["shgo_s"] += time.perf_counter() - t
        nxt = []
        for i, c in enumerate(cur):
            r = recs[c["s"]]
            success, x, fun, replayed, message = results[i]
            r["init_replayed"] = replayed
            if not success:
                r["status"], r["init_message"] = "INITIALIZATION_FAILURE", message
                continue
            r["init_x"], r["init_cost"] = tuple(float(v) for v in x), float(fun)
            c["est"] = c["est"].compose(Pose2(*x))
            c["samples"] = np.array(c["samples"])
            nxt.append(c)
        if not nxt:
            return nxt
        t = time.perf_counter()
        # refine the target key: the keyframe most of the matched target points came from (slam.py:975-999)
        hist1, overlap = store.match_keys_many([src_h[c["s"]] for c in nxt], [_store.pose_T6(c["est"]) for c in nxt],
                                               [c["C"] for c in nxt], self.point_noise, K, flags=_store.F32_POINTS)
        cur, nxt = nxt, []
        for i, c in enumerate(cur):
            recs[c["s"]]["overlap_global"] = int(overlap[i])
            if overlap[i] == 0:
                recs[c["s"]]["status"] = "NOT_ENOUGH_OVERLAP"
                continue
            c["target_key"] = int(np.argmax(hist1[i]))
            c["target_pose"] = P(c["target_key"], c["s"])
            nxt.append(c)
        if nxt:
            T6 = np.array([[_store.pose_T6(c["target_pose"].between(P(f, c["s"]))) for f in target_frames] for c in nxt], np.float32)
            th = store.get_points(np.array([self.handles[c["s"], target_frames] for c in nxt], np.int32), T6, self.point_resolution)
            n = self._made(th, k, "refined target")
            for c, h, m in zip(nxt, th, n):
                c["tl"], c["n"] = int(h), int(m)
        st["device_s"] += time.perf_counter() - t
        return nxt

    @staticmethod
    def _replay_multi(*args):
        from . import shgo_fast
        return shgo_fast.replay_multi(*args)

    def _check_raw(self, k):
        """a ping with more detections than the batch's point capacity would be truncated silently"""
        raw = self.kb.d_cnt.download(np.int32, self.S)
        self.max_raw = max(self.max_raw, int(raw.max()))
        if int(raw.max()) > self.kb.cap:
            f = int(raw.argmax())
            raise _L.SonarFEError("step %d, session %d: %d points extracted, more than the batch capacity %d "
                                  "(max_points)" % (k, f, raw[f], self.kb.cap))

    def _check_counts(self, counts, k):
        bad = np.nonzero(counts < 0)[0]
        if len(bad):
            raise _L.SonarFEError("step %d, session %d: cloud not stored (count %d: -1 octree deeper than 24 levels, "
                                  "-3 store full)" % (k, int(bad[0]), int(counts[bad[0]])))

    def run(self):
        self.reset()
        for k in range(self.K):
            self.step(k)
        return self.records

    def free(self):
        if self._shgo_pool is not None:
            self._shgo_pool.close()
            self._shgo_pool = None
        self.kb.d_img = self._kb_img
        self.kb.free()
        self.d_frames.free()
        self.store.close()
        if self.maps is not None:
            self.maps.close()


PRIOR, SUCCESS, NOT_ENOUGH_POINTS, NOT_CONVERGED, LARGE_TRANSFORMATION, NOT_ENOUGH_OVERLAP, INITIALIZATION_FAILURE = range(7)
STATUS_NAMES = ("PRIOR", "SUCCESS", "NOT_ENOUGH_POINTS", "NOT_CONVERGED", "LARGE_TRANSFORMATION", "NOT_ENOUGH_OVERLAP",
                "INITIALIZATION_FAILURE")
