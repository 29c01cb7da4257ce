"""Drop-in for the reference's pybind11 module ``bruce_slam.pcl``.

Same names and call signatures as ``PYBIND11_MODULE(pcl, m)``
(bruce_slam/src/bruce_slam/cpp/pcl.cpp:176-214), backed by the HIP kernels of libsonarfe.so:

    match(ref, in, knn, max_dist) -> (ids int32 [knn x N], dists float32 [knn x N])  pcl.cpp:161
    remove_outlier(points, radius, min_points) -> points'                           pcl.cpp:54
    class ICP: loadFromYaml(path), compute(source, target, guess) -> (message, T),
               getCovariance()                                                      pcl.cpp:184-213
    downsample(points[, descriptors], resolution) -> points'[, descriptors']       pcl.cpp:128-159
    density_filter(points[, descriptors], knn, min_density, max_density)           pcl.cpp:76-126 (raises like
                   the reference does; knn_density / max_density_filter are the working pieces)

Clouds are N x 2, or -- for ``match``, ``remove_outlier``, ``downsample``, ``knn_density`` and ``max_density_filter`` --
N x 3, as pcl.cpp takes them (fromEigen labels a z row when mat.cols() == 3, pcl.cpp:23,39; every function returns
topRows(mat_in.cols())): an N x 3 cloud goes to HIP kernels of its own (sfe_pcl3.hip; the 2-D rules with one more
coordinate, an 8-way tree for ``downsample``; brute force, quadratic in the cloud size) and comes back N' x 3; ``match``
wants both clouds of one width (RuntimeError otherwise, like libnabo).  ``ICP.compute*`` takes N x 3 clouds with 4 x 4
guesses too (PM::ICP::compute is dimension-generic) and returns 4 x 4 transforms: the chain of the shipped icp.yaml with
its point-to-point minimiser, with ``PointToPlaneErrorMinimizer {force2D: 0}`` (``minimizer = 2``) or with its yaw-and-
translation form ``{force4DOF: 1}`` (``minimizer = 3``) on a HIP kernel of its own (sfe_icp3.hip, brute force); mixed widths,
data-point filters, the MinDist / MedianDist / Bound modules and the 2-D point-to-plane form (``force2D: 1``) raise
NotImplementedError on 3-D input, the 3-D forms on N x 2 input.

Extension (not in the reference): ``ICP.compute_batch(source, target, guesses)`` runs the
many-guesses-one-pair loop of SLAM.compute_icp_with_cov (slam.py:346-358) in one launch.
``ICP.loadFromYaml`` also takes the data-point filters of a chain (``icp_config.parse_icp_chain``); they run on the
device in front of the ICP launch of ``compute`` / ``compute_batch`` / ``compute_pairs`` / ``compute_jobs``.
"""
import ctypes as _C
import os as _os

import numpy as _np

from . import _lib as _L
from . import icp_config as _cfg


def _cloud(a, name):
    a = _np.ascontiguousarray(a, _np.float32)
    if a.ndim != 2 or a.shape[1] not in (2, 3):
        raise TypeError("%s: expected an N x 2 array, got shape %r" % (name, a.shape))
    if a.shape[1] == 3:
        raise NotImplementedError(
            "%s: N x 3 clouds (3-D ICP) are outside the sonar front-end path; the SLAM node only "
            "passes N x 2 in-plane points (slam.py:309-310)" % name)
    return a


def _cloud23(a, name):
    """a cloud of the filter / matcher functions: N x 2, or N x 3 as the reference's pcl.cpp takes it (fromEigen labels
    a z row when mat.cols() == 3, pcl.cpp:23,39).  The 2-D-only callers keep ``_cloud``."""
    a = _np.ascontiguousarray(a, _np.float32)
    if a.ndim != 2 or a.shape[1] not in (2, 3):
        raise TypeError("%s: expected an N x 2 or N x 3 array, got shape %r" % (name, a.shape))
    return a


def _fn(ctx, name, cloud):
    """the library entry point ``name`` for the cloud's width (``name`` + "3" for N x 3)"""
    return getattr(ctx.lib, name + "3" if cloud.shape[1] == 3 else name)


def match(ref, pts, knn, max_dist, ctx=None):
    """KDTreeMatcher replacement (pcl.cpp:161-174): the knn exact nearest reference points of every query in
    ascending (d2, index) order, squared distances, -1 / inf beyond max_dist.  Both clouds N x 2 or both N x 3.
    -> (ids int32 [knn x N], dists float32 [knn x N]) like the pybind IntMatrix / Matrix pair."""
    knn = int(knn)
    if knn < 1:
        raise RuntimeError("pcl.match: knn must be >= 1, got %d" % knn)
    ref = _cloud23(ref, "match(ref)")
    pts = _cloud23(pts, "match(in)")
    if ref.shape[1] != pts.shape[1]:
        # libnabo: "Query has different dimensionality than the cloud" (a std::runtime_error)
        raise RuntimeError("pcl.match: the reference cloud is N x %d and the query cloud N x %d (libnabo refuses a query "
                           "of another dimensionality)" % (ref.shape[1], pts.shape[1]))
    ctx = ctx or _L.default_context()
    if knn > len(ref):
        # libnabo: "Requesting more points (k) than available in cloud" (a std::runtime_error -> RuntimeError through
        # pybind); knn_density mirrors the same throw
        raise RuntimeError("pcl.match: knn = %d exceeds the %d points of the reference cloud (libnabo throws)"
                           % (knn, len(ref)))
    ids = _np.full((knn, len(pts)), -1, _np.int32)
    d2 = _np.full((knn, len(pts)), _np.inf, _np.float32)
    if len(pts):
        with ctx.lock:
            if knn == 1:    # the SLAM node's only use (slam.py:418): one pass over the reference
                ctx._check(_fn(ctx, "sfe_match", pts)(ctx.handle, _L.ptr(ref, _C.c_float), len(ref),
                                                      _L.ptr(pts, _C.c_float), len(pts), float(max_dist),
                                                      _L.ptr(ids, _C.c_int32), _L.ptr(d2, _C.c_float)))
            else:
                ctx._check(_fn(ctx, "sfe_match_knn", pts)(ctx.handle, _L.ptr(ref, _C.c_float), len(ref),
                                                          _L.ptr(pts, _C.c_float), len(pts), knn, float(max_dist),
                                                          _L.ptr(ids, _C.c_int32), _L.ptr(d2, _C.c_float)))
    return ids, d2


def remove_outlier(points, radius, min_points, ctx=None):
    """PCL RadiusOutlierRemoval replacement (pcl.cpp:54-74); N x 2 or N x 3 (pcl.cpp:61-62 sets .z), same width back."""
    pts = _cloud23(points, "remove_outlier(points)")
    ctx = ctx or _L.default_context()
    out = _np.zeros_like(pts)
    n = _C.c_int(0)
    if len(pts):
        with ctx.lock:
            ctx._check(_fn(ctx, "sfe_remove_outlier", pts)(ctx.handle, _L.ptr(pts, _C.c_float), len(pts),
                                                           float(radius), int(min_points),
                                                           _L.ptr(out, _C.c_float), _C.byref(n)))
    return out[:n.value].copy()


def downsample(points, *args, **kw):
    """libpointmatcher OctreeGridDataPointsFilter replacement (pcl.cpp:128-159), both overloads:
    ``downsample(points, resolution)`` -> points' and
    ``downsample(points, descriptors, resolution)`` -> (points', descriptors').  N x 3 points go through the 8-way
    tree libpointmatcher builds for 3-D features and come back N' x 3."""
    ctx = kw.pop("ctx", None)
    if len(args) == 1:
        desc, resolution = None, args[0]
    elif len(args) == 2:
        desc, resolution = _np.ascontiguousarray(args[0], _np.float32), args[1]
    else:
        raise TypeError("downsample(points, resolution) or downsample(points, descriptors, resolution)")
    pts = _cloud23(points, "downsample(points)")
    if desc is not None and len(desc) != len(pts):
        raise TypeError("downsample: %d descriptors for %d points" % (len(desc), len(pts)))
    if len(pts) == 0:  # pcl.cpp:130-131,145-146
        return pts if desc is None else (pts, desc)
    ctx = ctx or _L.default_context()
    out = _np.zeros_like(pts)
    # (only the descriptor overload needs the indices; the 3-D call always hands them back)
    idx = _np.zeros(len(pts), _np.int32) if desc is not None or pts.shape[1] == 3 else None
    n = _C.c_int(0)
    with ctx.lock:
        ctx._check(_fn(ctx, "sfe_downsample", pts)(ctx.handle, _L.ptr(pts, _C.c_float), len(pts), float(resolution),
                                                   _L.ptr(out, _C.c_float),
                                                   _L.ptr(idx, _C.c_int32) if idx is not None else None, _C.byref(n)))
    out = out[:n.value].copy()
    return out if desc is None else (out, desc[idx[:n.value]].copy())


class _GlibcRand(object):
    """glibc's rand() (TYPE_3 additive feedback generator, r[i] = r[i-3] + r[i-31]), which is what the std::rand()
    of libpointmatcher's MaxDensityDataPointsFilter resolves to on the reference's platform (Ubuntu / ROS noetic).
    Process-wide state like the C library's: seeded with 1 until somebody calls srand."""
    RAND_MAX = 2147483647

    def __init__(self, seed=1):
        self.srand(seed)

    def srand(self, seed):
        seed = int(seed) & 0xFFFFFFFF or 1
        r = [0] * 34
        r[0] = seed
        for i in range(1, 31):
            hi, lo = divmod(r[i - 1], 127773)                 # 16807 * x mod (2^31 - 1), Schrage
            w = 16807 * lo - 2836 * hi
            r[i] = w + 2147483647 if w < 0 else w
        for i in range(31, 34):
            r[i] = r[i - 31]
        self._r = r
        for _ in range(310):
            self._step()

    def _step(self):
        r = self._r
        o = (r[-31] + r[-3]) & 0xFFFFFFFF
        r.append(o)
        del r[0]
        return o

    def rand(self):
        return self._step() >> 1


_rand = _GlibcRand(1)


def srand(seed):
    """std::srand for the random thinning of max_density_filter (extension: the reference never seeds)."""
    _rand.srand(seed)


def knn_density(points, knn, ctx=None):
    """The ``densities`` descriptor pcl.density_filter computes first (pcl.cpp:81-88): libpointmatcher
    SurfaceNormalDataPointsFilter{knn, keepDensities}: knn / ((4/3) pi r^3), r = the largest distance of one of the
    point's knn nearest points (itself included) from their mean.  N x 2 or N x 3 points.  -> float32 [N]"""
    pts = _cloud23(points, "knn_density(points)")
    knn = int(knn)
    if knn < 1:
        raise RuntimeError("knn_density: knn must be >= 1")
    if knn > len(pts):
        raise RuntimeError("Requesting more points than available in cloud")   # libnabo
    ctx = ctx or _L.default_context()
    dens = _np.zeros(len(pts), _np.float32)
    if len(pts):
        with ctx.lock:
            ctx._check(_fn(ctx, "sfe_knn_density", pts)(ctx.handle, _L.ptr(pts, _C.c_float), len(pts), knn,
                                                        _L.ptr(dens, _C.c_float)))
    return dens


def surface_normals(points, knn, ctx=None):
    """The ``normals`` descriptor of libpointmatcher's SurfaceNormalDataPointsFilter{knn, keepNormals} on an N x 3 cloud
    (extension; the routine the 3-D point-to-plane ICP runs on its targets): per point the unit eigenvector of the smallest
    eigenvalue of the scatter matrix of its min(knn, N) nearest points, itself included, ties in distance to the lowest
    index; the sign is arbitrary.  Degenerate neighbourhoods give a finite unit vector ((1, 0, 0) for coincident points).
    ``include/sonarfe.h`` at ``sfe_normals3`` spells the rule out.  2 <= knn <= 16.  -> float32 [N x 3].  N x 2 clouds raise
    NotImplementedError (the 2-D normals exist inside the 2-D ICP kernels only)."""
    pts = _cloud23(points, "surface_normals(points)")
    if pts.shape[1] != 3:
        raise NotImplementedError("surface_normals: N x 2 clouds: the 2-D normals are computed inside the 2-D ICP kernels "
                                  "and are not exposed; pass an N x 3 cloud")
    knn = int(knn)
    if not 2 <= knn <= 16:
        raise RuntimeError("surface_normals: knn %d outside [2, 16]" % knn)
    ctx = ctx or _L.default_context()
    out = _np.zeros((len(pts), 3), _np.float32)
    if len(pts):
        with ctx.lock:
            ctx._check(ctx.lib.sfe_normals3(ctx.handle, _L.ptr(pts, _C.c_float), len(pts), knn, _L.ptr(out, _C.c_float)))
    return out


def max_density_filter(points, *args, **kw):
    """What the body of the reference's ``density_filter`` does once its stray ``minDensity`` parameter is taken out
    (pcl.cpp:76-126): densities from the knn nearest neighbours (``knn_density``), then libpointmatcher's
    MaxDensityDataPointsFilter: a point with density <= max_density stays; a denser one stays with probability
    max_density / density (scaled by 1 - nbSaturated / nbPoints -- an integer division, i.e. 1 unless every point is
    saturated -- for the points at the maximum density), drawn with std::rand() in input order.
    ``max_density_filter(points, knn, max_density)`` -> points', or with descriptors
    ``max_density_filter(points, descriptors, knn, max_density)`` -> (points', descriptors').  Extension."""
    ctx = kw.pop("ctx", None)
    if len(args) == 2:
        desc, (knn, max_density) = None, args
    elif len(args) == 3:
        desc, knn, max_density = _np.ascontiguousarray(args[0], _np.float32), args[1], args[2]
    else:
        raise TypeError("max_density_filter(points, [descriptors,] knn, max_density)")
    pts = _cloud23(points, "max_density_filter(points)")
    if len(pts) == 0:
        return pts if desc is None else (pts, desc)
    dens = knn_density(pts, knn, ctx=ctx)
    max_density = _np.float32(max_density)
    last = dens.max()
    n_sat = int((dens == last).sum())
    keep = _np.ones(len(pts), bool)
    for i in _np.nonzero(dens > max_density)[0]:        # input order; only the dense points draw a number
        r = _np.float32(_rand.rand()) / _np.float32(_GlibcRand.RAND_MAX)
        accept = _np.float32(max_density / dens[i])
        if dens[i] == last:
            accept = _np.float32(accept * _np.float32(1 - n_sat // len(pts)))
        keep[i] = r < accept
    return pts[keep].copy() if desc is None else (pts[keep].copy(), desc[keep].copy())


def density_filter(points, *args):
    """``pcl.density_filter(points[, descriptors], knn, min_density, max_density)`` (pcl.cpp:76-126, both overloads).
    The reference hands libpointmatcher's MaxDensityDataPointsFilter a ``minDensity`` parameter that filter does not
    have (pcl.cpp:90-92, 115-117); its registrar rejects parameters a module never reads, so on a non-empty cloud the
    reference call ends in ``InvalidParameter`` -- a RuntimeError in Python -- which is presumably why its only call
    site is commented out (feature_extraction.py:246).  This drop-in behaves the same: empty clouds come back
    unchanged (:78-79, :103-104), anything else raises with libpointmatcher's message.  ``max_density_filter`` is the
    working form."""
    if len(args) not in (3, 4):
        raise TypeError("density_filter(points, knn, min_density, max_density) or "
                        "density_filter(points, descriptors, knn, min_density, max_density)")
    pts = _np.asarray(points)
    if pts.ndim == 2 and pts.shape[0] == 0:
        return pts if len(args) == 3 else (pts, _np.asarray(args[0]))
    raise RuntimeError("Parameter minDensity for module MaxDensityDataPointsFilter was set but is not used")


class ICP(object):
    """``pcl.ICP`` (PM::ICP bound at pcl.cpp:184-213)."""

    def __init__(self, ctx=None):
        self._ctx = ctx
        # PM::ICP() starts without a chain (pcl.cpp:185); the SLAM node always calls loadFromYaml next (slam.py:99)
        self.params = None
        self.chain = None   # icp_config.IcpChain: params + the data-point filters (empty after setParams)

    def loadFromYaml(self, filename, strict=None, dims=2):
        """pcl.cpp:187-197.  ``dims=3`` (extension): the file is a chain for N x 3 clouds (``icp_config.parse_icp_chain``
        with ``dims=3``): its data-point filters and MinDist / MedianDist / Bound modules then run on N x 3 clouds.  A file that cannot be opened makes the reference print a message and fall back to
        PM::ICP::setDefault(): random sub-sampling of the reading, surface-normal sampling of the reference and a
        3-D point-to-plane chain -- not reproducible and not what any bruce_slam launch file intends.  Default
        (``strict`` True): an error instead of a silently different chain (deviations).

        ``strict=False``, or ``SONARFE_YAML_FALLBACK=shipped`` in the environment when ``strict`` is not given: behave
        like the reference AT THE CALL SITE (slam_ros.py:124-125 sees no exception) -- print the reference's exact
        line (pcl.cpp:192) and carry on with a default chain; the default installed here is the chain of the shipped
        ``config/icp.yaml`` (``icp_config.shipped_params``), since libpointmatcher's ``setDefault`` chain is 3-D and
        random and has no counterpart on this path."""
        if strict is None:
            strict = _os.environ.get("SONARFE_YAML_FALLBACK", "").strip().lower() != "shipped"
        try:
            with open(filename, "r") as fh:
                text = fh.read()
        except (IOError, OSError) as e:
            if not strict:
                print("Failed to load %s. Use default configuration." % filename)      # pcl.cpp:192, verbatim
                self.setParams(_cfg.shipped_params())
                return
            raise RuntimeError("ICP.loadFromYaml: cannot open %s (%s).  The reference would print 'Failed to load ... Use "
                               "default configuration.' and run libpointmatcher's setDefault() chain (random sampling + "
                               "surface normals), which this front end does not provide: fix the path, install a "
                               "chain with setParams(), or pass strict=False / set SONARFE_YAML_FALLBACK=shipped to "
                               "carry on with the chain of the shipped config/icp.yaml" % (filename, e))
        self.setChain(_cfg.parse_icp_chain(text, dims=dims))

    def setParams(self, params):
        """Extension: install an ``IcpParams`` directly (a chain without data-point filters)."""
        self.params = params
        self.chain = _cfg.IcpChain(params)

    def setChain(self, chain):
        """Extension: install an ``icp_config.IcpChain`` (what ``loadFromYaml`` parses): its reading filters run once
        on every distinct source cloud of a call, its reference filters once on every distinct target cloud, on the
        device and before any guess is applied; ICP then runs on the filtered clouds.  A job left with an empty cloud
        reports status 7, one whose octree stage would need more than 24 levels status 8 (T = the guess).  Its
        ``outliers`` (MinDist / MedianDist outlier filters, BoundTransformationChecker) run inside the ICP loop; a job
        the Bound checker stops reports status 9, "limit out of bounds" (T = the guess).  ``chain.dims`` says which clouds
        the chain was written for: a ``dims=3`` chain runs all of this on N x 3 clouds with 4 x 4 guesses (the rules with one
        more coordinate, no status 8) and is refused on N x 2 clouds; a ``dims=2`` chain with filters or those modules is
        refused on N x 3 clouds."""
        self.params = chain.params
        self.chain = chain

    def _stages(self):
        """(reading array, n, reference array, n) of the device stages, or None for a chain without filters"""
        ch = self.chain
        if ch is None or not ch.has_filters():
            return None
        rd, n_rd = ch.device_stages(ch.reading)
        rf, n_rf = ch.device_stages(ch.reference)
        return rd, n_rd, rf, n_rf

    def _outliers(self):
        """the chain's ``IcpOutliers`` (MinDist / MedianDist / Bound), or None when it lists none of them"""
        ch = self.chain
        return ch.outliers if ch is not None and ch.outliers.any() else None

    def _chain(self):
        if self.params is None:
            raise RuntimeError("ICP.compute before loadFromYaml / setParams: the chain is empty (PM::ICP() has no "
                               "default chain either, pcl.cpp:185)")
        return self.params

    def _call(self, ctx, shape, clouds, g, n, T, st, it):
        """One host-pointer ICP call of ``shape`` ("guesses", "pairs", "jobs"; ``clouds`` = its cloud arguments).  The
        chain picks the entry point: no stages and no outliers -> the plain one; outliers -> ``_chain_ext``; stages
        only -> ``_chain``."""
        stages, ox = self._stages(), self._outliers()
        name, extra = "sfe_icp_compute_" + shape, ()
        if ox is not None:
            name, extra = name + "_chain_ext", (_C.byref(ox),) + (stages or (None, 0, None, 0))
        elif stages is not None:
            name, extra = name + "_chain", stages
        args = (ctx.handle, _C.byref(self.params)) + tuple(extra) + tuple(clouds) + (
            _L.ptr(g, _C.c_float), n, _L.ptr(T, _C.c_float), _L.ptr(st, _C.c_int32), _L.ptr(it, _C.c_int32))
        with ctx.lock:
            ctx._check(getattr(ctx.lib, name)(*args))

    @staticmethod
    def _guess(guess):
        g = _np.asarray(guess, _np.float32)
        if g.shape == (4, 4):
            raise NotImplementedError("4 x 4 guesses (3-D ICP) are outside the sonar front-end path")
        if g.shape != (3, 3):
            raise TypeError("ICP.compute: guess must be 3 x 3, got %r" % (g.shape,))
        return _np.ascontiguousarray(g)

    def _chain2(self, what):
        """a 2-D call: the 3-D point-to-plane minimiser and a chain written for N x 3 clouds are refused before anything
        reaches the library"""
        if self._chain().minimizer == 2:
            raise NotImplementedError("%s: PointToPlaneErrorMinimizer {force2D: 0} on N x 2 clouds: libpointmatcher would "
                                      "run its 2-D form there; say force2D: 1 (minimizer = 1) for 2-D clouds" % what)
        if self._chain().minimizer == 3:
            raise NotImplementedError("%s: PointToPlaneErrorMinimizer {force4DOF: 1} on N x 2 clouds: yaw and translation "
                                      "of a 3-D cloud have no 2-D form; say force2D: 1 (minimizer = 1) for 2-D clouds" % what)
        ch = self.chain
        if ch is not None and ch.dims == 3:
            raise NotImplementedError("%s: a chain written for N x 3 clouds (dims = 3) on N x 2 clouds: its dim: 2, zMin / "
                                      "zMax, 8-way octree and Bound rotation have no 2-D meaning; parse the chain with "
                                      "dims = 2 for 2-D clouds" % what)
        if ch is not None and any(isinstance(s, _L.IcpDpf) and s.kind in (_L.DPF_MAX_DIST, _L.DPF_MIN_DIST) and s.dim == 2
                                  for s in ch.reading + ch.reference):
            raise NotImplementedError("%s: a data-point filter stage with dim: 2 (the z axis) on N x 2 clouds: the device "
                                      "stages of a 2-D chain take dim -1, 0 or 1" % what)

    # ---- N x 3 clouds with 4 x 4 guesses: the point-to-point or 3-D point-to-plane chain on sfe_icp3_compute_jobs ----
    @staticmethod
    def _is3d(clouds, guess_shapes, what):
        """True when the call is a 3-D one: every cloud N x 3 and every guess 4 x 4.  False: leave it to the 2-D path
        (whose ``_cloud`` / ``_guess`` refuse what it does not take).  Mixed input raises here."""
        widths = set(_np.shape(c)[1] for c in clouds if _np.ndim(c) == 2 and _np.shape(c)[1] in (2, 3))
        if len(widths) == 2:
            raise NotImplementedError("%s: source and target of different widths (N x 2 with N x 3): libpointmatcher "
                                      "matches clouds of one dimension only" % what)
        if widths != {3}:
            return False
        if any(tuple(s) == (3, 3) for s in guess_shapes):
            raise NotImplementedError("%s: N x 3 clouds with a 3 x 3 guess: a 3-D cloud needs a 4 x 4 transform "
                                      "(PM::ICP::compute checks the guess against the cloud's dimension)" % what)
        for s in guess_shapes:
            if tuple(s) != (4, 4):
                raise TypeError("%s: guess must be 4 x 4 for N x 3 clouds, got %r" % (what, tuple(s)))
        return True

    def _chain3(self, what):
        """the chain's params for a 3-D call; the filters and modules of a chain that was not written for N x 3 clouds
        (``dims != 3``) are refused"""
        p = self._chain()
        dims3 = self.chain is not None and self.chain.dims == 3
        if self._stages() is not None and not dims3:
            raise NotImplementedError("%s: data-point filters on N x 3 clouds: the device stages of a chain are 2-D "
                                      "(sfe_icp_dpf); filter the clouds with pcl.downsample / remove_outlier first" % what)
        if self._outliers() is not None and not dims3:
            raise NotImplementedError("%s: MinDist / MedianDist outlier filters and the Bound checker on N x 3 clouds: "
                                      "the 3-D kernel runs the modules of the shipped icp.yaml only" % what)
        if p.minimizer == 1:
            raise NotImplementedError("%s: PointToPlaneErrorMinimizer {force2D: 1} on N x 3 clouds: its normal equations "
                                      "are the 2-D ones; 3-D clouds take the point-to-point minimiser or force2D: 0 "
                                      "(minimizer = 2)" % what)
        return p

    def _ext3(self):
        """the arguments a ``*_chain_ext`` call of a dims = 3 chain puts behind the params (outliers, reading stages,
        reference stages), or None when the chain lists neither stages nor modules: the plain entry point then"""
        stages, ox = self._stages(), self._outliers()
        if stages is None and ox is None:
            return None
        return (None if ox is None else _C.byref(ox),) + (stages or (None, 0, None, 0))

    def _call3(self, ctx, src, tgt, jobs4, g, T, st, it):
        n = len(jobs4)
        ext = self._ext3()
        if ext is not None:
            with ctx.lock:
                ctx._check(ctx.lib.sfe_icp3_compute_jobs_chain_ext(
                    ctx.handle, _C.byref(self.params), *(ext + (
                        _L.ptr(src, _C.c_float), len(src), _L.ptr(tgt, _C.c_float), len(tgt), _L.ptr(jobs4, _C.c_int32),
                        _L.ptr(g, _C.c_float), n, _L.ptr(T, _C.c_float), _L.ptr(st, _C.c_int32), _L.ptr(it, _C.c_int32)))))
            return
        with ctx.lock:
            ctx._check(ctx.lib.sfe_icp3_compute_jobs(ctx.handle, _C.byref(self.params), _L.ptr(src, _C.c_float), len(src),
                                                     _L.ptr(tgt, _C.c_float), len(tgt), _L.ptr(jobs4, _C.c_int32),
                                                     _L.ptr(g, _C.c_float), n, _L.ptr(T, _C.c_float),
                                                     _L.ptr(st, _C.c_int32), _L.ptr(it, _C.c_int32)))

    def _pairs3(self, srcs, tgts, guesses, what):
        """3-D jobs (source cloud, target cloud, guess) -> (messages, T [n x 4 x 4], iterations)"""
        self._chain3(what)
        ctx = self._ctx or _L.default_context()
        srcs = [_cloud23(s, what + "(source)") for s in srcs]
        tgts = [_cloud23(t, what + "(target)") for t in tgts]
        if any(len(s) == 0 for s in srcs) or any(len(t) == 0 for t in tgts):
            raise RuntimeError("%s: empty point cloud (libpointmatcher would throw)" % what)
        n = len(guesses)
        g = _np.ascontiguousarray(_np.stack([_np.asarray(x, _np.float32) for x in guesses]), _np.float32)
        # a cloud handed in several times (compute_batch: one pair, many guesses) goes up once
        pools, jobs4 = ([], []), _np.zeros((n, 4), _np.int32)
        for side, clouds in enumerate((srcs, tgts)):
            seen, off = {}, 0
            for j, c in enumerate(clouds):
                if id(c) not in seen:
                    seen[id(c)] = off
                    pools[side].append(c)
                    off += len(c)
                jobs4[j, 2 * side], jobs4[j, 2 * side + 1] = seen[id(c)], len(c)
        src = _np.ascontiguousarray(_np.concatenate(pools[0]), _np.float32)
        tgt = _np.ascontiguousarray(_np.concatenate(pools[1]), _np.float32)
        T = _np.zeros((n, 4, 4), _np.float32)
        st = _np.zeros(n, _np.int32)
        it = _np.zeros(n, _np.int32)
        self._call3(ctx, src, tgt, jobs4, g, T, st, it)
        msgs = [_L.ICP_STATUS_MESSAGES.get(int(s), "ICP failure %d" % s) for s in st]
        return msgs, T, it

    def compute(self, source, target, guess):
        """-> (message, T): ("success", T 3x3 float32) or (ConvergenceError text, guess); N x 3 clouds with a 4 x 4
        guess: T 4x4."""
        msgs, Ts, _ = self.compute_batch(source, target, [guess])
        return msgs[0], Ts[0]

    def compute_batch(self, source, target, guesses):
        """Many initial guesses on one cloud pair in one launch.
        -> (messages [n], T [n x 3 x 3] float32, iterations [n]); N x 3 clouds with 4 x 4 guesses: T [n x 4 x 4]"""
        self._chain()
        if self._is3d([source, target], [_np.shape(x) for x in guesses], "ICP.compute"):
            src, tgt = _cloud23(source, "ICP.compute(source)"), _cloud23(target, "ICP.compute(target)")
            return self._pairs3([src] * len(guesses), [tgt] * len(guesses), guesses, "ICP.compute")
        ctx = self._ctx or _L.default_context()
        src = _cloud(source, "ICP.compute(source)")
        tgt = _cloud(target, "ICP.compute(target)")
        self._chain2("ICP.compute")
        g = _np.ascontiguousarray(_np.stack([self._guess(x) for x in guesses]), _np.float32)
        n = len(g)
        if len(src) == 0 or len(tgt) == 0:
            raise RuntimeError("ICP.compute: empty point cloud (libpointmatcher would throw)")
        T = _np.zeros((n, 3, 3), _np.float32)
        st = _np.zeros(n, _np.int32)
        it = _np.zeros(n, _np.int32)
        self._call(ctx, "guesses", (_L.ptr(src, _C.c_float), len(src), _L.ptr(tgt, _C.c_float), len(tgt)), g, n, T, st, it)
        msgs = [_L.ICP_STATUS_MESSAGES.get(int(s), "ICP failure %d" % s) for s in st]
        return msgs, T, it

    def compute_pairs(self, sources, targets, guesses):
        """Many independent (source, target, guess) scan matches in ONE launch (extension; the job
        farm's unit).  -> (messages [n], T [n x 3 x 3] float32, iterations [n]); N x 3 clouds with 4 x 4 guesses:
        T [n x 4 x 4]"""
        self._chain()
        ctx = self._ctx or _L.default_context()
        n = len(sources)
        if not (len(targets) == n and len(guesses) == n):
            raise TypeError("compute_pairs: %d sources, %d targets, %d guesses" % (n, len(targets), len(guesses)))
        if n == 0:
            return [], _np.zeros((0, 3, 3), _np.float32), _np.zeros(0, _np.int32)
        if self._is3d(list(sources) + list(targets), [_np.shape(x) for x in guesses], "ICP.compute_pairs"):
            return self._pairs3(sources, targets, guesses, "ICP.compute_pairs")
        srcs = [_cloud(s, "ICP.compute_pairs(source)") for s in sources]
        tgts = [_cloud(t, "ICP.compute_pairs(target)") for t in targets]
        self._chain2("ICP.compute_pairs")
        if any(len(s) == 0 for s in srcs) or any(len(t) == 0 for t in tgts):
            raise RuntimeError("ICP.compute_pairs: empty point cloud (libpointmatcher would throw)")
        so = _np.zeros(n + 1, _np.int32)
        to = _np.zeros(n + 1, _np.int32)
        so[1:] = _np.cumsum([len(s) for s in srcs])
        to[1:] = _np.cumsum([len(t) for t in tgts])
        src = _np.ascontiguousarray(_np.concatenate(srcs), _np.float32)
        tgt = _np.ascontiguousarray(_np.concatenate(tgts), _np.float32)
        g = _np.ascontiguousarray(_np.stack([self._guess(x) for x in guesses]), _np.float32)
        T = _np.zeros((n, 3, 3), _np.float32)
        st = _np.zeros(n, _np.int32)
        it = _np.zeros(n, _np.int32)
        self._call(ctx, "pairs", (_L.ptr(src, _C.c_float), _L.ptr(so, _C.c_int32), _L.ptr(tgt, _C.c_float),
                                  _L.ptr(to, _C.c_int32)), g, n, T, st, it)
        msgs = [_L.ICP_STATUS_MESSAGES.get(int(s), "ICP failure %d" % s) for s in st]
        return msgs, T, it

    def compute_jobs(self, src_all, tgt_all, jobs4, guesses9, out=None):
        """Scan matches named by a job table over two cloud pools (extension; what a farm worker runs per
        chunk): src_all / tgt_all = clouds back to back (N x 2 float32), jobs4 = n x (src_start, n_src,
        tgt_start, n_tgt) in points, guesses9 = n x 9.  Jobs may share clouds; jobs naming the same target slice
        share its preparation.  -> (status int32 [n], T [n x 3 x 3] float32, iterations int32 [n]); the three
        arrays may be handed in preallocated (``out=(status, T, iters)``, e.g. views of shared memory).  N x 3 pools
        take n x 16 guesses (4 x 4 row-major) and return T [n x 4 x 4]."""
        self._chain()
        ctx = self._ctx or _L.default_context()
        n_g = _np.size(guesses9) // max(len(_np.reshape(_np.asarray(jobs4), (-1, 4))), 1)
        if self._is3d([src_all, tgt_all], [(4, 4) if n_g == 16 else (3, 3) if n_g == 9 else (n_g,)], "ICP.compute_jobs"):
            self._chain3("ICP.compute_jobs")
            src = _cloud23(src_all, "ICP.compute_jobs(src_all)")
            tgt = _cloud23(tgt_all, "ICP.compute_jobs(tgt_all)")
            jobs4 = _np.ascontiguousarray(jobs4, _np.int32).reshape(-1, 4)
            n = len(jobs4)
            g = _np.ascontiguousarray(guesses9, _np.float32).reshape(n, 16)
            st, T, it = out if out is not None else (_np.zeros(n, _np.int32), _np.zeros((n, 4, 4), _np.float32),
                                                     _np.zeros(n, _np.int32))
            for a, shape, dt in ((st, (n,), _np.int32), (T, (n, 4, 4), _np.float32), (it, (n,), _np.int32)):
                if not (isinstance(a, _np.ndarray) and a.shape == shape and a.dtype == dt and a.flags.c_contiguous):
                    raise TypeError("ICP.compute_jobs: out= wants C-contiguous (status int32 [n], T float32 [n x 4 x 4], "
                                    "iterations int32 [n]) for N x 3 clouds")
            if n and ((jobs4[:, 1] <= 0).any() or (jobs4[:, 3] <= 0).any()):
                raise RuntimeError("ICP.compute_jobs: empty point cloud (libpointmatcher would throw)")
            self._call3(ctx, src, tgt, jobs4, g, T, st, it)
            return st, T, it
        if n_g == 16:
            raise NotImplementedError("ICP.compute_jobs: 4 x 4 guesses (n x 16) with N x 2 clouds: a 2-D cloud needs "
                                      "3 x 3 transforms (n x 9)")
        src = _cloud(src_all, "ICP.compute_jobs(src_all)")
        tgt = _cloud(tgt_all, "ICP.compute_jobs(tgt_all)")
        self._chain2("ICP.compute_jobs")
        jobs4 = _np.ascontiguousarray(jobs4, _np.int32).reshape(-1, 4)
        n = len(jobs4)
        g = _np.ascontiguousarray(guesses9, _np.float32).reshape(n, 9)
        if out is None:
            st, T, it = _np.zeros(n, _np.int32), _np.zeros((n, 3, 3), _np.float32), _np.zeros(n, _np.int32)
        else:
            st, T, it = out
        if n and ((jobs4[:, 1] <= 0).any() or (jobs4[:, 3] <= 0).any()):
            raise RuntimeError("ICP.compute_jobs: empty point cloud (libpointmatcher would throw)")
        self._call(ctx, "jobs", (_L.ptr(src, _C.c_float), len(src), _L.ptr(tgt, _C.c_float), len(tgt),
                                 _L.ptr(jobs4, _C.c_int32)), g, n, T, st, it)
        return st, T, it

    def getCovariance(self):
        """errorMinimizer->getCovariance() (pcl.cpp:213).  For the shipped point-to-point chain libpointmatcher's
        base ``ErrorMinimizer::getCovariance`` logs a warning and returns ``Matrix::Zero(6, 6)`` (restated from its
        published source, unpinned like the rest of pcl.cpp's third-party behaviour): 6 x 6 float32 zeros here.
        ``PointToPlaneErrorMinimizer`` overrides it with Censi's estimate from its 3-D normal equations and
        ``sensorStdDev``; the reference cannot run that chain (icp.yaml configures no normals) and the 2-D form
        is not defined anywhere, so a point-to-plane chain raises instead of returning a made-up matrix.  No
        caller in the reference reads either (grep)."""
        if self._chain().minimizer in (1, 2, 3):
            raise NotImplementedError("ICP.getCovariance for a point-to-plane chain: libpointmatcher's Censi estimate "
                                      "is 3-D only and the reference never runs this chain; use "
                                      "SLAM.compute_icp_with_cov's sampled covariance (slam.py:325-387)")
        return _np.zeros((6, 6), _np.float32)
