"""Parser for the libpointmatcher ICP chain YAML the reference ships
(bruce_slam/config/icp.yaml:1-31, loaded by ``ICP.loadFromYaml``, pcl.cpp:187-197).

The file is accepted byte for byte.  Supported modules (anything else is rejected loudly --
silently ignoring a filter would change the pose):

    readingDataPointsFilters / referenceDataPointsFilters (``parse_icp_chain`` only; ``parse_icp_yaml``
                       refuses any), at most MAX_STAGES per side, 2-D:
                       MaxDistDataPointsFilter {dim: -1|0|1, maxDist}, MinDistDataPointsFilter {dim, minDist},
                       BoundingBoxDataPointsFilter {xMin, xMax, yMin, yMax, zMin, zMax, removeInside},
                       OctreeGridDataPointsFilter {maxSizeByNode, samplingMethod: 3, maxPointByNode: 1, buildParallel},
                       SurfaceNormalDataPointsFilter {knn, epsilon: 0, keep*} -- last reference stage of a
                       point-to-plane chain only, where it is ``normals_knn``
    matcher            KDTreeMatcher {knn: 1, epsilon: 0, maxDist}
    outlierFilters     MaxDistOutlierFilter {maxDist}, TrimmedDistOutlierFilter {ratio}; with ``parse_icp_chain``
                       also MinDistOutlierFilter {minDist}, MedianDistOutlierFilter {factor}, NullOutlierFilter
                       (each at most once, any order; the weights are the product of the filters')
    errorMinimizer     PointToPointErrorMinimizer | PointToPlaneErrorMinimizer {force2D: 1} (the 2-D form, N x 2 clouds);
                       with ``parse_icp_chain`` also PointToPlaneErrorMinimizer {force2D: 0} or without parameters
                       (libpointmatcher's default): the 3-D form, ``minimizer = 2``, N x 3 clouds only; with
                       ``parse_icp_chain(text, dims=3)`` also {force4DOF: 1} (``force2D: 0`` may stand beside it): the 3-D
                       form solved for yaw and translation only, ``minimizer = 3``, N x 3 clouds only
    transformationCheckers  CounterTransformationChecker {maxIterationCount},
                            DifferentialTransformationChecker {minDiffRotErr, minDiffTransErr,
                                                               smoothLength};
                            with ``parse_icp_chain`` also BoundTransformationChecker {maxRotationNorm,
                                                               maxTranslationNorm} (its place in the list is kept)
    inspector          NullInspector
    logger             NullLogger

The outlier filters and the checker only ``parse_icp_chain`` takes live in ``IcpChain.outliers`` (``IcpOutliers``, the
mirror of ``sfe_icp_outliers``; its comment in include/sonarfe.h states their rules), not in ``IcpParams``.  Every
route ICP takes runs the whole chain: ``pcl.ICP``, ``store.CloudStore.icp``, ``replay.FrontEnd``,
``chained.SessionBatch`` and ``farm.IcpFarm`` all accept an ``IcpChain`` (the farm sends ``IcpChain.as_dict()``).

Data-point filters, restated from libpointmatcher's published ICP::compute / computeWithTransformedReference and
the filters' sources (UNPINNED, like the rest of pcl.cpp's third-party behaviour; tools/pin_thirdparty.py writes
the fixture that would pin them):
  * the reading filters run once on the reading in its own frame, before the guess is applied; the reference
    filters once on the reference in its own frame; the reference mean used for centring is that of the FILTERED
    reference.  So ICP with a chain is ICP on the filtered clouds.  (Should the library turn out to centre on the
    unfiltered mean, only float rounding differs: the centring cancels out of the solved transformation.)
  * stages run in the order listed and keep the relative order of the points they keep.
  * MaxDist keeps a point when dim -1: sqrtf(x*x + y*y) < |maxDist|, dim 0 / 1: x / y < maxDist (signed);
    MinDist when dim -1: the norm > |minDist|, dim 0 / 1: |x| / |y| > |minDist| (every product / sum in float);
    BoundingBox when (xMin < x < xMax and yMin < y < yMax) != removeInside (defaults +-1, removeInside 1);
    OctreeGrid {samplingMethod: 3, maxPointByNode: 1} is ``pcl.downsample(cloud, maxSizeByNode)``.
  * refused: the random filters (RandomSampling, MaxPointCount, MaxDensity: not reproducible), OctreeGrid with
    another sampling method (libpointmatcher's default 0, FirstPoint, is not restated) or maxPointByNode != 1,
    dim >= 2 (3-D), a SurfaceNormal with epsilon != 0 or maxDist, or anywhere but the last reference stage of a
    point-to-plane chain, unknown parameter names, readingStepDataPointsFilters.

Chains for N x 3 clouds: a chain says which dimension it was written for.  ``parse_icp_chain(text, dims=3)`` (and
``IcpChain(..., dims=3)``) makes a 3-D chain: ``dim: 2`` (the z axis) is accepted, BoundingBox uses zMin / zMax, OctreeGrid
is the 8-way tree of ``pcl.downsample`` on N x 3 clouds, the Bound checker measures the 3-D rotation angle, and
``PointToPlaneErrorMinimizer {force4DOF: 1}`` is read (``minimizer = 3``; a 2-D chain keeps refusing ``force4DOF``, with
either value, wherever ``force2D: 1`` does not stand beside it -- beside ``force2D: 1`` a 2-D chain examines no other
parameter, as before, and a 3-D chain refuses ``force4DOF: 1``).  ``pcl.ICP``
and ``store.CloudStore3.icp`` run such a chain's filters and modules on N x 3 clouds and refuse it on N x 2 clouds; a chain
with ``dims=2`` (the default) stays what it was, refused with filters or extra modules on N x 3 clouds.  The stage rules are
the ones above with one more coordinate (include/sonarfe.h at ``sfe_icp3_filter_clouds_dev``).
"""
import math

import yaml

from ._lib import (DPF_BOUNDING_BOX, DPF_MAX_DIST, DPF_MAX_STAGES, DPF_MIN_DIST, DPF_OCTREE_GRID, IcpDpf,
                   IcpOutliers, IcpParams)

MAX_STAGES = DPF_MAX_STAGES     # data-point filter stages per side of a chain


class IcpConfigError(ValueError):
    pass


def shipped_params(**over):
    """The chain of bruce_slam/config/icp.yaml as shipped."""
    p = dict(matcher_max_dist=10.0, use_max_dist_filter=1, max_dist_filter=3.0,
             use_trimmed_filter=1, trim_ratio=0.8, minimizer=0, max_iter=40, use_diff_checker=1,
             min_diff_rot=0.01, min_diff_trans=0.1, smooth_len=4, normals_knn=10)
    p.update(over)
    return IcpParams(**p)


def _single(node, what):
    """YAML module node -> (name, params dict).  Accepts 'Name' or {'Name': {...}}."""
    if isinstance(node, str):
        return node, {}
    if isinstance(node, dict) and len(node) == 1:
        (name, params), = node.items()
        return name, dict(params or {})
    raise IcpConfigError("cannot parse %s entry: %r" % (what, node))


def _load(text):
    doc = yaml.safe_load(text) or {}
    known = {"readingDataPointsFilters", "referenceDataPointsFilters", "matcher", "outlierFilters",
             "errorMinimizer", "transformationCheckers", "inspector", "logger",
             "readingStepDataPointsFilters"}
    for key in doc:
        if key not in known:
            raise IcpConfigError("unknown ICP chain section %r" % key)
    return doc


def parse_icp_yaml(text):
    """YAML text -> IcpParams.  Refuses any data-point filter (``parse_icp_chain`` takes them)."""
    doc = _load(text)
    for key in ("readingDataPointsFilters", "referenceDataPointsFilters", "readingStepDataPointsFilters"):
        if doc.get(key):
            raise IcpConfigError("%s are not supported by parse_icp_yaml (parse_icp_chain takes them)" % key)
    return _params(doc)


# modules only parse_icp_chain takes (their settings go to IcpChain.outliers)
_CHAIN_ONLY = {"MinDistOutlierFilter", "MedianDistOutlierFilter", "NullOutlierFilter", "BoundTransformationChecker"}


def _positive(name, key, v):
    v = float(v)
    if not (math.isfinite(v) and v > 0.0):
        raise IcpConfigError("%s: %s must be finite and > 0 (got %r)" % (name, key, v))
    return v


def _params(doc, ox=None, dims=2):
    """the sections other than the data-point filters -> IcpParams; ``ox`` (an IcpOutliers to fill: parse_icp_chain)
    takes the modules of _CHAIN_ONLY and the 3-D point-to-plane minimiser, without it they are refused; ``dims`` = 3
    (a chain for N x 3 clouds) also takes ``force4DOF``"""
    p = dict(matcher_max_dist=float("inf"), use_max_dist_filter=0, max_dist_filter=0.0,
             use_trimmed_filter=0, trim_ratio=1.0, minimizer=0, max_iter=40, use_diff_checker=0,
             min_diff_rot=0.001, min_diff_trans=0.01, smooth_len=3, normals_knn=10)

    if "matcher" in doc and doc["matcher"] is not None:
        name, mp = _single(doc["matcher"], "matcher")
        if name != "KDTreeMatcher":
            raise IcpConfigError("unsupported matcher %r" % name)
        if int(mp.get("knn", 1)) != 1:
            raise IcpConfigError("KDTreeMatcher.knn must be 1")
        if float(mp.get("epsilon", 0)) != 0:
            raise IcpConfigError("KDTreeMatcher.epsilon must be 0 (exact search)")
        unknown = set(mp) - {"knn", "epsilon", "maxDist", "searchType"}
        if unknown:
            raise IcpConfigError("unsupported KDTreeMatcher parameters %r" % sorted(unknown))
        p["matcher_max_dist"] = float(mp.get("maxDist", float("inf")))

    listed = set()
    for node in doc.get("outlierFilters") or []:
        name, fp = _single(node, "outlierFilters")
        if name in _CHAIN_ONLY and ox is None:
            raise IcpConfigError("%s is not supported by parse_icp_yaml (parse_icp_chain takes it)" % name)
        if name in listed:
            raise IcpConfigError("%s listed twice" % name)
        listed.add(name)
        if name == "MaxDistOutlierFilter":
            p["use_max_dist_filter"] = 1
            p["max_dist_filter"] = float(fp.get("maxDist", 1.0))
        elif name == "TrimmedDistOutlierFilter":
            p["use_trimmed_filter"] = 1
            p["trim_ratio"] = float(fp.get("ratio", 0.85))
        elif name == "MinDistOutlierFilter":
            _known_params(name, fp, ("minDist",))
            v = float(fp.get("minDist", 1.0))
            if not v >= 0.0:
                raise IcpConfigError("%s: minDist must be >= 0 (got %r)" % (name, v))
            ox.use_min_dist, ox.min_dist = 1, v
        elif name == "MedianDistOutlierFilter":
            _known_params(name, fp, ("factor",))
            ox.use_median, ox.median_factor = 1, _positive(name, "factor", fp.get("factor", 3.0))
        elif name == "NullOutlierFilter":
            _known_params(name, fp, ())      # keeps every pair
        else:
            raise IcpConfigError("unsupported outlier filter %r" % name)

    if doc.get("errorMinimizer") is not None:
        name, ep = _single(doc["errorMinimizer"], "errorMinimizer")
        if name == "PointToPointErrorMinimizer":
            p["minimizer"] = 0
        elif name == "PointToPlaneErrorMinimizer":
            if int(ep.get("force2D", 0)) == 1:
                if dims == 3 and int(ep.get("force4DOF", 0)) == 1:
                    raise IcpConfigError("PointToPlaneErrorMinimizer: force2D: 1 and force4DOF: 1 name two different "
                                         "systems; give one of them")
                p["minimizer"] = 1
            elif ox is not None and int(ep.get("force2D", 0)) == 0:
                # sensorStdDev, ...: a parameter that is not restated would change the pose silently.  force4DOF is a
                # statement about the z axis (like dim: 2 and zMin / zMax): a chain written for N x 3 clouds may make it
                _known_params(name, ep, ("force2D", "force4DOF") if dims == 3 else ("force2D",))
                # 2: libpointmatcher's default, the 3-D normal equations; 3: their yaw-and-translation form (N x 3 clouds)
                p["minimizer"] = 3 if int(ep.get("force4DOF", 0)) == 1 else 2
            else:
                raise IcpConfigError("PointToPlaneErrorMinimizer needs force2D: 1 (clouds are 2-D)")
        else:
            raise IcpConfigError("unsupported error minimizer %r" % name)

    seen_counter = seen_diff = False
    for node in doc.get("transformationCheckers") or []:
        name, cp = _single(node, "transformationCheckers")
        if name in _CHAIN_ONLY and ox is None:
            raise IcpConfigError("%s is not supported by parse_icp_yaml (parse_icp_chain takes it)" % name)
        if name == "CounterTransformationChecker":
            seen_counter = True
            p["max_iter"] = int(cp.get("maxIterationCount", 40))
        elif name == "BoundTransformationChecker":
            if ox.use_bound:
                raise IcpConfigError("%s listed twice" % name)
            _known_params(name, cp, ("maxRotationNorm", "maxTranslationNorm"))
            ox.use_bound = 1
            ox.max_rotation_norm = _positive(name, "maxRotationNorm", cp.get("maxRotationNorm", 1.0))
            ox.max_translation_norm = _positive(name, "maxTranslationNorm", cp.get("maxTranslationNorm", 1.0))
            # where it runs among the others: after a Counter / a Differential listed before it
            ox.bound_order = (1 if seen_counter else 0) | (2 if seen_diff else 0)
        elif name == "DifferentialTransformationChecker":
            seen_diff = True
            p["use_diff_checker"] = 1
            p["min_diff_rot"] = float(cp.get("minDiffRotErr", 0.001))
            p["min_diff_trans"] = float(cp.get("minDiffTransErr", 0.001))
            p["smooth_len"] = int(cp.get("smoothLength", 3))
        else:
            raise IcpConfigError("unsupported transformation checker %r" % name)

    for key, ok in (("inspector", "NullInspector"), ("logger", "NullLogger")):
        if doc.get(key) is not None:
            name, _ = _single(doc[key], key)
            if name != ok:
                raise IcpConfigError("unsupported %s %r" % (key, name))
    return IcpParams(**p)


class SurfaceNormalStage(object):
    """SurfaceNormalDataPointsFilter as the last reference stage of a point-to-plane chain: keeps every point; its
    ``knn`` is the chain's ``normals_knn`` (the neighbours, the point itself included, of the PCA normals)."""

    def __init__(self, knn):
        self.knn = int(knn)

    def __repr__(self):
        return "SurfaceNormalStage(knn=%d)" % self.knn

    def __eq__(self, other):
        return isinstance(other, SurfaceNormalStage) and other.knn == self.knn


class IcpChain(object):
    """A parsed ICP chain: ``params`` (IcpParams), ``reading`` and ``reference`` (lists of data-point filter stages:
    ``IcpDpf`` structures, and on the reference side possibly a final ``SurfaceNormalStage``), ``outliers``
    (IcpOutliers: MinDist / MedianDist outlier filters and the Bound checker; all zero when none is listed), ``dims`` (2
    or 3: the dimension of the clouds the chain was written for; it decides what ``dim: 2``, zMin / zMax, the octree and
    the Bound checker's rotation mean)."""

    def __init__(self, params, reading=(), reference=(), outliers=None, dims=2):
        if dims not in (2, 3):
            raise IcpConfigError("IcpChain: dims must be 2 or 3 (got %r)" % (dims,))
        self.params = params
        self.reading = list(reading)
        self.reference = list(reference)
        self.outliers = outliers if outliers is not None else IcpOutliers()
        self.dims = int(dims)

    @staticmethod
    def device_stages(stages):
        """the stages the device runs (SurfaceNormal keeps every point and is ``normals_knn``: a chain whose only stage
        it is has none, which is what a 3-D point-to-plane chain looks like) -> (ctypes array of IcpDpf or None, count)"""
        dev = [s for s in stages if isinstance(s, IcpDpf)]
        if not dev:
            return None, 0
        arr = (IcpDpf * len(dev))()
        for i, st in enumerate(dev):
            arr[i] = st
        return arr, len(dev)

    def has_filters(self):
        return any(isinstance(s, IcpDpf) for s in self.reading + self.reference)

    def has_modules(self):
        """True when the chain lists anything ``IcpParams`` cannot carry: a data-point filter the device runs, or an
        outlier filter / checker of ``outliers``"""
        return self.has_filters() or self.outliers.any()

    def as_dict(self):
        """plain, picklable values (what a farm worker receives); ``IcpChain.from_dict`` rebuilds the chain exactly"""
        d = {"params": self.params.as_dict(), "reading": [_stage_dict(s) for s in self.reading],
             "reference": [_stage_dict(s) for s in self.reference], "outliers": self.outliers.as_dict()}
        if self.dims == 3:      # (a 2-D chain's dictionary is what it always was)
            d["dims"] = 3
        return d

    @staticmethod
    def from_dict(d):
        return IcpChain(IcpParams(**d["params"]), [_stage_of(x) for x in d["reading"]],
                        [_stage_of(x) for x in d["reference"]], IcpOutliers(**d["outliers"]), dims=d.get("dims", 2))

    def __eq__(self, other):
        return isinstance(other, IcpChain) and self.as_dict() == other.as_dict()

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def __repr__(self):
        return "IcpChain(%r)" % (self.as_dict(),)


def _stage_dict(st):
    if isinstance(st, SurfaceNormalStage):
        return {"stage": "SurfaceNormal", "knn": st.knn}
    return {"stage": "dpf", "kind": st.kind, "dim": st.dim, "remove_inside": st.remove_inside, "f": list(st.f)}


def _stage_of(d):
    if d["stage"] == "SurfaceNormal":
        return SurfaceNormalStage(d["knn"])
    if d["stage"] != "dpf":
        raise IcpConfigError("unknown chain stage %r" % (d["stage"],))
    st = IcpDpf()
    st.kind, st.dim, st.remove_inside = d["kind"], d["dim"], d["remove_inside"]
    for i, v in enumerate(d["f"]):
        st.f[i] = v
    return st


_RANDOM = {"RandomSamplingDataPointsFilter", "MaxPointCountDataPointsFilter", "MaxDensityDataPointsFilter"}


def _known_params(name, fp, allowed):
    unknown = set(fp) - set(allowed)
    if unknown:
        raise IcpConfigError("%s: unsupported parameters %r" % (name, sorted(unknown)))


def _dim(name, fp, dims=2):
    dim = int(fp.get("dim", -1))
    if dims == 3:
        if dim > 2 or dim < -1:
            raise IcpConfigError("%s: dim %d is not -1, 0, 1 or 2" % (name, dim))
        return dim
    if dim >= 2:
        raise IcpConfigError("%s: dim %d is a 3-D axis (the sonar clouds are 2-D)" % (name, dim))
    if dim < -1:
        raise IcpConfigError("%s: dim %d is not -1, 0 or 1" % (name, dim))
    return dim


def _stage(name, fp, dims=2):
    """one YAML data-point filter entry -> IcpDpf or SurfaceNormalStage (defaults: libpointmatcher's)"""
    if name in _RANDOM:
        raise IcpConfigError("%s draws random numbers: results would not be reproducible" % name)
    st = IcpDpf()
    if name == "MaxDistDataPointsFilter":
        _known_params(name, fp, ("dim", "maxDist"))
        st.kind, st.dim, st.f[0] = DPF_MAX_DIST, _dim(name, fp, dims), float(fp.get("maxDist", 1.0))
    elif name == "MinDistDataPointsFilter":
        _known_params(name, fp, ("dim", "minDist"))
        st.kind, st.dim, st.f[0] = DPF_MIN_DIST, _dim(name, fp, dims), float(fp.get("minDist", 1.0))
    elif name == "BoundingBoxDataPointsFilter":
        keys = ("xMin", "xMax", "yMin", "yMax", "zMin", "zMax")
        _known_params(name, fp, keys + ("removeInside",))
        st.kind, st.dim = DPF_BOUNDING_BOX, -1
        st.remove_inside = 1 if int(fp.get("removeInside", 1)) else 0
        for i, k in enumerate(keys):
            st.f[i] = float(fp.get(k, -1.0 if k.endswith("Min") else 1.0))
    elif name == "OctreeGridDataPointsFilter":
        _known_params(name, fp, ("maxSizeByNode", "samplingMethod", "maxPointByNode", "buildParallel"))
        if int(fp.get("samplingMethod", 0)) != 3:
            raise IcpConfigError("%s needs samplingMethod: 3 (medoid); libpointmatcher's default 0 (FirstPoint) and the "
                                 "other methods are not restated" % name)
        if int(fp.get("maxPointByNode", 1)) != 1:
            raise IcpConfigError("%s: maxPointByNode must be 1" % name)
        size = float(fp.get("maxSizeByNode", 0.0))
        if not size > 0.0:
            raise IcpConfigError("%s: maxSizeByNode must be given and > 0 (got %r)" % (name, size))
        st.kind, st.dim, st.f[0] = DPF_OCTREE_GRID, -1, size
    elif name == "SurfaceNormalDataPointsFilter":
        _known_params(name, fp, ("knn", "epsilon", "keepNormals", "keepDensities", "keepEigenValues",
                                 "keepEigenVectors", "maxDist"))
        if "maxDist" in fp:
            raise IcpConfigError("%s: maxDist is not supported (the normals use the knn nearest points)" % name)
        if float(fp.get("epsilon", 0)) != 0:
            raise IcpConfigError("%s: epsilon must be 0 (exact neighbour search)" % name)
        knn = int(fp.get("knn", 5))
        if not 2 <= knn <= 16:
            raise IcpConfigError("%s: knn %d outside [2, 16]" % (name, knn))
        return SurfaceNormalStage(knn)
    else:
        raise IcpConfigError("unsupported data-point filter %r" % name)
    return st


def parse_icp_chain(text, dims=2):
    """YAML text -> IcpChain: the IcpParams of ``parse_icp_yaml`` plus the reading and reference data-point filters and
    the outlier filters / checker of ``IcpChain.outliers``.  ``dims=3``: a chain for N x 3 clouds (``dim: 2`` is the z
    axis; ``IcpChain.dims`` is 3)."""
    if dims not in (2, 3):
        raise IcpConfigError("parse_icp_chain: dims must be 2 or 3 (got %r)" % (dims,))
    doc = _load(text)
    if doc.get("readingStepDataPointsFilters"):
        raise IcpConfigError("readingStepDataPointsFilters are not supported")
    sides = {}
    for key in ("readingDataPointsFilters", "referenceDataPointsFilters"):
        nodes = doc.get(key) or []
        if not isinstance(nodes, list):
            nodes = [nodes]
        if len(nodes) > MAX_STAGES:
            raise IcpConfigError("%s: %d stages, at most %d" % (key, len(nodes), MAX_STAGES))
        sides[key] = [_stage(*_single(node, key), dims=dims) for node in nodes]
    outliers = IcpOutliers()
    params = _params(doc, outliers, dims)
    reading, reference = sides["readingDataPointsFilters"], sides["referenceDataPointsFilters"]
    if any(isinstance(s, SurfaceNormalStage) for s in reading):
        raise IcpConfigError("SurfaceNormalDataPointsFilter in readingDataPointsFilters: only the last reference stage "
                             "of a point-to-plane chain is supported")
    for i, s in enumerate(reference):
        if isinstance(s, SurfaceNormalStage):
            if i != len(reference) - 1:
                raise IcpConfigError("SurfaceNormalDataPointsFilter must be the last referenceDataPointsFilters stage")
            if params.minimizer not in (1, 2, 3):
                raise IcpConfigError("SurfaceNormalDataPointsFilter is only supported in a point-to-plane chain "
                                     "(PointToPlaneErrorMinimizer), where it sets the normals")
            params.normals_knn = s.knn
    return IcpChain(params, reading, reference, outliers, dims=dims)
