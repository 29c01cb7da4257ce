"""CPU: the data-point filters of an ICP chain -- icp_config.parse_icp_chain (supported modules, defaults, order,
refusals), parse_icp_yaml still refusing them, the sfe_icp_dpf mirror against the header, and the numpy restatement
of the predicate stages (tests/dpf_ref.py) on hand-computed float32 boundary cases."""
import os
import re

import numpy as np
import pytest

from sonar_slam_amd import _lib, icp_config

from dpf_ref import apply, keep_mask, stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "sonarfe.h")).read()

SHIPPED = """readingDataPointsFilters:

referenceDataPointsFilters:

matcher:
  KDTreeMatcher:
    knn: 1
    epsilon: 0 
    maxDist: 10.0

outlierFilters:
  - MaxDistOutlierFilter:
      maxDist: 3.0
  - TrimmedDistOutlierFilter:
      ratio: 0.8

errorMinimizer:
  # PointToPlaneErrorMinimizer:
  #   force2D: 1
  PointToPointErrorMinimizer

transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 40
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.01
      minDiffTransErr: 0.1
      smoothLength: 4   

inspector:
  NullInspector
"""

P2PLANE = SHIPPED.replace("  PointToPointErrorMinimizer\n", "").replace(
    "  # PointToPlaneErrorMinimizer:\n  #   force2D: 1", "  PointToPlaneErrorMinimizer:\n    force2D: 1")


def with_filters(reading="", reference="", base=SHIPPED):
    """the shipped file with entries under its (empty) filter sections"""
    return base.replace("readingDataPointsFilters:\n", "readingDataPointsFilters:\n" + reading, 1).replace(
        "referenceDataPointsFilters:\n", "referenceDataPointsFilters:\n" + reference, 1)


def lpm_point_to_plane(knn=10):
    """the form libpointmatcher runs: the reference carries normals"""
    return with_filters(reference="  - SurfaceNormalDataPointsFilter:\n      knn: %d\n      epsilon: 0\n"
                                  "      keepNormals: 1\n      keepDensities: 0\n" % knn, base=P2PLANE)


def test_shipped_file_gives_shipped_params_and_no_stages():
    ch = icp_config.parse_icp_chain(SHIPPED)
    assert ch.params.as_dict() == icp_config.shipped_params().as_dict()
    assert ch.reading == [] and ch.reference == [] and not ch.has_filters()


def test_each_module_and_its_defaults():
    y = with_filters(reading="  - MaxDistDataPointsFilter:\n      maxDist: 20.5\n"
                             "  - MinDistDataPointsFilter\n"
                             "  - BoundingBoxDataPointsFilter\n",
                     reference="  - MaxDistDataPointsFilter:\n      dim: 1\n      maxDist: -3\n"
                               "  - MinDistDataPointsFilter:\n      dim: 0\n      minDist: 0.25\n"
                               "  - BoundingBoxDataPointsFilter:\n      xMin: -2\n      xMax: 5\n      yMin: 0\n"
                               "      yMax: 7.5\n      zMin: -9\n      zMax: 9\n      removeInside: 0\n"
                               "  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.5\n      samplingMethod: 3\n"
                               "      maxPointByNode: 1\n      buildParallel: 1\n")
    ch = icp_config.parse_icp_chain(y)
    assert ch.params.as_dict() == icp_config.shipped_params().as_dict()
    r, f = ch.reading, ch.reference
    assert [s.kind for s in r] == [_lib.DPF_MAX_DIST, _lib.DPF_MIN_DIST, _lib.DPF_BOUNDING_BOX]
    assert [s.kind for s in f] == [_lib.DPF_MAX_DIST, _lib.DPF_MIN_DIST, _lib.DPF_BOUNDING_BOX, _lib.DPF_OCTREE_GRID]
    assert (r[0].dim, r[0].f[0]) == (-1, 20.5)
    assert (r[1].dim, r[1].f[0]) == (-1, 1.0)                                # libpointmatcher's defaults
    assert list(r[2].f) == [-1, 1, -1, 1, -1, 1] and r[2].remove_inside == 1
    assert (f[0].dim, f[0].f[0]) == (1, -3.0)
    assert (f[1].dim, f[1].f[0]) == (0, 0.25)
    assert list(f[2].f) == [-2, 5, 0, 7.5, -9, 9] and f[2].remove_inside == 0
    assert f[3].f[0] == 0.5
    rd, n_rd = ch.device_stages(ch.reading)
    assert n_rd == 3 and rd[0].f[0] == 20.5


def test_libpointmatcher_form_point_to_plane():
    ch = icp_config.parse_icp_chain(lpm_point_to_plane(10))
    assert ch.params.minimizer == 1 and ch.params.normals_knn == 10
    assert ch.reference == [icp_config.SurfaceNormalStage(10)] and not ch.has_filters()
    assert ch.device_stages(ch.reference) == (None, 0)
    ch6 = icp_config.parse_icp_chain(lpm_point_to_plane(6))
    assert ch6.params.normals_knn == 6
    want = icp_config.shipped_params(minimizer=1, normals_knn=6).as_dict()
    assert ch6.params.as_dict() == want


def test_octree_then_normals_in_the_reference():
    y = with_filters(reference="  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.3\n      samplingMethod: 3\n"
                               "  - SurfaceNormalDataPointsFilter:\n      knn: 7\n", base=P2PLANE)
    ch = icp_config.parse_icp_chain(y)
    assert ch.params.normals_knn == 7 and ch.device_stages(ch.reference)[1] == 1


@pytest.mark.parametrize("reading,reference,base,why", [
    ("  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n", "", SHIPPED, "random"),
    ("", "  - MaxPointCountDataPointsFilter:\n      maxCount: 100\n", SHIPPED, "random"),
    ("  - MaxDensityDataPointsFilter:\n      maxDensity: 10\n", "", SHIPPED, "random"),
    ("", "  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.5\n", SHIPPED, "samplingMethod"),
    ("", "  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.5\n      samplingMethod: 1\n", SHIPPED,
     "samplingMethod"),
    ("", "  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.5\n      samplingMethod: 3\n      maxPointByNode: 2\n",
     SHIPPED, "maxPointByNode"),
    ("  - MaxDistDataPointsFilter:\n      dim: 2\n      maxDist: 3\n", "", SHIPPED, "3-D"),
    ("", "  - MinDistDataPointsFilter:\n      dim: 2\n", SHIPPED, "3-D"),
    ("", "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n      epsilon: 0.1\n", P2PLANE, "epsilon"),
    ("", "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n      maxDist: 1\n", P2PLANE, "maxDist"),
    ("", "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n", SHIPPED, "point-to-plane"),
    ("  - SurfaceNormalDataPointsFilter:\n      knn: 10\n", "", P2PLANE, "readingDataPointsFilters"),
    ("", "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n  - MaxDistDataPointsFilter:\n      maxDist: 9\n", P2PLANE,
     "last"),
    ("", "  - SurfaceNormalDataPointsFilter:\n      knn: 17\n", P2PLANE, "knn"),
    ("  - MaxDistDataPointsFilter:\n      maxDist: 3\n      radius: 1\n", "", SHIPPED, "radius"),
    ("  - BoundingBoxDataPointsFilter:\n      xmin: 3\n", "", SHIPPED, "xmin"),
    ("", "  - MedianDistOutlierFilter\n", SHIPPED, "MedianDistOutlierFilter"),
    ("  - MaxDistDataPointsFilter:\n      maxDist: 3\n" * 9, "", SHIPPED, "at most 8"),
])
def test_refusals_name_module_and_reason(reading, reference, base, why):
    with pytest.raises(icp_config.IcpConfigError, match=why):
        icp_config.parse_icp_chain(with_filters(reading, reference, base))


def test_reading_step_filters_stay_refused():
    with pytest.raises(icp_config.IcpConfigError, match="readingStepDataPointsFilters"):
        icp_config.parse_icp_chain(SHIPPED + "readingStepDataPointsFilters:\n  - MaxDistDataPointsFilter:\n"
                                             "      maxDist: 3\n")


@pytest.mark.parametrize("reading,reference,base", [
    ("  - MaxDistDataPointsFilter:\n      maxDist: 20\n", "", SHIPPED),
    ("", "  - MinDistDataPointsFilter:\n      minDist: 1\n", SHIPPED),
    ("", "  - BoundingBoxDataPointsFilter\n", SHIPPED),
    ("", "  - OctreeGridDataPointsFilter:\n      maxSizeByNode: 0.5\n      samplingMethod: 3\n", SHIPPED),
    ("", "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n", P2PLANE),
])
def test_parse_icp_yaml_still_refuses_every_filter(reading, reference, base):
    y = with_filters(reading, reference, base)
    icp_config.parse_icp_chain(y)                      # a supported chain ...
    with pytest.raises(icp_config.IcpConfigError):     # ... that the params-only parser turns away
        icp_config.parse_icp_yaml(y)


def test_dpf_struct_and_codes_match_header():
    body = HDR[HDR.index("typedef struct sfe_icp_dpf {"):HDR.index("} sfe_icp_dpf;")]
    fields = re.findall(r"^\s*(float|int)\s+([a-z_]+)(?:\[(\d+)\])?;", body, re.M)
    mirror = _lib.IcpDpf._fields_
    assert [n for _, n, _ in fields] == [n for n, _ in mirror]
    import ctypes as C
    for (ty, name, count), (_, cty) in zip(fields, mirror):
        base = C.c_float if ty == "float" else C.c_int
        want = base * int(count) if count else base
        assert cty._type_ == want._type_ if count else cty == want, name
        if count:
            assert cty._length_ == int(count)
    codes = dict(re.findall(r"#define SFE_DPF_([A-Z_]+) (\d+)", HDR))
    assert {n: int(v) for n, v in codes.items()} == {n[len("DPF_"):]: getattr(_lib, n)
                                                    for n in dir(_lib) if n.startswith("DPF_")}
    assert int(codes["MAX_STAGES"]) == icp_config.MAX_STAGES
    status = dict(re.findall(r"#define SFE_ICP_(DPF_[A-Z]+) (\d+)", HDR))
    assert set(status) == {"DPF_EMPTY", "DPF_DEPTH"}
    for v in status.values():
        assert int(v) in _lib.ICP_STATUS_MESSAGES


def _nx(a, toward):
    return np.nextafter(np.float32(a), np.float32(toward), dtype=np.float32)


def test_restatement_boundaries_hand_computed():
    f32 = np.float32
    # MaxDist dim -1: |(3, 4)| = 5 exactly in float; 5 < 5 is false, 5 < next(5) true; the sign of maxDist is dropped
    p = np.array([[3, 4], [0, _nx(5, 0)], [_nx(5, 9), 0]], f32)
    assert keep_mask(p, stage(_lib.DPF_MAX_DIST, -1, f=[5])).tolist() == [False, True, False]
    assert keep_mask(p, stage(_lib.DPF_MAX_DIST, -1, f=[-5])).tolist() == [False, True, False]
    assert keep_mask(p, stage(_lib.DPF_MAX_DIST, -1, f=[_nx(5, 9)])).tolist() == [True, True, False]
    # MinDist dim -1: strict >
    assert keep_mask(p, stage(_lib.DPF_MIN_DIST, -1, f=[5])).tolist() == [False, False, True]
    # the float rounding of x*x + y*y: (1, 2^-12) squares to 1 + 2^-24, which rounds to 1 -> norm 1, not above 1
    q = np.array([[1, 2.0 ** -12], [_nx(1, 2), 0]], f32)
    assert keep_mask(q, stage(_lib.DPF_MIN_DIST, -1, f=[1])).tolist() == [False, True]
    # dim 0 / 1: signed for MaxDist, absolute for MinDist
    r = np.array([[-7, 2], [_nx(-2, 0), _nx(2, 0)], [2, -2]], f32)
    assert keep_mask(r, stage(_lib.DPF_MAX_DIST, 0, f=[-2])).tolist() == [True, False, False]
    assert keep_mask(r, stage(_lib.DPF_MAX_DIST, 1, f=[2])).tolist() == [False, True, True]
    assert keep_mask(r, stage(_lib.DPF_MIN_DIST, 1, f=[-2])).tolist() == [False, False, False]
    assert keep_mask(r, stage(_lib.DPF_MIN_DIST, 0, f=[_nx(2, 0)])).tolist() == [True, False, True]
    # BoundingBox: strict inside, removeInside flips it
    b = np.array([[-1, 0], [_nx(-1, 0), 0], [0, 1], [0, _nx(1, 0)], [5, 5]], f32)
    box = [-1, 1, -1, 1, 0, 0]
    assert keep_mask(b, stage(_lib.DPF_BOUNDING_BOX, remove_inside=0, f=box)).tolist() == [False, True, False, True, False]
    assert keep_mask(b, stage(_lib.DPF_BOUNDING_BOX, remove_inside=1, f=box)).tolist() == [True, False, True, False, True]


def test_restatement_composes_in_order():
    rng = np.random.default_rng(3)
    p = rng.uniform(-10, 10, (500, 2)).astype(np.float32)
    st = [stage(_lib.DPF_MAX_DIST, -1, f=[8]), stage(_lib.DPF_BOUNDING_BOX, remove_inside=1, f=[-2, 2, -3, 3])]
    out = apply(p, st)
    m = keep_mask(p, st[0]) & keep_mask(p, st[1])
    assert np.array_equal(out, p[m])
    with pytest.raises(ValueError):
        apply(p, [stage(_lib.DPF_OCTREE_GRID, f=[0.5])])
