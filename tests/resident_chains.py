"""ICP chains (YAML text, parsed by icp_config.parse_icp_chain) for the tests of chains on the resident paths: the
store, replay.FrontEnd, chained.SessionBatch and farm.IcpFarm.  Test infrastructure only."""
from sonar_slam_amd import icp_config

_MATCHER = """matcher:
  KDTreeMatcher: {knn: 1, epsilon: 0, maxDist: 10.0}
"""
_CHECKERS = """transformationCheckers:
  - CounterTransformationChecker: {maxIterationCount: 40}
  - DifferentialTransformationChecker: {minDiffRotErr: 0.01, minDiffTransErr: 0.1, smoothLength: 4}
"""
_TAIL = """inspector: NullInspector
logger: NullLogger
"""
_SHIPPED_OUTLIERS = """outlierFilters:
  - MaxDistOutlierFilter: {maxDist: 3.0}
  - TrimmedDistOutlierFilter: {ratio: 0.8}
"""
_P2P = "errorMinimizer: PointToPointErrorMinimizer\n"

# bruce_slam/config/icp.yaml as shipped: no module beyond IcpParams
SHIPPED = _MATCHER + _SHIPPED_OUTLIERS + _P2P + _CHECKERS + _TAIL

CHAINS = {
    # a reading MaxDist and a reference octree (medoid) stage
    "filters": """readingDataPointsFilters:
  - MaxDistDataPointsFilter: {dim: -1, maxDist: 18.0}
referenceDataPointsFilters:
  - OctreeGridDataPointsFilter: {maxSizeByNode: 0.8, samplingMethod: 3, maxPointByNode: 1}
""" + _MATCHER + _SHIPPED_OUTLIERS + _P2P + _CHECKERS + _TAIL,
    # MinDist + MedianDist outlier filters and a Bound checker tight enough to stop the jobs with a poor guess
    "outliers": _MATCHER + """outlierFilters:
  - MaxDistOutlierFilter: {maxDist: 3.0}
  - TrimmedDistOutlierFilter: {ratio: 0.8}
  - MinDistOutlierFilter: {minDist: 0.01}
  - MedianDistOutlierFilter: {factor: 2.5}
""" + _P2P + _CHECKERS + """  - BoundTransformationChecker: {maxRotationNorm: 0.08, maxTranslationNorm: 0.45}
""" + _TAIL,
    # point-to-plane: a reference bounding box, then the normals
    "plane": """referenceDataPointsFilters:
  - BoundingBoxDataPointsFilter: {xMin: -26.0, xMax: 26.0, yMin: -26.0, yMax: 26.0, zMin: -1.0, zMax: 1.0, removeInside: 0}
  - SurfaceNormalDataPointsFilter: {knn: 8, epsilon: 0}
""" + _MATCHER + _SHIPPED_OUTLIERS + """errorMinimizer:
  PointToPlaneErrorMinimizer: {force2D: 1}
transformationCheckers:
  - CounterTransformationChecker: {maxIterationCount: 30}
""" + _TAIL,
    # keeps x > 0 only: a cloud that lies at x < 0 is left empty (status 7)
    "empty": """readingDataPointsFilters:
  - BoundingBoxDataPointsFilter: {xMin: 0.0, xMax: 60.0, yMin: -60.0, yMax: 60.0, removeInside: 0}
""" + _MATCHER + _SHIPPED_OUTLIERS + _P2P + _CHECKERS + _TAIL,
    # the replay chain: filters on both sides and a median outlier filter
    "replay": """readingDataPointsFilters:
  - MaxDistDataPointsFilter: {dim: -1, maxDist: 20.0}
referenceDataPointsFilters:
  - OctreeGridDataPointsFilter: {maxSizeByNode: 0.7, samplingMethod: 3}
""" + _MATCHER + """outlierFilters:
  - MaxDistOutlierFilter: {maxDist: 3.0}
  - TrimmedDistOutlierFilter: {ratio: 0.8}
  - MedianDistOutlierFilter: {factor: 3.0}
""" + _P2P + _CHECKERS + _TAIL,
}


def chain(name):
    return icp_config.parse_icp_chain(SHIPPED if name == "shipped" else CHAINS[name])
