"""CPU: the outlier filters and the checker an ICP chain takes beyond IcpParams -- MinDistOutlierFilter,
MedianDistOutlierFilter, NullOutlierFilter, BoundTransformationChecker: icp_config.parse_icp_chain (defaults,
combinations and orders, the Bound checker's place, refusals), parse_icp_yaml still refusing them, the
sfe_icp_outliers mirror against the header, and the numpy restatement of the ICP loop (tests/icp_chain_ref.py)
against the oracle on the chains the oracle covers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from sonar_slam_amd import _lib, icp_config, synth

import icp_chain_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "sonarfe.h")).read()

BASE = """matcher:
  KDTreeMatcher:
    knn: 1
    epsilon: 0
    maxDist: 10.0

outlierFilters:
%s
errorMinimizer:
  PointToPointErrorMinimizer

transformationCheckers:
%s
inspector:
  NullInspector
"""
SHIPPED_OUT = "  - MaxDistOutlierFilter:\n      maxDist: 3.0\n  - TrimmedDistOutlierFilter:\n      ratio: 0.8\n"
COUNTER = "  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
DIFF = ("  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.01\n      minDiffTransErr: 0.1\n"
        "      smoothLength: 4\n")
BOUND = "  - BoundTransformationChecker:\n      maxRotationNorm: 0.5\n      maxTranslationNorm: 2.0\n"


def chain(outliers=SHIPPED_OUT, checkers=COUNTER + DIFF):
    return icp_config.parse_icp_chain(BASE % (outliers, checkers))


def test_shipped_chain_has_no_outlier_record():
    ch = chain()
    assert ch.outliers == _lib.IcpOutliers() and not ch.outliers.any()
    assert ch.params.as_dict() == icp_config.shipped_params().as_dict()


def test_each_module_and_its_defaults():
    ch = chain("  - MinDistOutlierFilter\n  - MedianDistOutlierFilter\n  - NullOutlierFilter\n",
               COUNTER + "  - BoundTransformationChecker\n")
    o = ch.outliers
    assert (o.use_min_dist, o.min_dist, o.use_median, o.median_factor) == (1, 1.0, 1, 3.0)
    assert (o.use_bound, o.max_rotation_norm, o.max_translation_norm, o.bound_order) == (1, 1.0, 1.0, 1)
    assert not ch.params.use_max_dist_filter and not ch.params.use_trimmed_filter
    ch = chain("  - MinDistOutlierFilter:\n      minDist: 0.25\n  - MedianDistOutlierFilter:\n      factor: 2\n", COUNTER)
    assert (ch.outliers.min_dist, ch.outliers.median_factor, ch.outliers.use_bound) == (0.25, 2.0, 0)
    # value equality and a repr, like the stage classes
    same = chain("  - MedianDistOutlierFilter:\n      factor: 2\n  - MinDistOutlierFilter:\n      minDist: 0.25\n", COUNTER)
    assert same.outliers == ch.outliers and repr(same.outliers) == repr(ch.outliers)
    assert "median_factor=2.0" in repr(ch.outliers)
    assert chain("  - NullOutlierFilter\n").outliers == _lib.IcpOutliers()


@pytest.mark.parametrize("order", [
    ["MaxDistOutlierFilter", "TrimmedDistOutlierFilter", "MinDistOutlierFilter", "MedianDistOutlierFilter",
     "NullOutlierFilter"],
    ["NullOutlierFilter", "MedianDistOutlierFilter", "TrimmedDistOutlierFilter", "MinDistOutlierFilter",
     "MaxDistOutlierFilter"],
    ["MinDistOutlierFilter", "MaxDistOutlierFilter", "MedianDistOutlierFilter"],
])
def test_combinations_in_any_order_give_the_same_chain(order):
    text = {"MaxDistOutlierFilter": "  - MaxDistOutlierFilter:\n      maxDist: 2.0\n",
            "TrimmedDistOutlierFilter": "  - TrimmedDistOutlierFilter:\n      ratio: 0.7\n",
            "MinDistOutlierFilter": "  - MinDistOutlierFilter:\n      minDist: 0.1\n",
            "MedianDistOutlierFilter": "  - MedianDistOutlierFilter:\n      factor: 2.5\n",
            "NullOutlierFilter": "  - NullOutlierFilter\n"}
    ch = chain("".join(text[n] for n in order))
    rev = chain("".join(text[n] for n in reversed(order)))
    assert ch.outliers == rev.outliers and ch.params.as_dict() == rev.params.as_dict()
    assert ch.outliers.use_min_dist == ("MinDistOutlierFilter" in order)
    assert ch.outliers.use_median == 1 and ch.outliers.median_factor == 2.5
    assert ch.params.use_max_dist_filter == 1 and ch.params.max_dist_filter == 2.0
    assert ch.params.use_trimmed_filter == ("TrimmedDistOutlierFilter" in order)


@pytest.mark.parametrize("checkers, order", [
    (BOUND + COUNTER + DIFF, 0),
    (COUNTER + BOUND + DIFF, 1),
    (DIFF + BOUND + COUNTER, 2),
    (COUNTER + DIFF + BOUND, 3),
    (DIFF + COUNTER + BOUND, 3),
    (BOUND, 0),
])
def test_bound_position_is_recorded(checkers, order):
    ch = chain(SHIPPED_OUT, checkers)
    o = ch.outliers
    assert (o.use_bound, o.bound_order, o.max_rotation_norm, o.max_translation_norm) == (1, order, 0.5, 2.0)
    # Counter and Differential are read as before, wherever they stand
    if "Counter" in checkers:
        assert ch.params.max_iter == 40
    assert ch.params.use_diff_checker == ("Differential" in checkers)


@pytest.mark.parametrize("outliers, checkers, why", [
    ("  - MinDistOutlierFilter:\n      minDist: -0.5\n", COUNTER, "MinDistOutlierFilter: minDist must be >= 0"),
    ("  - MinDistOutlierFilter:\n      minDist: .nan\n", COUNTER, "MinDistOutlierFilter: minDist"),
    ("  - MinDistOutlierFilter:\n      maxDist: 1\n", COUNTER, r"MinDistOutlierFilter: unsupported parameters \['maxDist'\]"),
    ("  - MedianDistOutlierFilter:\n      factor: 0\n", COUNTER, "MedianDistOutlierFilter: factor must be finite and > 0"),
    ("  - MedianDistOutlierFilter:\n      factor: -1\n", COUNTER, "MedianDistOutlierFilter: factor"),
    ("  - MedianDistOutlierFilter:\n      factor: .inf\n", COUNTER, "MedianDistOutlierFilter: factor must be finite"),
    ("  - MedianDistOutlierFilter:\n      ratio: 0.5\n", COUNTER, r"MedianDistOutlierFilter: unsupported parameters"),
    ("  - NullOutlierFilter:\n      ratio: 0.5\n", COUNTER, "NullOutlierFilter: unsupported parameters"),
    ("  - MedianDistOutlierFilter\n  - MedianDistOutlierFilter\n", COUNTER, "MedianDistOutlierFilter listed twice"),
    ("  - MinDistOutlierFilter\n  - MinDistOutlierFilter\n", COUNTER, "MinDistOutlierFilter listed twice"),
    ("  - NullOutlierFilter\n  - NullOutlierFilter\n", COUNTER, "NullOutlierFilter listed twice"),
    (SHIPPED_OUT + "  - MaxDistOutlierFilter:\n      maxDist: 1.0\n", COUNTER, "MaxDistOutlierFilter listed twice"),
    (SHIPPED_OUT + "  - TrimmedDistOutlierFilter:\n      ratio: 0.5\n", COUNTER, "TrimmedDistOutlierFilter listed twice"),
    ("  - VarTrimmedDistOutlierFilter:\n      minRatio: 0.1\n", COUNTER, "unsupported outlier filter"),
    ("  - RobustOutlierFilter\n", COUNTER, "unsupported outlier filter"),
    (SHIPPED_OUT, COUNTER + "  - BoundTransformationChecker:\n      maxRotationNorm: 0\n",
     "BoundTransformationChecker: maxRotationNorm must be finite and > 0"),
    (SHIPPED_OUT, COUNTER + "  - BoundTransformationChecker:\n      maxTranslationNorm: .inf\n",
     "BoundTransformationChecker: maxTranslationNorm must be finite"),
    (SHIPPED_OUT, COUNTER + "  - BoundTransformationChecker:\n      maxTranslationNorm: -2\n",
     "BoundTransformationChecker: maxTranslationNorm"),
    (SHIPPED_OUT, COUNTER + "  - BoundTransformationChecker:\n      maxRotation: 1\n",
     "BoundTransformationChecker: unsupported parameters"),
    (SHIPPED_OUT, BOUND + COUNTER + BOUND, "BoundTransformationChecker listed twice"),
])
def test_refusals_name_module_and_reason(outliers, checkers, why):
    with pytest.raises(icp_config.IcpConfigError, match=why):
        chain(outliers, checkers)


@pytest.mark.parametrize("outliers, checkers, name", [
    ("  - MinDistOutlierFilter\n", COUNTER, "MinDistOutlierFilter"),
    ("  - MedianDistOutlierFilter\n", COUNTER, "MedianDistOutlierFilter"),
    ("  - NullOutlierFilter\n", COUNTER, "NullOutlierFilter"),
    (SHIPPED_OUT, COUNTER + BOUND, "BoundTransformationChecker"),
])
def test_parse_icp_yaml_still_refuses_the_new_modules(outliers, checkers, name):
    with pytest.raises(icp_config.IcpConfigError, match=name + ".*parse_icp_chain"):
        icp_config.parse_icp_yaml(BASE % (outliers, checkers))


def test_median_stays_refused_as_a_data_point_filter():
    with pytest.raises(icp_config.IcpConfigError, match="MedianDistOutlierFilter"):
        icp_config.parse_icp_chain("readingDataPointsFilters:\n  - MedianDistOutlierFilter\n")


def test_outliers_struct_and_status_match_header():
    body = HDR[HDR.index("typedef struct sfe_icp_outliers {"):HDR.index("} sfe_icp_outliers;")]
    fields = re.findall(r"^\s*(float|int)\s+([a-z_]+);", body, re.M)
    mirror = _lib.IcpOutliers._fields_
    assert [n for _, n in fields] == [n for n, _ in mirror]
    for (ty, name), (_, cty) in zip(fields, mirror):
        assert cty == (C.c_float if ty == "float" else C.c_int), name
    assert C.sizeof(_lib.IcpOutliers) == 4 * len(fields)
    assert int(re.search(r"#define SFE_ICP_BOUND (\d+)", HDR).group(1)) == _lib.ICP_BOUND == 9
    assert _lib.ICP_STATUS_MESSAGES[_lib.ICP_BOUND] == "limit out of bounds"
    for fn in ("guesses", "pairs", "jobs"):
        name = "sfe_icp_compute_%s_chain_ext" % fn
        base = _lib.SIGNATURES["sfe_icp_compute_%s_chain" % fn][1]
        args = _lib.SIGNATURES[name][1]
        # the _chain call's arguments with the struct next to sfe_icp_params
        assert args[:2] + args[3:] == base and args[2] == C.POINTER(_lib.IcpOutliers)


# ---- the restatement against the oracle, on chains the oracle covers ----
def _pose_diff(Ta, Tb):
    a, b = synth.pose_of(Ta), synth.pose_of(Tb)
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]), abs(np.arctan2(np.sin(a[2] - b[2]), np.cos(a[2] - b[2]))))


CHAINS = {
    "shipped": {},
    "p2plane": dict(minimizer=1),
    "maxdist_only": dict(use_trimmed_filter=0),
    "trimmed_only": dict(use_max_dist_filter=0),
    "no_diff": dict(use_diff_checker=0, max_iter=12),
    "trim_half_no_diff": dict(use_max_dist_filter=0, trim_ratio=0.5, use_diff_checker=0, max_iter=8),
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_restatement_equals_oracle(name):
    p = icp_config.shipped_params(**CHAINS[name])
    op = oracle.shipped_icp_params(precision=1, **p.as_dict())
    for seed in range(3):
        src, tgt, guess, _ = synth.scan_pair(seed=70 + seed, n_src=220, n_tgt=260)
        st, T, it = icp_chain_ref.icp(src, tgt, guess, p)
        st_o, T_o, it_o = oracle.icp(src, tgt, guess, op)
        assert (st, it) == (st_o, it_o), (name, seed)
        if st == 0:
            assert _pose_diff(T, T_o) < 1e-6, (name, seed, _pose_diff(T, T_o))
        else:
            assert np.array_equal(T, T_o)


def test_restatement_neutral_modules_change_nothing():
    """MinDist 0, a Bound never reached, NullOutlierFilter (no field) and MedianDist{1} == Trimmed{0.5}"""
    src, tgt, guess, _ = synth.scan_pair(seed=91, n_src=200, n_tgt=240)
    p = icp_config.shipped_params()
    base = icp_chain_ref.icp(src, tgt, guess, p)
    ox = _lib.IcpOutliers(use_min_dist=1, min_dist=0.0, use_bound=1, max_rotation_norm=3.0, max_translation_norm=1e6)
    got = icp_chain_ref.icp(src, tgt, guess, p, ox)
    assert got[0] == base[0] and got[2] == base[2] and np.array_equal(got[1], base[1])
    pt = icp_config.shipped_params(use_trimmed_filter=1, trim_ratio=0.5)
    pm = icp_config.shipped_params(use_trimmed_filter=0)
    a = icp_chain_ref.icp(src, tgt, guess, pt)
    b = icp_chain_ref.icp(src, tgt, guess, pm, _lib.IcpOutliers(use_median=1, median_factor=1.0))
    assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])
