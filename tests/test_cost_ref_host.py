"""The references of tests/cost_ref.py against the oracle, and the constructed cases of tests/test_gpu_cost_edges.py against what
they are built to hold: every named wrong variant changes the answer of the case built for it.  No GPU."""
import functools
import os
import sys
import time
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
import cost_ref as R  # noqa: E402

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _cases():
    return R.cell_cases()


CASE_NAMES = ("near_tie_0.03", "near_tie_0.035", "near_tie_0.03_T", "true_tie", "true_tie_T", "edge_of_grid", "non_finite", "fma",
              "random_checkerboard")


def _moved(case, variant, f64):
    """per pose: the number of source points whose hit / miss the variant changes"""
    a = [R.hits(case["grid"], case["src"], T, case["xmin"], case["ymin"], case["res"], f64) for T in case["T6"]]
    b = [R.hits(case["grid"], case["src"], T, case["xmin"], case["ymin"], case["res"], f64, variant) for T in case["T6"]]
    return np.array([int(np.sum(x != y)) for x, y in zip(a, b)])


# ---- the references -----------------------------------------------------------------------------------------------------------
def test_ellipse_equals_the_oracle_and_the_opencv_tutorial():
    for hs in list(range(0, 46)) + [64, 100]:
        assert np.array_equal(R.ellipse(hs), oracle.ellipse_kernel(hs)), hs
    assert R.ellipse(0).tolist() == [[1]]
    # cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (5, 5)) and (7, 7) as printed in OpenCV's morphology tutorial
    assert R.ellipse(2).tolist() == [[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]]
    assert R.ellipse(3).tolist() == [[0, 0, 0, 1, 0, 0, 0], [0, 1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1],
                                     [1, 1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 0], [0, 0, 0, 1, 0, 0, 0]]


@pytest.mark.parametrize("shape", R.STAMP_SHAPES, ids=lambda s: "%dx%d_hs%d" % s)
def test_grid_equals_the_oracle_on_every_stamp_case(shape):
    rows, cols, hs = shape
    r, c = R.stamp_case(rows, cols, hs)
    g = R.grid(r, c, rows, cols, hs)
    assert g.dtype == np.uint8 and g.shape == (rows, cols) and set(np.unique(g)) <= {0, 255}
    assert np.array_equal(g, oracle.cost_grid(r, c, rows, cols, hs))
    assert np.all(g[r, c] == 255)
    # all four corners and the border midpoints are targets
    have = set(zip(r.tolist(), c.tolist()))
    assert {(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (0, cols // 2), (rows // 2, cols - 1)} <= have
    assert np.array_equal(R.grid([], [], rows, cols, hs), np.zeros((rows, cols), np.uint8))


def test_grid_equals_the_oracle_on_the_other_grids_the_gpu_tests_build():
    for name, c in R.stamp_points_cases().items():
        r, cc = R.cells_of_points(c["pts"], c["xmin"], c["ymin"], c["res"], c["rows"], c["cols"])
        assert np.array_equal(R.stamp_points_grid(c), oracle.cost_grid(r, cc, c["rows"], c["cols"], c["hs"])), name
    cases = [R.counts_case()] + [R.lds_case(*s) for s in R.LDS_SHAPES.values()] + list(_cases().values())
    for c in cases:
        assert np.array_equal(c["grid"], oracle.cost_grid(c["tgt_r"], c["tgt_c"], c["rows"], c["cols"], c["hs"])), c["name"]
        assert np.array_equal(c["grid"], R.grid(c["tgt_r"], c["tgt_c"], c["rows"], c["cols"], c["hs"])), c["name"]


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_cost_equals_the_oracle_on_every_checkerboard_case(name, f64):
    c = _cases()[name]
    want = oracle.matching_cost(c["grid"], c["src"], c["T6"], c["xmin"], c["ymin"], c["res"], f64_points=f64)
    got = R.cost(c["grid"], c["src"], c["T6"], c["xmin"], c["ymin"], c["res"], f64)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if f64 in c["dtypes"]:
        assert len(set(got.tolist())) >= 5, got          # a cost written to the wrong pose slot shows


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_cost_equals_the_oracle_on_the_count_and_lds_cases(f64):
    for c in [R.counts_case()] + [R.lds_case(*s) for s in R.LDS_SHAPES.values()]:
        want = oracle.matching_cost(c["grid"], c["src"], c["T6"], c["xmin"], c["ymin"], c["res"], f64_points=f64)
        got = R.cost(c["grid"], c["src"], c["T6"], c["xmin"], c["ymin"], c["res"], f64)
        assert np.array_equal(got, want), c["name"]
        assert len(set(got.tolist())) >= 5 and got.min() < -20, (c["name"], got)
        assert len(set(got[:9].tolist())) >= 5, (c["name"], got[:9])


def _fl32(x):
    """the float32 nearest to the Fraction x, ties to even"""
    if x == 0:
        return 0.0
    e = max(int(np.floor(np.log2(float(abs(x))))), -126)
    while Fraction(2) ** e > abs(x) and e > -126:
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(x):
        e += 1
    n = round(abs(x) / Fraction(2) ** (e - 23))             # Python rounds a Fraction half to even
    v = float(n * Fraction(2) ** (e - 23))
    return -v if x < 0 else v


def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(111)
    a = (rng.uniform(-1, 1, 3000) * 2.0 ** rng.integers(-8, 9, 3000)).astype(F32)
    b = (rng.uniform(-1, 1, 3000) * 2.0 ** rng.integers(-8, 9, 3000)).astype(F32)
    c = (rng.uniform(-1, 1, 3000) * 2.0 ** rng.integers(-30, 9, 3000)).astype(F32)
    c[:500] = -(a[:500] * b[:500]) * F32(1 + 2.0 ** -20)     # cancellation
    # products that ARE float32 half-way points (1 + k 2^-12)(1 + m 2^-12), k m odd, with an addend far below an ulp of the
    # double sum: the float64 sum lands on the tie and a second rounding to float32 goes the wrong way for one sign
    k, m = 2 * rng.integers(0, 2000, 600) + 1, 2 * rng.integers(0, 2000, 600) + 1
    ta, tb = (1 + k * 2.0 ** -12).astype(F32), (1 + m * 2.0 ** -12).astype(F32)
    tc = (np.where(np.arange(600) % 2, 1, -1) * 2.0 ** -rng.integers(58, 90, 600)).astype(F32)
    a, b, c = np.r_[a, ta], np.r_[b, tb], np.r_[c, tc]
    got = R.fma32(a, b, c)
    assert got.dtype == F32
    want = np.array([_fl32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.astype(np.float64), want)
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert np.sum(twice.astype(np.float64) != want) >= 100   # the triples do tell one rounding from two
    with np.errstate(over="ignore", invalid="ignore"):       # non-finite operands pass through
        assert np.isnan(R.fma32(F32(np.nan), F32(1), F32(1))) and R.fma32(F32(3e38), F32(3e38), F32(1)) == np.inf
        assert np.isnan(R.fma32(F32(np.inf), F32(0), F32(1))) and R.fma32(F32(0), F32(5), F32(-np.inf)) == -np.inf


def test_cells_of_points_clamps_and_drops_nan():
    r, c = R.cells_of_points(np.array([[0.0, 0.0], [-9, 9], [9, -9], [np.nan, 0], [0, np.nan], [np.inf, -np.inf], [0.125, 0.375]], F32),
                             F32(0), F32(0), 0.25, 5, 7)
    assert r.tolist() == [0, 4, 0, 0, 2] and c.tolist() == [0, 0, 6, 6, 0]      # 0.5 -> 0 and 1.5 -> 2: half to even


# ---- every wrong variant moves the case built for it --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["near_tie_0.03", "near_tie_0.035", "near_tie_0.03_T"])
def test_near_tie_case_is_exact_and_moves_mul_not_div(name):
    c = _cases()[name]
    axis = 1 if name.endswith("_T") else 0
    x = c["src"][:, axis].astype(np.float64)
    assert np.array_equal(x - float(R.NEAR_TIE_XMIN), c["d"]) and len(np.unique(c["d"])) == len(x)
    d, differs = R.near_tie_lattice(c["res"])
    assert np.isin(d, c["d"]).all()
    moved = _moved(c, "mul_not_div", True)
    print(name, "lattice points kept", len(d), "of them with another cell by multiplication", int(differs.sum()),
          "points moved per pose", moved.tolist())
    assert moved[0] == differs.sum() >= 10 and len(d) >= 40
    assert np.all(moved[:4] >= 10)                       # ... and under every pure x translation
    # under the identity every point sits on a set cell, so cells that are wrong cannot cancel
    assert R.cost(c["grid"], c["src"], c["T6"][:1], c["xmin"], c["ymin"], c["res"], True)[0] == -len(x)
    if c["res"] == 0.03 and not axis:
        for dd in (1.875, 3.375, 6.375, 12.375, 13.875):
            assert dd in c["d"] and np.rint(dd * (1.0 / 0.03)) != np.rint(dd / 0.03)


@pytest.mark.parametrize("name", ["true_tie", "true_tie_T"])
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("variant", ["half_away", "floor_cell"])
def test_true_tie_case_moves_the_rounding_variants(name, f64, variant):
    c = _cases()[name]
    q = (c["src"].astype(np.float64) - [float(c["xmin"]), float(c["ymin"])]) / c["res"]
    assert np.array_equal(q * 2, np.round(q * 2)) and np.all(np.any(q != np.round(q), axis=1))     # every point on a k + 0.5
    for k, n in ((0, c["cols"]), (1, c["rows"])):
        assert -0.5 in q[:, k] and n - 0.5 in q[:, k]
    moved = _moved(c, variant, f64)
    print(name, variant, "f64" if f64 else "f32", "points moved per pose", moved.tolist())
    assert moved[0] >= 100 and moved.sum() >= 500


def test_fma_case_moves_unfused():
    t0 = time.perf_counter()
    c = R.fma_case()
    took = time.perf_counter() - t0
    moved = _moved(c, "unfused", False)
    print("fma: found per pose", c["n_found"], "points moved per pose", moved.tolist(), "search %.2f s" % took)
    assert took < 2.0
    assert sum(c["n_found"]) >= R.FMA_MIN_POINTS and np.all(moved >= np.array(c["n_found"])) and moved.sum() >= R.FMA_MIN_POINTS
    assert np.array_equal(c["src"][:len(c["found"])], c["found"])
    again = R.fma_case()
    assert np.array_equal(again["src"], c["src"]) and np.array_equal(again["T6"], c["T6"])        # seeded


def test_res32_in_f64_moves_a_checkerboard_case():
    moved = {n: _moved(_cases()[n], "res32_in_f64", True) for n in ("near_tie_0.03", "near_tie_0.035", "random_checkerboard")}
    print("res32_in_f64: points moved per pose", {n: m.tolist() for n, m in moved.items()})
    # float(float32(0.03)) is 2e-8 of itself away from 0.03: a thousandth of a cell at the far end of these grids, which only
    # the near-tie points feel
    assert np.all(moved["near_tie_0.03"] > 0) and np.all(moved["near_tie_0.035"] > 0)
    assert float(F32(0.03)) != 0.03 and float(F32(0.035)) != 0.035


def test_no_variant_is_the_reference_itself():
    """each variant changes a COST of its case (not only single points that cancel)"""
    C = _cases()
    for variant, name, f64 in (("mul_not_div", "near_tie_0.03", True), ("mul_not_div", "near_tie_0.035", True),
                               ("mul_not_div", "near_tie_0.03_T", True), ("half_away", "true_tie", True),
                               ("half_away", "true_tie", False), ("floor_cell", "true_tie", True), ("floor_cell", "true_tie_T", False),
                               ("unfused", "fma", False), ("res32_in_f64", "near_tie_0.03", True),
                               ("res32_in_f64", "near_tie_0.035", True)):
        c = C[name]
        right = R.cost(c["grid"], c["src"], c["T6"], c["xmin"], c["ymin"], c["res"], f64)
        wrong = R.cost(c["grid"], c["src"], c["T6"], c["xmin"], c["ymin"], c["res"], f64, variant)
        assert not np.array_equal(right, wrong), (variant, name)


def _box_can_show(rows, hs):
    """a grid of ``rows`` rows sees the element rows |dy| <= rows - 1 of a target: a square element differs from the ellipse
    only if one of those is narrower than the square"""
    e = R.ellipse(hs)
    lo = hs - min(hs, rows - 1)
    return bool((e[lo:2 * hs + 1 - lo] == 0).any())


@pytest.mark.parametrize("shape", R.STAMP_SHAPES, ids=lambda s: "%dx%d_hs%d" % s)
def test_stamp_cases_move_the_grid_variants(shape):
    rows, cols, hs = shape
    r, c = R.stamp_case(rows, cols, hs)
    g = R.grid(r, c, rows, cols, hs)
    n_clip = int(np.sum(g != R.grid(r, c, rows, cols, hs, "no_clip")))
    n_box = int(np.sum(g != R.grid(r, c, rows, cols, hs, "box")))
    rs, cs = R.stamp_case(rows, cols, hs, sparse=True)
    gs = R.grid(rs, cs, rows, cols, hs)
    assert np.array_equal(gs, oracle.cost_grid(rs, cs, rows, cols, hs))
    s_clip = int(np.sum(gs != R.grid(rs, cs, rows, cols, hs, "no_clip")))
    s_box = int(np.sum(gs != R.grid(rs, cs, rows, cols, hs, "box")))
    print(shape, "cells changed by no_clip", n_clip, "by box", n_box, "| one target: by no_clip", s_clip, "by box", s_box,
          "| cells set", int((g > 0).sum()), "and", int((gs > 0).sum()), "of", g.size)
    assert (n_clip > 0) == (hs > 0) and (s_clip > 0) == (hs > 0)
    # a square element can only add cells: where the corner, midpoint and interior targets have filled the grid already
    # (1 x 33, 9 x 64, 3 x 97 and 6 x 96 at hs >= 17) it cannot show.  The one-target case shows it wherever the grid sees an
    # element row that is narrower than the square: all shapes with hs >= 2 but 1 x 33, 3 x 97 and 6 x 96, whose visible rows
    # |dy| <= rows - 1 are as wide as the square at hs = 17, 40 and 33.
    assert (n_box > 0) == (hs >= 2 and not np.all(g == 255))
    assert _box_can_show(rows, hs) == (hs >= 2 and shape not in ((1, 33, 17), (3, 97, 40), (6, 96, 33)))
    assert (s_box > 0) == _box_can_show(rows, hs)
    assert hs == 0 or (gs == 0).any()                    # the one-target grid is never full: a stray bit shows


OUTSIDE_SHAPES = R.OUTSIDE_SHAPES


@pytest.mark.parametrize("shape", OUTSIDE_SHAPES, ids=lambda s: "%dx%d_hs%d" % s)
def test_grid_equals_the_oracle_with_targets_outside_the_grid(shape):
    rows, cols, hs = shape
    r, c = R.outside_targets(rows, cols, hs)
    assert not np.any((r >= 0) & (r < rows) & (c >= 0) & (c < cols))
    g = R.grid(r, c, rows, cols, hs)
    assert np.array_equal(g, oracle.cost_grid(r, c, rows, cols, hs))
    assert g.any() and not g.all()
    far = (r < -hs) | (r > rows - 1 + hs) | (c < -hs) | (c > cols - 1 + hs)
    assert far.any() and np.array_equal(g, R.grid(r[~far], c[~far], rows, cols, hs))     # some reach in, the farthest do not


def test_word_mask_cases_are_among_the_stamp_shapes():
    """a span that covers a whole middle word, hs = 0, cols % 32 == 0 and == 1, cols < 32, an element larger than the grid"""
    S = R.STAMP_SHAPES
    assert any(hs >= 16 and cols >= 96 for _, cols, hs in S) and any(hs == 0 for _, _, hs in S)
    assert any(cols % 32 == 0 for _, cols, _ in S) and any(cols % 32 == 1 for _, cols, _ in S) and any(cols < 32 for _, cols, _ in S)
    assert any(2 * hs + 1 > max(rows, cols) for rows, cols, hs in S)
    g = R.grid(*R.stamp_case(6, 96, 33), 6, 96, 33)
    assert np.all(g[:, 32:64] == 255)                    # the middle word of every row, whole


# ---- conditions on the stamp-points, count and LDS cases ------------------------------------------------------------------------
def test_stamp_points_cases_hold_what_they_are_for():
    S = R.stamp_points_cases()
    c = S["clamped"]
    with np.errstate(invalid="ignore"):
        q = np.c_[(c["pts"][:, 0] - c["xmin"]) / F32(c["res"]), (c["pts"][:, 1] - c["ymin"]) / F32(c["res"])]
    assert (q[:, 0] < -0.5).sum() >= 5 and (q[:, 0] > c["cols"] - 0.5).sum() >= 5          # clamp on all four sides
    assert (q[:, 1] < -0.5).sum() >= 5 and (q[:, 1] > c["rows"] - 0.5).sum() >= 5
    r, cc = R.cells_of_points(c["pts"], c["xmin"], c["ymin"], c["res"], c["rows"], c["cols"])
    assert len(r) == len(c["pts"]) - 2 and np.isnan(c["pts"]).any(axis=1).sum() == 2
    for k, n in ((r, c["rows"]), (cc, c["cols"])):
        assert k.min() == 0 and k.max() == n - 1
    h = S["half_cells"]
    q = (h["pts"].astype(np.float64) - [float(h["xmin"]), float(h["ymin"])]) / h["res"]
    assert np.all(q - np.floor(q) == 0.5) and q.min() == -0.5 and float(F32(h["res"])) == h["res"]
    assert len(S["one_point"]["pts"]) == 1 and len(S["empty"]["pts"]) == 0 and not R.stamp_points_grid(S["empty"]).any()
    b = S["8193_items"]
    assert len(b["pts"]) * (2 * b["hs"] + 1) == 8193 == R.STAMP_POINTS_ITEMS + 1
    # the last point's cell is set by nothing else: a launch that drops the 8193rd item shows
    g_all = R.stamp_points_grid(b)
    g_less = R.stamp_points_grid(dict(b, pts=b["pts"][:-1]))
    assert not np.array_equal(g_all, g_less)


def test_count_and_lds_cases_hold_what_they_are_for():
    c = R.counts_case()
    assert len(c["src"]) == max(R.SOURCE_SIZES) and len(c["T6"]) == max(R.POSE_COUNTS)
    # the last point of every source prefix is on a set cell under the identity: a lost tail shows
    h = R.hits(c["grid"], c["src"], c["T6"][0], c["xmin"], c["ymin"], c["res"], True)
    print("counts: hits of the prefixes", [int(h[:n].sum()) for n in R.SOURCE_SIZES])
    assert all(h[n - 1] for n in R.SOURCE_SIZES[1:])
    assert R.LDS_SHAPES["lds_exact"][0] * ((R.LDS_SHAPES["lds_exact"][1] + 31) // 32) == R.LDS_WORDS
    assert R.LDS_SHAPES["one_row_more"][0] * ((R.LDS_SHAPES["one_row_more"][1] + 31) // 32) == R.LDS_WORDS + 32
    assert R.LDS_SHAPES["partial_last_word"][1] % 32 and \
        R.LDS_SHAPES["partial_last_word"][0] * ((R.LDS_SHAPES["partial_last_word"][1] + 31) // 32) <= R.LDS_WORDS
    for rows, cols in R.LDS_SHAPES.values():
        c = R.lds_case(rows, cols)
        assert len(c["src"]) == 300 and 30 <= len(c["tgt_r"]) <= 48 and c["hs"] == 10
        assert (rows - 1) in c["tgt_r"] and (cols - 1) in c["tgt_c"]
        fr, fc = R.cell_floats(c["src"], c["T6"][0], c["xmin"], c["ymin"], c["res"], True)
        h = R.hits(c["grid"], c["src"], c["T6"][0], c["xmin"], c["ymin"], c["res"], True)
        assert (h & (fr >= rows - 3)).sum() >= 3 and (h & (fc >= cols - 3)).sum() >= 3     # hits in the last rows and columns
        assert (fr >= rows).any() and (fc >= cols).any()                                    # and points just beyond them
