"""The constructed cases of tests/mapping_edges.py run through tests/mapping_ref.py alone: every case holds what it is for, so
that tests/test_gpu_mapping_edges.py cannot pass vacuously.  Conditions on the cases, not measurements of the product."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mapping_edges as E  # noqa: E402
import mapping_ref  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402

GROUPS = E.measure_groups()
F32 = np.float32


def test_pings_are_small_and_give_their_shapes():
    for shape, ping in E.SHAPES.items():
        if ping is not None:
            assert E.image_shape(E.MEASURE_SETTINGS, ping) == shape
            assert len(ping.bearings) <= 33 and ping.num_ranges <= 40 and len(ping.bearings) % 2 == 1
            assert ping.bearings[len(ping.bearings) // 2] == 0
    assert max(r * c for r, c in E.SHAPES) == 40 * 33
    # fixed-table and computed kernel sizes, one-tap axes, and per shape one window larger than the image on both axes
    assert {(0, 0), (0, 2), (3, 0), (1, 1), (2, 3), (4, 4), (5, 2)} <= set(E.PAIRS) and None in E.PAIRS
    assert len(GROUPS) == len(E.SHAPES) * len(E.PAIRS) + 1
    for case in itertools.chain(*GROUPS.values()):
        if case.hits is not None and len(case.hits):
            assert case.hits.min() >= 0 and (case.hits.max(axis=0) < case.shape).all()


def single(mask, r, c):
    return mask.sum() == 1 and mask[r, c] == 1


@pytest.mark.parametrize("group", list(GROUPS))
def test_measure_cases_hold_what_their_names_claim(group):
    seen = set()
    for case in GROUPS[group]:
        rows, cols = case.shape
        lo, st = E.measure_ref(case)
        prob, miss, hit = st["prob"], F32(case.miss_prob), F32(case.hit_prob)
        assert prob.shape == case.shape and prob.dtype == np.float32 and lo.shape == (rows * cols,)
        lay = case.layout
        seen.add(lay)
        if case.hits is None:
            assert lay == "no_points" and case.hr == -1 and "hits" not in st and (prob == miss).all()
            continue
        assert case.hr >= 0 and case.hc >= 0
        mask, fh, hr = st["hits"], st["first_hits"], case.hr
        top = np.nonzero(mask[0])[0]
        # np.argmax's quirk: a first value above 0.5 in row 0 reads as "no hit", and the whole column becomes miss
        assert (fh[top] == rows).all() and (prob[:, top] == miss).all()
        last = rows - 1
        if lay in ("corner_tl", "corner_tr", "edge_top"):
            c = {"corner_tl": 0, "corner_tr": cols - 1, "edge_top": cols // 2}[lay]
            assert single(mask, 0, c) and fh[c] == rows and len(top) == 1
        elif lay in ("corner_bl", "corner_br", "edge_bottom"):
            c = {"corner_bl": 0, "corner_br": cols - 1, "edge_bottom": cols // 2}[lay]
            assert single(mask, last, c)
            if hr == 0 and rows > 1:
                assert fh[c] == last and prob[last, c] == hit and (prob[:last, c] == miss).all()
        elif lay in ("edge_left", "edge_right"):
            assert single(mask, rows // 2, 0 if lay == "edge_left" else cols - 1)
        elif lay == "row0":
            assert mask[0].all() and mask.sum() == cols and (fh == rows).all() and (prob == miss).all()
        elif lay == "last_row":
            assert mask[last].all() and mask.sum() == cols
            if hr == 0 and rows > 1:
                assert (fh == last).all() and (prob[last] == hit).all()
        elif lay == "full_column":
            assert mask[:, cols // 2].all() and mask.sum() == rows and fh[cols // 2] == rows
        elif lay == "checkerboard":
            assert mask.sum() == (rows * cols + 1) // 2 and mask[0, 0] == 1 and (rows * cols == 1 or not mask.all())
        elif lay == "every":
            assert mask.all() and (fh == rows).all() and (prob == miss).all()
        elif lay == "duplicates":
            assert len(case.hits) >= mask.sum() + 3 and len(np.unique(case.hits, axis=0)) == mask.sum()
        elif lay == "scatter":
            assert mask.any() and len(np.unique(case.hits, axis=0)) == len(case.hits) == mask.sum()
            assert rows < 8 or (not mask[:6].any() and mask.sum() < 0.2 * rows * cols)
        elif lay == "empty":
            assert len(case.hits) == 0 and not mask.any() and (prob == miss).all() and (fh == rows).all()
        elif lay == "neighbour_lit":
            # columns without a hit of their own whose first value above 0.5 comes from a neighbour's inflation
            lit = [c for c in range(cols) if not mask[:, c].any() and fh[c] < rows]
            assert lit and all(prob[fh[c], c] > F32(0.5) and prob[fh[c], c] < hit for c in lit)
            # ... and columns the inflation reaches without lifting them above 0.5: exactly 0.5 after the clip, so all miss
            dim = [c for c in range(cols) if st["filtered"][:, c].any() and fh[c] == rows and not mask[0, c]]
            assert dim
        elif lay == "exactly_half":
            gk = mapping_ref.getGaussianKernel
            kernel = gk(2 * case.hr + 1, -1).dot(gk(2 * case.hc + 1, -1).T)
            v = st["filtered"].astype(np.float64) / (kernel[case.hr, case.hc] / case.hit_prob)
            half = v == 0.5                             # in float64, before the cast and the clip
            assert half.any()
            # a line of pixels that reach exactly 0.5 and nothing more are no hit: with >= in place of > they would be
            quiet = [c for c in range(cols) if half[:, c].any() and not (v[:, c] > 0.5).any()] if case.hc else []
            rows_quiet = [r for r in range(rows) if half[r].any()] if case.hr else []
            assert quiet or rows_quiet
            assert all(fh[c] == rows for c in quiet)
            for r in rows_quiet:
                for c in np.nonzero(half[r])[0]:
                    assert fh[c] != r
        else:
            raise AssertionError("layout %r has no claim" % lay)
    if group != "specials":
        assert seen == set(E.layouts(3, 3))


def filtered_in_order(mask, k32, reverse):
    """mapping_ref.filter2D's sum with the taps taken in row-major order, or in the reverse of it"""
    kh, kw = k32.shape
    rows, cols = mask.shape
    pad = np.zeros((rows + kh - 1, cols + kw - 1), np.float32)
    pad[kh // 2:kh // 2 + rows, kw // 2:kw // 2 + cols] = mask
    out = np.zeros((rows, cols), np.float32)
    order = [(i, j) for i in range(kh) for j in range(kw)]
    for i, j in (order[::-1] if reverse else order):
        out = (out + k32[i, j] * pad[i:i + rows, j:j + cols]).astype(np.float32)
    return out


@pytest.mark.parametrize("group", ["40x33-hr4-hc4", "24x17-hr4-hc4", "40x33-hr5-hc2"])
def test_filtered_values_depend_on_the_summation_order(group):
    """the computed 9 x 9 kernel: where the hits of a window are not symmetric about its centre (clipped at a border, or a
    scattered pattern), the float32 taps summed in row-major order and in reverse give different bits"""
    case = [c for c in GROUPS[group] if c.layout == "scatter"][0]
    _, st = E.measure_ref(case)
    kernel = mapping_ref.getGaussianKernel(2 * case.hr + 1, -1).dot(mapping_ref.getGaussianKernel(2 * case.hc + 1, -1).T)
    k32 = kernel.astype(np.float32)
    fwd, rev = filtered_in_order(st["hits"], k32, False), filtered_in_order(st["hits"], k32, True)
    assert np.array_equal(fwd.view(np.int32), st["filtered"].view(np.int32))
    differ = fwd.view(np.int32) != rev.view(np.int32)
    assert differ.sum() >= 10, differ.sum()
    # ... and it reaches the image before logit: below the first hits the two orders end in different probabilities
    div = kernel[case.hr, case.hc] / case.hit_prob
    pf, pr = (np.clip((x / div).astype(np.float32), 0.5, F32(case.hit_prob)) for x in (fwd, rev))
    kept = np.arange(case.shape[0])[:, None] >= st["first_hits"][None, :]
    assert np.array_equal(pf[kept].view(np.int32), st["prob"][kept].view(np.int32))
    assert (pf.view(np.int32) != pr.view(np.int32))[kept].sum() >= 5


def test_exactly_half_needs_another_hit_prob_than_the_default():
    """no subset of OpenCV's fixed taps (1 x 3, 1 x 5, 1 x 7, 3 x 3, 3 x 5) gives exactly 0.5 before the clip at hit_prob 0.8;
    at 0.75 the 1 x 5 kernel does"""
    found = {0.8: 0, 0.75: 0}
    for hr, hc in ((0, 1), (0, 2), (0, 3), (1, 1), (1, 2)):
        kernel = mapping_ref.getGaussianKernel(2 * hr + 1, -1).dot(mapping_ref.getGaussianKernel(2 * hc + 1, -1).T)
        taps = kernel.astype(np.float32).ravel()
        sums = np.zeros(1, np.float64)
        for t in taps:                      # (dyadic taps: every partial sum is exact in float32, whatever the order)
            sums = np.unique(np.concatenate([sums, sums + np.float64(t)]))
        for hp in found:
            v = (sums / (kernel[hr, hc] / hp)).astype(np.float32)
            found[hp] += int((v == F32(0.5)).sum())
    assert found[0.8] == 0 and found[0.75] > 0


# ---- fit ------------------------------------------------------------------------------------------------------------------
def run_ref(case, check=None):
    m = E.ref_map(case.settings)
    E.run_session(m, case, Pose2, check=check and (lambda i: check(i, m)))
    return m


def add_quotients(case):
    """for a session that never grows: the quotients of every added keyframe's pixels, at the pose it was added with"""
    first = E.ref_map(case.settings)
    m = run_ref(case)
    assert [m.rows, m.cols, m.x0, m.y0] == [first.rows, first.cols, first.x0, first.y0]
    out = []
    for st in case.steps:
        if st[0] == "add":
            out.append((st[1],) + E.quotients(first, m.sonar_xy_of(m.keyframes[st[1]]).astype(np.float64), Pose2(*st[2])))
    return m, out


@pytest.mark.parametrize("case", [E.tie_session(), E.tie_session_quarter()], ids=lambda c: c.name)
def test_tie_cases_sit_exactly_on_halves(case):
    m, quots = add_quotients(case)
    ks = {"r": [], "c": []}
    for key, qr, qc in quots:
        for axis, q in (("r", qr), ("c", qc)):
            tie = q - np.floor(q) == 0.5
            ks[axis] += list(np.floor(q[tie]).astype(int))
    for axis in "rc":
        k = np.array(ks[axis])
        assert len(k) >= 8, (axis, len(k))
        assert (k % 2 == 0).any() and (k % 2 == 1).any() and (k == -1).any()       # k + 0.5 with k even, odd, and -0.5
    # -0.5 rounded to 0, not to -1: cells in row 0 and column 0, and the map as large as configured (add_quotients)
    assert min(int(kf.r.min()) for kf in m.keyframes) == 0 and min(int(kf.c.min()) for kf in m.keyframes) == 0


def test_coarse_map_has_crowded_cells_and_fine_map_has_none():
    case = E.dedup_session()
    first = E.ref_map(case.settings)
    st = case.steps[0]
    m = E.ref_map(case.settings)
    m.add_keyframe_logodds(st[1], Pose2(*st[2]), st[3], st[4])
    kf = m.keyframes[0]
    qr, qc = E.quotients(first, kf.sonar_xy.astype(np.float64), Pose2(*st[2]))
    cell = np.rint(qr).astype(np.int64) * first.cols + np.rint(qc).astype(np.int64)
    cells, counts = np.unique(cell, return_counts=True)
    assert counts.max() >= 10
    crowded = cells[np.argmax(counts)]
    # pixel p carries p + 1: the smallest pixel index of the cell is the one kept
    at = np.nonzero(kf.r.astype(np.int64) * m.cols + kf.c == crowded)[0][0]
    assert kf.l[at] == np.nonzero(cell == crowded)[0].min() + 1
    fine = run_ref(E.fine_session())
    for kf in fine.keyframes:
        assert len(kf.logodds) - len(kf.r) <= 0.01 * len(kf.logodds)


def test_window_case_is_one_column_wide_then_one_row_high_then_one_cell():
    case = E.window_session()
    seen = []
    spans = lambda m: [(len(np.unique(kf.r)), len(np.unique(kf.c)), len(kf.logodds)) for kf in m.keyframes]
    run_ref(case, lambda i, m: seen.append(spans(m)))
    adds = seen[2]
    assert adds[0][0] > 1 and adds[0][1] == 1
    assert adds[1][0] == 1 and adds[1][1] > 1
    assert adds[2][:2] == (1, 1)


def test_compaction_cases_hit_their_counts():
    t = E.compact_threads()
    counts = [c for c, _ in E.compact_sessions()]
    assert counts == [63, 64, 65, t - 1, t, t + 1]
    for count, case in E.compact_sessions():
        m = run_ref(case)
        assert len(m.keyframes[0].r) == count
        assert m.rows == 100 and m.cols == 100       # no growth: one fit, one window


def test_growth_steps_grow_as_named():
    case = E.growth_session()
    inc = int(E.GROW_SETTINGS["inc"] / E.GROW_SETTINGS["resolution"])
    prev = {}

    def check(i, m):
        if i < len(E.GROW_STEPS):
            key, _, top, bottom, left, right = E.GROW_STEPS[i]
            if prev:
                assert m.rows - prev["rows"] == top + bottom and m.cols - prev["cols"] == left + right
                assert m.y0 == prev["y0"] - top * m.resolution and m.x0 == prev["x0"] - left * m.resolution
                kf = m.keyframes[key]
                # one step: the outermost cell was at exactly -1, or at exactly rows / cols; two: further out than one step
                if top:
                    assert (kf.r.min() == inc - 1) if top == inc else (top == 2 * inc and kf.r.min() < inc)
                if bottom:
                    assert (kf.r.max() == prev["rows"]) if bottom == inc else \
                        (bottom == 2 * inc and kf.r.max() >= prev["rows"] + inc)
                if left:
                    assert (kf.c.min() == inc - 1) if left == inc else (left == 2 * inc and kf.c.min() < inc)
                if right:
                    assert (kf.c.max() == prev["cols"]) if right == inc else \
                        (right == 2 * inc and kf.c.max() >= prev["cols"] + inc)
        else:
            # the update_poses step: keyframe 0 went out on the left and then at the bottom, keyframe 5 came back to the middle
            assert m.cols > prev["cols"] and m.rows > prev["rows"] and m.x0 < prev["x0"] and m.y0 == prev["y0"]
        prev.update(rows=m.rows, cols=m.cols, x0=m.x0, y0=m.y0)

    run_ref(case, check)
    grown = [s[2:] for s in E.GROW_STEPS]
    for side in range(4):
        assert {g[side] for g in grown} == {0, inc, 2 * inc}


# ---- render ---------------------------------------------------------------------------------------------------------------
def test_render_cases_hold_ties_gates_and_empty_outputs():
    case = E.render_session()
    m = run_ref(case)
    res = m.resolution
    assert m.keyframes[2] is None and len(m.keyframes) == 5
    assert any(kw["frames"] and 2 in kw["frames"] and 99 in kw["frames"] for kw in case.pubs)
    ties = set()
    for kw in case.pubs:
        msg = m.get_occupancy_grid1(**kw)
        full = m.get_occupancy_grid1(frames=kw["frames"])
        h, w = full.info.height, full.info.width
        r = kw["resolution"]
        if r is None or r <= 0 or abs(r - res) <= 0.1 * res:
            # the 10 % gate (1.09 is inside it): no resize, the map's own resolution is published
            assert (msg.info.height, msg.info.width, msg.info.resolution) == (h, w, res)
            continue
        ratio = res / r
        assert (msg.info.height, msg.info.width) == (int(np.rint(h * ratio)), int(np.rint(w * ratio)))
        if r == 2 * res:
            for n in (h, w):
                if n % 2:
                    ties.add("up" if np.rint(n * ratio) > n * ratio else "down")
    assert ties == {"up", "down"}
    assert any(kw["resolution"] == res * 1.09 for kw in case.pubs) and any(kw["resolution"] == res * 1.11 for kw in case.pubs)
    # frames that name no keyframe at all: an empty image
    empty = m.get_occupancy_grid1(frames=[2, 99])
    assert (empty.info.height, empty.info.width, empty.data) == (0, 0, [])
    for r in E.REFUSED_RESOLUTIONS:
        with pytest.raises(AssertionError):
            m.get_occupancy_grid1(resolution=r)


def test_inexact_inverse_ratio_and_the_clamp_that_never_binds():
    case = E.render_session_fifth()
    assert any(kw["resolution"] == 0.3 for kw in case.pubs)
    assert 1.0 / (0.2 / 0.3) != 1.5
    ratios = set()
    for s in E.render_sessions():
        res = s.settings["resolution"]
        asked = [kw["resolution"] for kw in s.pubs if kw["resolution"] and kw["resolution"] > 0]
        ratios |= {res / r for r in asked if abs(r - res) > 0.1 * res}
    assert len(ratios) >= 5 and max(ratios) < 1
    for ratio in ratios:
        for n in range(1, 200):
            assert E.clamp_never_binds(n, ratio), (n, ratio)
    m = run_ref(case)
    for kw in case.pubs:
        m.get_occupancy_grid1(**kw)


def test_pixel_geometry_publishes_one_cell_or_none():
    case = E.pixel_session()
    m = run_ref(case)
    assert E.image_shape(case.settings, E.PIXEL_PING) == (1, 1)
    assert (m.rmin, m.cmin) == (m.rmax, m.cmax)
    sizes = {kw["resolution"]: m.get_occupancy_grid1(**kw).occ.shape for kw in case.pubs}
    assert sizes[0.5] == (1, 1) and sizes[0.75] == (1, 1) and sizes[1.0] == (0, 0)


def test_saturation_case_publishes_exact_0_and_100():
    case = E.saturation_session()
    m = run_ref(case)
    assert np.isfinite(m.logodds_grid).all() and np.abs(m.logodds_grid).max() > 1e38
    for v in (20.0, 40.0, 104.0, 1e38):
        assert v in E.SATURATING and -v in E.SATURATING
    for kw in case.pubs:
        msg = m.get_occupancy_grid1(**kw)
        p100 = (100 * msg.probs).astype(np.float32)
        # exactly 50 or 100, or so close to 0 that truncation cannot tell: nothing for data_agrees to excuse
        assert ((p100 == 50) | (p100 == 100) | ((p100 >= 0) & (p100 < 1e-6))).all() and (p100 == 0).any()
        assert {0, 100} <= set(msg.data) <= {0, 50, 100}


@pytest.mark.parametrize("name,ping,error", E.REFUSED_PINGS, ids=[r[0] for r in E.REFUSED_PINGS])
def test_reference_refuses_pings_below_four_beams(name, ping, error):
    m = E.ref_map(E.TIE_SETTINGS)
    with pytest.raises(error):
        m.add_keyframe_logodds(0, Pose2(0.0, 0.0, 0.0), ping, np.ones(8, np.float32))
