"""Host side of the pcl edge cases (tests/pcl_edges.py), no GPU:

* building the cases asserts the property each one exists for (the constructors do it);
* the two references agree on every 2-D case: the C oracle on (x, y) and tests/pcl3_ref.py on (x, y, 0), bit for bit;
* the numpy model of the kernels' structure (``pcl_edges.model_*``) with no rule broken is the reference on every case;
* every deliberately wrong variant of the model is caught by the case named in ``CAUGHT_BY``, and every case moves at least
  one variant away from the reference -- except the ``DEGENERATE`` ones, whose answer no rule of the list can change;
* on the random match cases the float rule stays within its derived rounding bound of the float64 nearest neighbour;
* the rules settled with this suite: a point at d2 = +inf is nobody's neighbour (both references, max_dist = inf
  included), knn_density divides by the real neighbours, and the recorded difference at the 2-D level cap.
"""
import numpy as np
import pytest

import oracle
import pcl3_ref
import pcl_edges as E

KIND_DIM = [(k, d) for k in E.KINDS for d in (2, 3)]

# variant -> the case that must catch it (both widths)
CAUGHT_BY = {
    "match": {"le_update": "ties_across_tiles_knn1", "tile_local_index": "nearest_at_tile_edges_knn1",
              "best_reset": "nearest_at_tile_edges_knn1", "stale_tail": "knn_run_and_suffix_knn5",
              "lt_radius": "bound_0.5_knn1", "r2_other_precision": "bound_0.1_knn1", "fused": "fused_flips",
              "knn_no_index_clause": "ties_across_tiles_knn2", "knn_ge_index": "knn_run_and_suffix_knn2",
              "inf_is_neighbour": "nonfinite_knn4_inf", "nan_is_zero": "nonfinite_knn1_2"},
    "outlier": {"stale_tail": "sizes_2049", "lt_radius": "bound_0.5", "r2_other_precision": "bound_0.1", "fused": "bound_0.2",
                "count_ge": "count_exact_one_tile", "count_no_self": "count_exact_three_tiles",
                "unsigned_min_points": "min_points_-1"},
    "density": {"le_update": "lattice_ties", "knn_no_index_clause": "coincident", "density_div_knn": "far_points",
                "sqrt_approx": "sqrt_rounding", "inf_is_neighbour": "far_points"},
    "downsample": {"rank_desc_index": "sizes_257", "segment_wave_edge": "leaf_per_point_1025",
                   "leaf_cut_at_tile": "one_long_leaf", "nonpositive_is_identity": "split_to_cap_300_res-1"},
}
# cases whose answer none of the listed rules can change: one point against one point, an empty call, a threshold nobody meets
DEGENERATE = {"match": {"sizes_1_1_knn1", "no_queries"}, "outlier": {"min_points_300", "min_points_1000", "empty"},
              "density": set(), "downsample": set()}
# the variants most cases fall to, first: the search below stops at the first one that moves a case
FIRST = {"match": ("fused", "tile_local_index", "best_reset"), "outlier": ("count_ge", "lt_radius"), "density": ("sqrt_approx",),
         "downsample": ("rank_desc_index",)}


def _want(kind, c):
    want = E.KINDS[kind][2](*c.args)
    return want[1] if kind == "outlier" else want


def test_the_variant_table_is_complete():
    for kind, (_, _, _, variants) in E.KINDS.items():
        assert set(CAUGHT_BY[kind]) == set(variants), kind
        for dim in (2, 3):
            names = {c.name for c in E.cases(kind, dim)}
            assert set(CAUGHT_BY[kind].values()) <= names and DEGENERATE[kind] <= names
            assert all(c.why for c in E.cases(kind, dim))


@pytest.mark.parametrize("kind,dim", KIND_DIM)
def test_the_model_with_no_rule_broken_is_the_reference(kind, dim):
    model = E.KINDS[kind][1]
    for c in E.cases(kind, dim):
        assert E.same(kind, model(*c.args), _want(kind, c)), c.name


@pytest.mark.parametrize("kind", list(E.KINDS))
def test_the_references_agree_on_every_2d_case(kind):
    """oracle (x, y) == pcl3_ref (x, y, 0).  (oracle.match == oracle.match_knn for knn = 1 is asserted by ref_match.)"""
    for c in E.cases(kind, 2):
        want = E.KINDS[kind][2](*c.args)
        if kind == "match":
            ref, pts, knn, m = c.args
            ids, d2 = pcl3_ref.match_knn(E.z0(ref), E.z0(pts), knn, m)
            assert np.array_equal(ids, want[0]) and np.array_equal(E.bits(d2), E.bits(want[1])), c.name
        elif kind == "outlier":
            rows, keep = pcl3_ref.remove_outlier(E.z0(c.args[0]), c.args[1], c.args[2], return_mask=True)
            assert np.array_equal(E.bits(rows), E.bits(E.z0(want[0]))) and np.array_equal(keep, want[1]), c.name
        elif kind == "density":
            assert np.array_equal(E.bits(pcl3_ref.knn_density(E.z0(c.args[0]), c.args[1])), E.bits(want)), c.name
        else:
            out, idx = pcl3_ref.downsample(E.z0(c.args[0]), c.args[1])
            assert np.array_equal(idx, want[1]) and np.array_equal(E.bits(out), E.bits(E.z0(want[0]))), c.name


@pytest.mark.parametrize("kind,dim", KIND_DIM)
def test_every_wrong_variant_is_caught_by_its_named_case(kind, dim):
    model = E.KINDS[kind][1]
    missed = []
    for variant, name in sorted(CAUGHT_BY[kind].items()):
        c = E.case(kind, dim, name)
        if E.same(kind, model(*c.args, variant=variant), _want(kind, c)):
            missed.append((variant, name))
    assert not missed, missed


@pytest.mark.parametrize("kind,dim", KIND_DIM)
def test_every_case_moves_a_wrong_variant(kind, dim):
    model, variants = E.KINDS[kind][1], E.KINDS[kind][3]
    order = FIRST[kind] + tuple(v for v in variants if v not in FIRST[kind])
    idle = []
    for c in E.cases(kind, dim):
        want = _want(kind, c)
        if not any(not E.same(kind, model(*c.args, variant=v), want) for v in order):
            idle.append(c.name)
    assert set(idle) == DEGENERATE[kind], idle


@pytest.mark.parametrize("dim", [2, 3])
def test_the_float_rule_stays_within_its_bound_of_the_float64_nearest(dim):
    """the random part of the match cases only (pcl_edges.true_nearest_bound derives the bound; it is not tuned)"""
    checked = 0
    for c in E.cases("match", dim):
        if c.name.startswith("sizes_"):
            checked += E.check_against_float64(c, *E.ref_match(*c.args))
    assert checked > 1000


# ---- the rules settled with this suite -------------------------------------------------------------------------------------
FAR6 = np.array([[0, 0], [1, 0], [0, 1], [3e19, 0], [0, 3e19], [-3e19, -3e19]], np.float32)


def test_a_point_at_infinite_distance_is_nobodys_neighbour():
    """both references and both oracle entry points, max_dist = inf included (libnabo is not vendored: parity unpinned)"""
    for ids, d2 in (oracle.match_knn(FAR6, FAR6, 4, np.inf), pcl3_ref.match_knn(E.z0(FAR6), E.z0(FAR6), 4, np.inf),
                    E.model_match(FAR6, FAR6, 4, np.inf)):
        assert ids[:3, :3].tolist() == [[0, 1, 2], [1, 0, 0], [2, 2, 1]] and (ids[3, :3] == -1).all()
        assert ids[0, 3:].tolist() == [3, 4, 5] and (ids[1:, 3:] == -1).all()
        assert np.isinf(d2[ids == -1]).all() and np.isfinite(d2[ids >= 0]).all()
    ids1, _ = oracle.match(FAR6[3:], FAR6[:3], np.inf)
    assert (ids1 == -1).all()


def test_knn_density_divides_by_the_real_neighbours():
    want = oracle.knn_density(FAR6, 4)
    assert (want[:3] > 0).all() and np.isfinite(want[:3]).all() and np.isinf(want[3:]).all()
    assert np.array_equal(E.bits(pcl3_ref.knn_density(E.z0(FAR6), 4)), E.bits(want))
    assert np.array_equal(E.bits(E.model_density(FAR6, 4)), E.bits(want))
    # three real neighbours: 3 / volume, not 4 / volume
    r = np.float64(np.sqrt(np.float32(5.0) / np.float32(9.0)))
    assert abs(float(want[0]) / (3.0 / (4.0 / 3.0 * np.pi * r ** 3)) - 1) < 1e-5


def test_the_2d_level_cap_is_a_recorded_difference():
    """resolution 0: the oracle's recursion has no depth cap and separates the two tiny points; the 31-level key of
    ds_key_kernel cannot, and they share a leaf.  Neither is changed; both answers are pinned here."""
    out, idx = oracle.downsample(E.LEVEL_CAP_CLOUD, 0.0, return_index=True)
    assert idx.tolist() == E.LEVEL_CAP_ORACLE_IDX and len(out) == 5
    info = {}
    out, idx = E.model_downsample(E.LEVEL_CAP_CLOUD, 0.0, info=info)
    assert idx.tolist() == E.LEVEL_CAP_KERNEL_IDX and info["levels"] == 31
    key, _ = E.ds_keys(E.LEVEL_CAP_CLOUD, 0.0)
    assert key[2] == key[3] and len(np.unique(key)) == 4
