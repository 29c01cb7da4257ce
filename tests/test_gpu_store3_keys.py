"""GPU: the keyed clouds of the 3-D keyframe store (sfe_store3.hip, ``store.CloudStore3``: put_keys, get_points_keys, read_keys,
fov_select, set_selection, compact_selected, match_keys).  Every comparison is bit for bit (``np.array_equal``) against
tests/store3_keys_ref.py -- points, keys, selection bytes, histograms and counts are deterministic and all counts are integers,
so there are no tolerances.  tests/test_store3_keys_host.py shows on the CPU that every input holds what it was built for, and
that on every gate input but the on-the-bound one the device must decide every point (``n_ambiguous == 0`` is asserted here).

Shapes (the kernels: 256 lanes and one point per lane, 64-lane ballots, one-workgroup stages of 1024 threads, chunks of 1024
in the compaction, LDS tiles of 2048 target points): clouds of 0, 1, 257 points; job totals 1, 255 .. 257, 2047 .. 2049, 4097;
gates on 63 .. 65 and 255 .. 257 points; selections of 1023 .. 1025 and 2049; sources 1 .. 257 on targets 2047 .. 4097."""
import ctypes

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import pcl, store
from sonar_slam_amd.store import CloudStore, CloudStore3, fov3_numpy

import store3_keys_ref as K
import store3_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _state(s):
    st, off, cnt = s.meta()
    return len(s), st.tolist(), off.tolist(), cnt.tolist()


def _compact(s):
    _, off, cnt = s.meta()
    assert off[0] == 0 if len(off) else True
    assert np.array_equal(off[1:], (off + cnt)[:-1])


def _holds(s, h, pts, keys):
    h = int(h)
    assert s.is_keyed(h)
    got_p, got_k = s.read(h), s.read_keys(h)
    assert _same(got_p, np.ascontiguousarray(pts, f32).reshape(-1, 3)), (len(got_p), len(pts))
    assert _same(got_k, np.asarray(keys, np.int32).reshape(-1))


# ---- put_keys, read_keys, is_keyed ---------------------------------------------------------------------------------------------
def test_put_read_keyed(ctx):
    s = CloudStore3(ctx, capacity_points=1024, max_clouds=8)
    plain = s.put(R.cloud(1, 5))
    handles = []
    for n in (0, 1, 257):
        pts, keys = R.cloud(20 + n, n), np.random.default_rng(n).integers(0, 2 ** 31, n)
        h = s.put_keys(pts, keys, stamp=50 + n)
        _holds(s, h, pts, keys.astype(np.int32))
        handles.append(h)
    assert handles == [1, 2, 3] and not s.is_keyed(plain)
    assert s.meta()[0].tolist() == [0, 50, 51, 307] and s.meta()[2].tolist() == [5, 0, 1, 257]
    with pytest.raises(ValueError):
        s.is_keyed(4)
    with pytest.raises(L.SonarFEError, match="error -1"):            # SFE_ERR_ARG: a plain slot has no keys
        s.read_keys(plain)
    # the C entry point refuses a negative key (the Python layer would not let it through) and leaves no slot
    before = _state(s)
    pts, bad = R.cloud(3, 4), np.array([1, 2, -1, 3], np.int32)
    h = ctypes.c_int32(-7)
    rc = ctx.lib.sfe_cloud_store3_put_keys(ctx.handle, s.handle, 0, L.ptr(pts, ctypes.c_float), L.ptr(bad, ctypes.c_int32), 4,
                                           ctypes.byref(h))
    assert rc == -1 and h.value == -7 and _state(s) == before
    assert s.put_keys(pts, [1, 2, 0, 3]) == 4                         # the next handle is unchanged
    # a put that does not fit changes nothing
    before = _state(s)
    with pytest.raises(L.SonarFEError, match="error -4"):            # SFE_ERR_CAP
        s.put_keys(R.cloud(4, 1024), np.zeros(1024, np.int32))
    assert _state(s) == before
    # truncate releases a keyed slot: the handle handed out again is plain
    s.truncate(1)
    assert s.put(R.cloud(5, 3)) == 1 and not s.is_keyed(1)
    s.close()


def test_a_store_without_keys_refuses_the_keyed_calls(ctx):
    s = CloudStore3(ctx, capacity_points=256, max_clouds=4)
    a, b = s.put(R.cloud(1, 10)), s.put(R.cloud(2, 10))
    for call in (lambda: s.read_keys(a), lambda: s.fov_select([a], [[R.EYE]], [[1.0]], [[1.0]], 2),
                 lambda: s.set_selection(a, np.ones(10)), lambda: s.compact_selected([a]),
                 lambda: s.match_keys([[a, b]], [R.EYE], 1.0, 2)):
        with pytest.raises(L.SonarFEError, match="error -1"):
            call()
    assert len(s) == 2
    s.close()


# ---- get_points_keys ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", K.KEY_TOTALS)
def test_get_points_keys_totals(ctx, total):
    clouds, Hs, keys = K.keyed_job(total)
    s = CloudStore3(ctx, capacity_points=4 * total + 64, max_clouds=16)
    hs = [s.put(c) for c in clouds]
    res = 1.5                                                         # leaves of 0.75 .. 1.5 m in a 12 x 12 x 4 m box
    out = s.get_points_keys([hs], [Hs], [keys], res, stamps=[9])
    want_p, want_k = K.get_points_keys(clouds, Hs, keys, res)
    print("get_points_keys", total, "->", len(want_p), "keys", np.bincount(want_k).tolist())
    _holds(s, out[0], want_p, want_k)
    assert 0 < len(want_p) <= total and (total < 255 or len(want_p) < total)
    # the unkeyed call on the same inputs leaves the same points
    plain = s.get_points([hs], [Hs], res)
    assert _same(s.read(int(plain[0])), want_p) and not s.is_keyed(int(plain[0]))
    # the host-pointer descriptor overload on the host-built concatenation
    cat, tags = K.get_points_keys(clouds, Hs, keys, 0.0)
    hp, hk = pcl.downsample(cat, tags.astype(f32), res, ctx=ctx)
    assert _same(hp, want_p) and _same(hk.astype(np.int32), want_k)
    _compact(s)
    s.close()


def test_get_points_keys_without_downsample_and_leaf_extremes(ctx):
    clouds, Hs, keys = K.keyed_job(257)
    s = CloudStore3(ctx, capacity_points=4096, max_clouds=16)
    hs = [s.put(c) for c in clouds]
    cat, tags = K.get_points_keys(clouds, Hs, keys, 0.0)
    assert len(cat) == 257
    for res in (0.0, -1.0):                                           # the tagged concatenation itself
        out = s.get_points_keys([hs], [Hs], [keys], res)
        _holds(s, out[0], cat, tags)
    # one leaf per point: a resolution below the closest pair keeps every point, in leaf order
    want_p, want_k = K.get_points_keys(clouds, Hs, keys, 1e-4)
    assert len(want_p) == 257
    _holds(s, s.get_points_keys([hs], [Hs], [keys], 1e-4)[0], want_p, want_k)
    # one leaf for all: a resolution above the cloud's extent leaves one point with its cloud's key
    want_p, want_k = K.get_points_keys(clouds, Hs, keys, 100.0)
    assert len(want_p) == 1
    _holds(s, s.get_points_keys([hs], [Hs], [keys], 100.0)[0], want_p, want_k)
    _compact(s)
    s.close()


def test_get_points_keys_unused_empty_and_keyed_inputs(ctx):
    s = CloudStore3(ctx, capacity_points=1 << 13, max_clouds=32)
    a, b, e = R.cloud(41, 700), R.cloud(42, 300), np.zeros((0, 3), f32)
    Ha, Hb = R.motion(43), R.motion(45)
    ha, he = s.put(a), s.put(e)
    hb = s.put_keys(b, np.full(300, 99, np.int32))                    # a keyed input: its stored keys are ignored
    out = s.get_points_keys([[-1, ha, he, hb, -1], [he, -1], [], [hb]],
                            [[R.EYE, Ha, R.EYE, Hb, R.EYE], [R.EYE, R.EYE], [], [R.EYE]],
                            [[1, 4, 2, 6, 3], [8, 9], [], [5]], 0.5, stamps=[1, 2, 3, 4])
    want_p, want_k = K.get_points_keys([a, b], [Ha, Hb], [4, 6], 0.5)
    _holds(s, out[0], want_p, want_k)
    assert set(want_k.tolist()) == {4, 6}
    for j in (1, 2):                                                  # jobs without points: empty keyed slots
        _holds(s, out[j], np.zeros((0, 3), f32), np.zeros(0, np.int32))
    want_p, want_k = K.get_points_keys([b], [R.EYE], [5], 0.5)
    _holds(s, out[3], want_p, want_k)
    assert np.all(want_k == 5)
    assert _same(s.read_keys(hb), np.full(300, 99, np.int32))         # the input keeps its keys
    _compact(s)
    s.close()


def test_get_points_keys_coincident_points_keep_the_earlier_clouds_key(ctx):
    clouds, Hs, keys, res = K.coincident_job()
    s = CloudStore3(ctx, capacity_points=4096, max_clouds=8)
    hs = [s.put(c) for c in clouds]
    out = s.get_points_keys([hs], [Hs], [keys], res)
    want_p, want_k = K.get_points_keys(clouds, Hs, keys, res)
    _holds(s, out[0], want_p, want_k)
    assert (want_k == keys[0]).sum() == len(clouds[0]) and (want_k == keys[1]).sum() == 2
    s.close()


def test_get_points_keys_forty_jobs_then_fed_on(ctx):
    clouds, jobs = K.forty_keyed_jobs()
    s = CloudStore3(ctx, capacity_points=1 << 18, max_clouds=128)
    hs = [s.put(c) for c in clouds]
    out = s.get_points_keys([[hs[i] if i >= 0 else -1 for i in ids] for ids, _, _ in jobs], [Hs for _, Hs, _ in jobs],
                            [ks for _, _, ks in jobs], 0.75, stamps=list(range(40)))
    assert out.tolist() == list(range(len(hs), len(hs) + 40))
    wants = []
    for (ids, Hs, ks), h in zip(jobs, out):
        used = [(clouds[i], H, k) for i, H, k in zip(ids, Hs, ks) if i >= 0]
        want = K.get_points_keys([u[0] for u in used], [u[1] for u in used], [u[2] for u in used], 0.75)
        _holds(s, h, *want)
        wants.append(want)
    _compact(s)
    # outputs fed into the next call, under new keys: placed right behind
    pick = [1, 5, 17]
    Hs2 = [R.motion(70 + k, big=False) for k in range(3)]
    nxt = s.get_points_keys([[int(out[j]) for j in pick]], [Hs2], [[100, 101, 102]], 0.5)
    want = K.get_points_keys([wants[j][0] for j in pick], Hs2, [100, 101, 102], 0.5)
    _holds(s, nxt[0], *want)
    _compact(s)
    s.close()


def test_get_points_keys_overflow_changes_nothing(ctx):
    s = CloudStore3(ctx, capacity_points=1000, max_clouds=4)
    a, b = R.cloud(1, 400), R.cloud(2, 300)
    ha, hb = s.put(a), s.put_keys(b, np.arange(300))
    before = _state(s)
    with pytest.raises(L.SonarFEError, match="error -4"):            # the bound (400 + 300) exceeds the 300 points left
        s.get_points_keys([[ha, hb]], [[R.EYE, R.EYE]], [[0, 1]], 0.5)
    with pytest.raises(L.SonarFEError, match="error -4"):            # three jobs, two slots left
        s.get_points_keys([[hb], [], []], [[R.EYE], [], []], [[0], [], []], 0.5)
    assert _state(s) == before and s.is_keyed(hb) and not s.is_keyed(ha)
    out = s.get_points_keys([[hb]], [[R.EYE]], [[3]], 0.5)           # the bound fits exactly
    assert out[0] == 2
    _holds(s, out[0], *K.get_points_keys([b], [R.EYE], [3], 0.5))
    s.close()


# ---- fov_select -----------------------------------------------------------------------------------------------------------------
def _gate_held(s, handles, cases, n_keys, resolve=False):
    """cases: (points, keys, Hinvs, rb, bb) per handle"""
    hist, n_sel, n_amb = s.fov_select(handles, [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases], n_keys,
                                      resolve=resolve)
    assert hist.shape == (len(handles), n_keys) and hist.dtype == n_sel.dtype == n_amb.dtype == np.int32
    sels = []
    for j, (pts, keys, Hinvs, rb, bb) in enumerate(cases):
        sel = K.fov(pts, Hinvs, rb, bb)
        print("fov", len(pts), "points", len(Hinvs), "frames ->", int(sel.sum()), "selected; device", int(n_sel[j]),
              "ambiguous", int(n_amb[j]))
        assert n_amb[j] == 0
        assert n_sel[j] == sel.sum()
        assert np.array_equal(hist[j], K.key_counts(keys[sel == 1], n_keys))
        sels.append(sel)
    # the selection bytes on the device, through the compaction
    comp = s.compact_selected(handles)
    for h, (pts, keys, _, _, _), sel in zip(comp, cases, sels):
        _holds(s, h, *K.compact(pts, keys, sel))
    return sels


@pytest.mark.parametrize("n", K.FOV_SIZES)
def test_fov_select_sizes(ctx, n):
    case = K.fov_case(n, 2)
    s = CloudStore3(ctx, capacity_points=4 * n, max_clouds=8)
    h = s.put_keys(case[0], case[1])
    sel = _gate_held(s, [h], [case], 12)[0]
    assert 0 < sel.sum() < n
    s.close()


def test_fov_select_zero_frames_and_union_of_three(ctx):
    s = CloudStore3(ctx, capacity_points=4096, max_clouds=16)
    none = K.fov_case(300, 0)
    three = K.fov_case(500, 3)
    hn, h3 = s.put_keys(none[0], none[1]), s.put_keys(three[0], three[1])
    sels = _gate_held(s, [hn, h3], [none, three], 12)
    assert sels[0].sum() == 0
    each = [K.fov(three[0], three[2][f:f + 1], three[3][f:f + 1], three[4][f:f + 1]) for f in range(3)]
    assert all(0 < e.sum() < sels[1].sum() for e in each) and np.array_equal(sels[1], each[0] | each[1] | each[2])
    s.close()


def test_fov_select_several_jobs_of_different_sizes(ctx):
    cases = [K.fov_case(n, 1 + k % 3, seed=1) for k, n in enumerate(K.FOV_MULTI)]
    s = CloudStore3(ctx, capacity_points=8192, max_clouds=32)
    hs = [s.put_keys(c[0], c[1]) for c in cases]
    _gate_held(s, hs, cases, 12)
    _compact(s)
    s.close()


def test_fov_select_special_points(ctx):
    pts, keys, Hinvs, rb, bb, want, n_keys = K.fov_special()
    s = CloudStore3(ctx, capacity_points=256, max_clouds=8)
    h = s.put_keys(pts, keys)
    sel = _gate_held(s, [h], [(pts, keys, Hinvs, rb, bb)], n_keys)[0]
    assert np.array_equal(sel, want)
    hist, n_sel, _ = s.fov_select([h], [Hinvs], [rb], [bb], n_keys)
    assert n_sel[0] == want.sum() and hist[0].sum() == want.sum() - 2       # keys 4 and 9: selected, not counted
    s.close()


def test_fov_select_on_the_bearing_bound_is_resolved_by_numpy(ctx):
    pts, keys, Hinvs, rb, bb, i = K.fov_on_the_bearing_bound()
    s = CloudStore3(ctx, capacity_points=2048, max_clouds=8)
    h = s.put_keys(pts, keys)
    want = K.fov(pts, Hinvs, rb, bb)
    others = np.delete(np.arange(len(pts)), i)
    hist, n_sel, n_amb = s.fov_select([h], [Hinvs], [rb], [bb], 12, resolve=False)
    print("on the bound: device selected", int(n_sel[0]), "ambiguous", int(n_amb[0]), "numpy selects", int(want.sum()))
    assert n_amb[0] == 1 and n_sel[0] == want[others].sum()           # the undecided point is left unselected
    assert np.array_equal(hist[0], K.key_counts(keys[others][want[others] == 1], 12))
    _holds(s, s.compact_selected([h])[0], *K.compact(pts[others], keys[others], want[others]))
    hist, n_sel, n_amb = s.fov_select([h], [Hinvs], [rb], [bb], 12, resolve=True)
    assert n_amb[0] == 0 and n_sel[0] == want.sum() and np.array_equal(hist[0], K.key_counts(keys[want == 1], 12))
    assert np.array_equal(want, fov3_numpy(pts, Hinvs[0], rb[0], bb[0]).astype(np.uint8))
    _holds(s, s.compact_selected([h])[0], *K.compact(pts, keys, want))
    s.close()


# ---- set_selection, compact_selected ---------------------------------------------------------------------------------------------
def test_compact_selected_sizes_and_survivors(ctx):
    s = CloudStore3(ctx, capacity_points=1 << 16, max_clouds=64)
    cases = [(n, "half") for n in K.COMPACT_SIZES] + [(2600, "survivors:%d" % m) for m in K.COMPACT_SIZES[:3]] + \
            [(2049, "none"), (2049, "all"), (1, "all"), (0, "all")]
    hs, data = [], []
    for k, (n, kind) in enumerate(cases):
        pts, keys = R.cloud(300 + k, n), np.random.default_rng(k).integers(0, 30, n).astype(np.int32)
        sel = K.selection(n, kind, seed=k)
        h = s.put_keys(pts, keys)
        s.set_selection(h, sel)
        hs.append(h)
        data.append((pts, keys, sel))
    out = s.compact_selected(hs, stamps=list(range(len(hs))))
    for h, (pts, keys, sel), (n, kind) in zip(out, data, cases):
        want_p, want_k = K.compact(pts, keys, sel)
        print("compact", n, kind, "->", len(want_p))
        _holds(s, h, want_p, want_k)                                  # order kept: boolean indexing
    assert s.counts(out).tolist()[4:7] == list(K.COMPACT_SIZES[:3]) and s.counts(out).tolist()[7:9] == [0, 2049]
    _compact(s)
    # the host's selection replaces the device's; a compacted cloud has no selection of its own
    s.set_selection(hs[0], np.ones(K.COMPACT_SIZES[0]))
    _holds(s, s.compact_selected([hs[0]])[0], data[0][0], data[0][1])
    with pytest.raises(L.SonarFEError, match="error -1"):
        s.compact_selected([int(out[0])])
    with pytest.raises(L.SonarFEError, match="error -1"):            # n must equal the cloud's count
        s.set_selection(hs[0], np.ones(5))
    s.close()


def test_compact_selected_refusals_and_overflow(ctx):
    s = CloudStore3(ctx, capacity_points=1000, max_clouds=4)
    pts, keys = R.cloud(1, 400), np.arange(400, dtype=np.int32)
    h = s.put_keys(pts, keys)
    before = _state(s)
    with pytest.raises(L.SonarFEError, match="error -1"):            # no selection was ever written
        s.compact_selected([h])
    s.set_selection(h, np.arange(400) % 2)
    with pytest.raises(L.SonarFEError, match="error -4"):            # twice 400 points: the bound exceeds the 600 left
        s.compact_selected([h, h])
    assert _state(s) == before
    out = s.compact_selected([h])
    _holds(s, out[0], pts[1::2], keys[1::2])
    with pytest.raises(L.SonarFEError, match="error -4"):            # three slots for the two that are left
        s.compact_selected([h, h, h])
    s.truncate(1)
    assert _state(s) == before
    # the selection flag goes with the slot: after truncate and a new put the handle has none
    s.truncate(0)
    h = s.put_keys(pts, keys)
    with pytest.raises(L.SonarFEError, match="error -1"):
        s.compact_selected([h])
    s.close()


# ---- match_keys -----------------------------------------------------------------------------------------------------------------
def _match_held(s, pairs, Hs, data, max_dist, n_keys):
    hist, ov = s.match_keys(pairs, Hs, max_dist, n_keys)
    assert hist.shape == (len(pairs), n_keys) and hist.dtype == ov.dtype == np.int32
    assert np.array_equal(ov, s.overlap(pairs, Hs, max_dist))
    for j, (src, H, tgt, keys) in enumerate(data):
        want_h, want_o = K.match_keys(src, H, tgt, keys, max_dist, n_keys)
        print("match_keys", len(src), "on", len(tgt), "->", want_o, "device", int(ov[j]))
        assert ov[j] == want_o and np.array_equal(hist[j], want_h)
    return hist, ov


@pytest.mark.parametrize("nt", K.MATCH_TARGETS)
def test_match_keys_sizes(ctx, nt):
    s = CloudStore3(ctx, capacity_points=1 << 15, max_clouds=32)
    pairs, Hs, data = [], [], []
    for ns in K.MATCH_SOURCES:
        src, H, tgt, keys, max_dist = K.match_pair(ns, nt)
        pairs.append([s.put(src), s.put_keys(tgt, keys)])
        Hs.append(H)
        data.append((src, H, tgt, keys))
    hist, ov = _match_held(s, pairs, Hs, data, 0.3, 20)
    assert ov[-1] > 50 and np.all(hist.sum(axis=1) == ov)
    # n_keys below the largest key: the matches stay, the histogram loses the keys it has no room for
    hist7, ov7 = _match_held(s, pairs, Hs, data, 0.3, 7)
    assert np.array_equal(ov7, ov) and np.array_equal(hist7, hist[:, :7]) and hist7.sum() < hist.sum()
    s.close()


def test_match_keys_ties_go_to_the_lowest_index(ctx):
    src, tgt, keys, max_dist, pairs = K.tie_case()
    s = CloudStore3(ctx, capacity_points=8192, max_clouds=8)
    hs, ht = s.put(src), s.put_keys(tgt, keys)
    hist, ov = _match_held(s, [[hs, ht]], [R.EYE], [(src, R.EYE, tgt, keys)], max_dist, 40)
    assert ov[0] == len(pairs)
    for lo, hi in pairs:
        assert hist[0, keys[lo]] == 1 and hist[0, keys[hi]] == 0
    s.close()


def test_match_keys_radius_non_finite_and_empty(ctx):
    src, tgt, keys, max_dist, want, want_hist = K.radius_case()
    s = CloudStore3(ctx, capacity_points=256, max_clouds=16)
    hs, ht = s.put(src), s.put_keys(tgt, keys)
    hist, ov = _match_held(s, [[hs, ht]], [R.EYE], [(src, R.EYE, tgt, keys)], max_dist, 2)
    assert ov[0] == want and np.array_equal(hist[0], want_hist)
    # empty sides give zeros; a keyed cloud may be the source; a plain target is refused
    he, hek = s.put(np.zeros((0, 3), f32)), s.put_keys(np.zeros((0, 3), f32), [])
    hist, ov = s.match_keys([[he, ht], [hs, hek], [ht, ht]], [R.EYE] * 3, max_dist, 6)
    assert ov.tolist() == [0, 0, 3] and hist[:2].sum() == 0 and hist[2].tolist() == [1, 1, 0, 0, 0, 1]
    assert np.array_equal(ov, s.overlap([[he, ht], [hs, hek], [ht, ht]], [R.EYE] * 3, max_dist))
    with pytest.raises(L.SonarFEError, match="error -1"):
        s.match_keys([[ht, hs]], [R.EYE], max_dist, 2)
    # an infinite radius matches every finite source point, a NaN radius nothing
    hist, ov = s.match_keys([[hs, ht]], [R.EYE], np.inf, 6)
    assert ov[0] == np.isfinite(src).all(axis=1).sum() and ov[0] == s.overlap([[hs, ht]], [R.EYE], np.inf)[0]
    hist, ov = s.match_keys([[hs, ht]], [R.EYE], np.nan, 6)
    assert ov[0] == 0 and hist.sum() == 0
    s.close()


# ---- z = 0: the 2-D store on the (x, y) columns -----------------------------------------------------------------------------------
def _T6(H):
    H = np.asarray(H, f32)
    return np.array([H[0, 0], H[0, 1], H[0, 3], H[1, 0], H[1, 1], H[1, 3]], f32)


def test_planar_session_equals_the_2d_store(ctx):
    frames, poses = K.planar_session()
    s3 = CloudStore3(ctx, capacity_points=1 << 14, max_clouds=32)
    s2 = CloudStore(ctx, capacity_points=1 << 14, max_clouds=32)
    h3 = [s3.put(c) for c in frames]
    h2 = [s2.put(c[:, :2]) for c in frames]
    H = [np.asarray(P, f32) for P in poses]
    res, n_keys = 0.25, 3
    t3 = int(s3.get_points_keys([h3[:3]], [H[:3]], [[0, 1, 2]], res)[0])
    t2 = s2.get_points_keys(h2[:3], np.stack([_T6(x) for x in H[:3]]), [0, 1, 2], res, flags=store.F32_POINTS)
    p3, k3 = s3.read(t3), s3.read_keys(t3)
    assert np.all(p3[:, 2] == 0) and np.array_equal(p3[:, :2], s2.read(t2)) and np.array_equal(k3, s2.read_keys(t2))
    assert len(set(k3.tolist())) == 3
    Hinv = np.asarray(np.linalg.inv(poses[4]), f32)
    hist3, sel3, amb3 = s3.fov_select([t3], [[Hinv]], [[14.0]], [[1.2]], n_keys, resolve=False)
    hist2, sel2, amb2 = s2.fov_select(t2, _T6(Hinv), [14.0], [1.2], n_keys)
    assert amb3[0] == 0 and amb2 == 0 and sel3[0] == sel2 and np.array_equal(hist3[0], hist2) and 0 < sel2 < len(p3)
    c3, c2 = int(s3.compact_selected([t3])[0]), s2.compact_selected(t2)
    assert np.array_equal(s3.read(c3)[:, :2], s2.read(c2)) and np.array_equal(s3.read_keys(c3), s2.read_keys(c2))
    G = np.asarray(np.asarray(poses[4]) @ np.asarray(R.C.planar_motion(0.05, -0.03, 0.01)), f32)
    m3, o3 = s3.match_keys([[h3[4], c3]], [G], 0.5, n_keys)
    m2, o2 = s2.match_keys(h2[4], _T6(G), c2, 0.5, n_keys, flags=store.F32_POINTS)
    print("planar session: target", len(p3), "selected", int(sel2), "overlap", int(o2), "per key", m2.tolist())
    assert o3[0] == o2 and np.array_equal(m3[0], m2) and o2 > 10
    s3.close()
    s2.close()


# ---- a small session with a loop --------------------------------------------------------------------------------------------------
def test_loop_session_selection_over_handles_equals_the_host_route(ctx):
    frames, poses = K.loop_session()
    P = K.LOOP
    n_keys = len(frames)
    s = CloudStore3(ctx, capacity_points=1 << 16, max_clouds=64)
    hk = [s.put(c) for c in frames]
    tf, sf = list(K.LOOP_TARGET_FRAMES), list(K.LOOP_SOURCE_FRAMES)
    Hg = [np.asarray(poses[k], f32) for k in tf]
    Hinvs, rb, bb = K.loop_frames_bounds(sf)
    ref_inv = np.linalg.inv(poses[sf[0]])
    Hs = [np.asarray(ref_inv @ poses[k], f32) for k in sf]
    est = np.asarray(poses[sf[0]] @ R.C.rigid((0, 0, 1), 0.004, (0.03, -0.02, 0.01)), f32)      # the estimated source pose

    # over handles
    tgt = int(s.get_points_keys([[hk[k] for k in tf]], [Hg], [tf], P["resolution"])[0])
    hist, n_sel, n_amb = s.fov_select([tgt], [Hinvs], [rb], [bb], n_keys)
    assert n_amb[0] == 0
    near = int(s.compact_selected([tgt])[0])
    src = int(s.get_points([[hk[k] for k in sf]], [Hs], P["resolution"])[0])
    hist1, ov = s.match_keys([[src, near]], [est], P["max_dist"], n_keys)

    # through read, numpy and the host-pointer pcl calls (slam.py:873-902, :977-985)
    clouds = [s.read(h) for h in hk]
    cat = np.concatenate([R.transform(clouds[k], H) for k, H in zip(tf, Hg)])
    tags = np.concatenate([np.full(len(clouds[k]), k, f32) for k in tf])
    target_points, target_keys = pcl.downsample(cat, tags, P["resolution"], ctx=ctx)
    sel = np.zeros(len(target_points), bool)
    for H, r, b in zip(Hinvs, rb, bb):
        sel |= fov3_numpy(target_points, H, r, b)
    target_points, target_keys = target_points[sel], target_keys[sel]
    target_frames, counts = np.unique(np.int32(target_keys), return_counts=True)
    source_points = pcl.downsample(np.concatenate([R.transform(clouds[k], H) for k, H in zip(sf, Hs)]), P["resolution"], ctx=ctx)
    ids = pcl.match(target_points, R.transform(source_points, est), 1, P["max_dist"], ctx=ctx)[0][0]
    target_frames1, counts1 = np.unique(np.int32(target_keys[ids[ids != -1]]), return_counts=True)

    print("loop session: target", len(sel), "selected", int(sel.sum()), "per key", counts.tolist(), "overlap", int(ov[0]),
          "per key", counts1.tolist())
    assert _same(s.read(near), target_points) and _same(s.read_keys(near), np.int32(target_keys))
    assert n_sel[0] == sel.sum() and 100 < sel.sum() < len(sel)
    assert np.array_equal(hist[0], np.bincount(target_frames, weights=counts, minlength=n_keys).astype(np.int32))
    assert np.array_equal(hist1[0], np.bincount(target_frames1, weights=counts1, minlength=n_keys).astype(np.int32))
    assert ov[0] == (ids != -1).sum() and ov[0] > 50
    assert len(counts) > 1 and int(np.argmax(hist[0])) == int(target_frames[np.argmax(counts)])
    assert int(np.argmax(hist1[0])) == int(target_frames1[np.argmax(counts1)])
    # ... and the keyed target is the reference's
    _holds(s, tgt, *K.loop_target())
    s.close()
