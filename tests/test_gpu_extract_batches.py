"""GPU parity of the batched extraction at the frame counts that change its launches ("What depends on the
frame count").  Several launch decisions of sonar_slam_amd/csrc/sfe_extract.hip hang on the number of frames in a call:
the workgroups per frame of extract_gather_kernel and their piece size (gather_shape, sfe_extract_shape.h; with them the
record layout that extract_merge_expand_kernel reads back), the chunks of ExtractCall::chunk = 1024 frames with their
seven pointer offsets, the 8-frame grid of the dense pass behind the gather of byte masks, the frame-striding waves of
extract_stage_fallback_kernel.  A mistake there gives a cloud that is plausible but belongs to another frame, lacks a
band or holds stale bits.  So: about a dozen distinct masks per geometry, dealt to the frames so that neighbours always
differ, and EVERY frame of every batch compared bit for bit, in np.nonzero order, with the oracle's cloud of the mask it
was given (computed once per distinct mask); counts for every frame; the output buffer pre-filled with a sentinel that
must survive behind every frame's points.  All calls go through the C ABI; CFAR is left out (covered elsewhere).  The
arithmetic of the launch shape itself is pinned on the CPU by tests/test_extract_shape_rules.py."""
import functools

import numpy as np
import pytest

import oracle
from sonar_slam_amd.feature_extraction import Geometry, build_maps, oculus_bearings

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
SPECIAL = (0, 63, 64, 1023, 1024)        # frames that must hold a cloud (+ the last of every batch): the edges of the
                                         # slice rule, of the per-frame rotation and of the chunks


class MaskSet(object):
    """The distinct masks of one geometry and what the oracle makes of them -- no GPU involved.
    masks[m]: uint8 polar image; pts[m]: oracle.px_to_m(oracle.nonzero(oracle.remap_u8(mask))), float64; words[m]: non-empty
    64-bit words of the canvas bitmap; streams[m]: the mask as a bit stream + the pad word (binary masks)."""

    def __init__(self, beams, ranges, res, cap, named_masks):
        _, self.height, _, self.width, _, self.mx, self.my = build_maps(oculus_bearings(beams), res, ranges)
        self.beams, self.ranges, self.cap = beams, ranges, cap
        self.names = [n for n, _ in named_masks]
        self.masks = np.stack([m for _, m in named_masks]).astype(np.uint8)
        self.binary = np.array([int(m.max(initial=0)) <= 1 for m in self.masks])
        self.pts, self.words = [], []
        for m in self.masks:
            rc = oracle.nonzero(oracle.remap_u8(m, self.mx, self.my))
            self.pts.append(oracle.px_to_m(rc, ranges, self.mx.shape[1], self.width, self.height))
            self.words.append(len(np.unique(rc[:, 0] * 4096 + rc[:, 1] // 64)))
        self.count = np.array([len(p) for p in self.pts])
        self.words = np.array(self.words)
        self.wpf = ranges * beams // 32 + 1
        self.streams = np.zeros((len(self.masks), self.wpf), np.uint32)
        self.streams[:, :self.wpf - 1] = np.packbits((self.masks != 0).reshape(len(self.masks), -1), axis=1,
                                                     bitorder="little").view(np.uint32)
        k = np.arange(len(self.masks))
        self.fit = [int(i) for i in k[self.binary & (self.count <= cap)]]                        # binary, within the capacity
        self.good = [int(i) for i in k[self.binary & (self.count > 0) & (self.count <= cap)]]    # ... and not empty
        self.over = [int(i) for i in k[self.binary & (self.count > cap)]]
        self.every = [int(i) for i in k[self.binary]]
        # masks with the same cloud count as one when neighbours must differ (a pixel that no canvas pixel taps is one more
        # empty mask: swapping the two would not show): cloud_id[m] = the first mask with the cloud of mask m
        self.cloud_id = np.array([next(j for j in range(i + 1) if np.array_equal(self.pts[j], self.pts[i]))
                                  for i in range(len(self.masks))])
        self._clouds = {}

    def index(self, name):
        return self.names.index(name)

    def capw(self):
        """a value for tuning extract_capw between the bitmap word counts of the non-empty fitting masks: the record path
        keeps the frames below it and hands the others back to the canvas kernels"""
        w = sorted(int(self.words[m]) for m in self.good)
        return (w[len(w) // 2 - 1] + w[len(w) // 2]) // 2

    def cloud(self, m):
        """the filtered cloud of mask m: feature_extraction.py:241-249 on the float32 points, by the oracle"""
        if m not in self._clouds:
            p = self.pts[m].astype(np.float32)
            self._clouds[m] = (oracle.remove_outlier(oracle.downsample(p, 0.5), 1.0, 5) if len(p) else p).reshape(-1, 2)
        return self._clouds[m]

    def deal(self, n, seed, pool=None, fixed=None):
        """mask index per frame: seeded, neighbours always hold different clouds, the SPECIAL frames and the last one are
        non-empty and within the capacity; fixed: {frame: mask} set by the caller"""
        rng = np.random.default_rng(seed)
        pool = self.every if pool is None else pool
        fixed = fixed or {}
        cid = self.cloud_id
        special = set(SPECIAL) | {n - 1}
        out = []
        for f in range(n):
            if f in fixed:
                m = fixed[f]
            else:
                c = [m for m in (self.good if f in special else pool)
                     if (not out or cid[m] != cid[out[-1]]) and (f + 1 not in fixed or cid[m] != cid[fixed[f + 1]])]
                m = c[int(rng.integers(len(c)))]
            out.append(m)
        a = np.array(out)
        assert np.all(cid[a[1:]] != cid[a[:-1]])
        for f in special:
            if f < n:
                assert 0 < self.count[a[f]] <= self.cap, f
        return a


@functools.lru_cache(maxsize=None)
def set_b():
    """geometry B: 256 beams x 512 ranges -> canvas 512 x 929, 15 words per row, 4096 stream words per frame"""
    rng = np.random.default_rng(1)
    beams, ranges = 256, 512
    shape = (ranges, beams)

    def pixel(y, x):
        m = np.zeros(shape, np.uint8)
        m[y, x] = 1
        return m

    def bands(rows):                       # what a sonar frame looks like: a few range bands
        m = np.zeros(shape, np.uint8)
        for r in rows:
            m[r:r + 3] = rng.random((3, beams)) < 0.5
        return m

    named = [("empty", np.zeros(shape, np.uint8)), ("pixel(0,0)", pixel(0, 0)), ("pixel(511,255)", pixel(511, 255))]
    named += [("density %g" % d, (rng.random(shape) < d).astype(np.uint8)) for d in (0.001, 0.003, 0.01)]
    named += [("bands %d" % i, bands(rows)) for i, rows in enumerate(((60, 200, 330), (10, 255, 500), (128, 131, 420)))]
    block = np.zeros(shape, np.uint8)
    block[200:204] = rng.random((4, beams)) < 0.5     # every detection inside one block of 4 polar rows
    named.append(("one block", block))
    named += [("density %g" % d, (rng.random(shape) < d).astype(np.uint8)) for d in (0.03, 0.1)]
    named.append(("ones", np.ones(shape, np.uint8)))
    # byte masks only (values > 1: cv2.remap's rounding depends on them, the dense pass takes these frames)
    d003, d01 = named[4][1], named[5][1]
    named.append(("all 255", d003 * np.uint8(255)))
    named.append(("1 and 2", d01 * rng.integers(1, 3, shape).astype(np.uint8)))
    named.append(("2 and 255", block * np.where(rng.random(shape) < 0.5, 2, 255).astype(np.uint8)))
    return MaskSet(beams, ranges, 30.0 / 512, 4096, named)


@functools.lru_cache(maxsize=None)
def set_c():
    """geometry C: 64 beams x 96 ranges -> canvas 96 x 175, 192 stream words: the stream-word cap holds slices at 3"""
    rng = np.random.default_rng(2)
    beams, ranges = 64, 96
    shape = (ranges, beams)
    named = [("empty", np.zeros(shape, np.uint8))]
    named += [("density %g" % d, (rng.random(shape) < d).astype(np.uint8)) for d in (0.01, 0.03, 0.1, 0.3)]
    band = np.zeros(shape, np.uint8)
    for r in (20, 50, 90):
        band[r:r + 3] = rng.random((3, beams)) < 0.5
    named.append(("bands", band))
    named.append(("ones", np.ones(shape, np.uint8)))
    named.append(("all 255", named[2][1] * np.uint8(255)))
    named.append(("1 and 2", named[3][1] * rng.integers(1, 3, shape).astype(np.uint8)))
    named.append(("2 and 255", band * np.where(rng.random(shape) < 0.5, 2, 255).astype(np.uint8)))
    named.append(("2 only", named[1][1] * np.uint8(2)))
    return MaskSet(beams, ranges, 0.25, 2048, named)


def check_mask_set_b(S):
    """what the tests below rely on, from the oracle alone"""
    assert S.names[0] == "empty" and S.count[0] == 0
    assert len(S.good) >= 7, S.count
    assert len(S.over) >= 2, S.count
    w = [int(S.words[m]) for m in S.good]
    assert min(w) < S.capw() < max(w) and sum(x > S.capw() for x in w) >= 2 and sum(x <= S.capw() for x in w) >= 2, w
    for name in ("all 255", "1 and 2", "2 and 255"):
        assert not S.binary[S.index(name)] and 0 < S.count[S.index(name)] <= S.cap, (name, S.count)
    # the remap's rounding: the byte values change the cloud
    assert S.count[S.index("all 255")] > S.count[S.index("density 0.003")]
    assert S.count[S.index("1 and 2")] != S.count[S.index("density 0.01")]


@pytest.fixture(scope="module")
def geom_b(ctx):
    S = set_b()
    check_mask_set_b(S)
    g = Geometry(ctx, S.mx, S.my, (S.ranges, S.beams), S.width, S.height)
    yield g, S
    g.close()


@pytest.fixture(scope="module")
def geom_c(ctx):
    S = set_c()
    g = Geometry(ctx, S.mx, S.my, (S.ranges, S.beams), S.width, S.height)
    yield g, S
    g.close()


def sentinel(n):
    return np.full(n, SENTINEL)


def knobs_of(S, hand_back):
    return {None: {}, "capw": {"extract_capw": S.capw()}, "rec_cap": {"extract_rec_cap": 64},
            "entries8": {"extract_compact": 0}}[hand_back]


def extract(ctx, g, S, deal, variant=0, knobs=None, byte_masks=False):
    """one call of sfe_extract_points_bits_batch_dev / sfe_extract_points_batch_dev -> counts, points [n][cap][2]"""
    n, cap = len(deal), S.cap
    src = S.masks[deal] if byte_masks else S.streams[deal]
    d_in, d_pts, d_cnt = ctx.alloc(src.nbytes), ctx.alloc(n * cap * 16), ctx.alloc(n * 4)
    try:
        d_in.upload(src)
        d_pts.upload(sentinel(n * cap * 2))
        fn = ctx.lib.sfe_extract_points_batch_dev if byte_masks else ctx.lib.sfe_extract_points_bits_batch_dev
        with ctx.tuning(**(knobs or {})):
            ctx._check(ctx.lib.sfe_extract_set_tuning(ctx.handle, variant))
            try:
                ctx._check(fn(ctx.handle, g.handle, d_in.ptr, n, cap, d_pts.ptr, d_cnt.ptr))
                ctx.sync()
            finally:
                ctx._check(ctx.lib.sfe_extract_set_tuning(ctx.handle, 0))
        return d_cnt.download(np.int32, n), d_pts.download(np.float64, n * cap * 2).reshape(n, cap, 2)
    finally:
        for b in (d_in, d_pts, d_cnt):
            b.free()


def check_points(S, deal, cnt, pts, what, frames=None, untouched=None):
    """every frame (or `frames`): the true count, the oracle's first min(count, cap) points bit for bit and in its order,
    the sentinel behind them; untouched: frames whose slots must hold nothing but the sentinel.  Frames are compared in
    groups of the same mask -- the same comparisons, one numpy call per mask."""
    deal = np.asarray(deal)
    sel = np.ones(len(deal), bool) if frames is None else np.asarray(frames)
    if untouched is not None:
        idx = np.nonzero(untouched)[0]
        bad = ~(pts[idx] == SENTINEL).all(axis=(1, 2))
        assert not bad.any(), "%s: frame %d was written" % (what, idx[bad][0])
    for m in np.unique(deal[sel]):
        idx = np.nonzero((deal == m) & sel)[0]
        want = S.pts[m]
        k = min(len(want), S.cap)
        bad = cnt[idx] != len(want)
        assert not bad.any(), "%s: frame %d (%s) reports %d points, the oracle has %d" % (
            what, idx[bad][0], S.names[m], cnt[idx[bad][0]], len(want))
        got = pts[idx]
        bad = ~((got[:, :k] == want[:k]).all(axis=(1, 2)))
        assert not bad.any(), "%s: frame %d (%s) holds other points than the oracle's" % (what, idx[bad][0], S.names[m])
        bad = ~((got[:, k:] == SENTINEL).all(axis=(1, 2)))
        assert not bad.any(), "%s: frame %d (%s) is written behind its %d points" % (what, idx[bad][0], S.names[m], k)


@pytest.mark.parametrize("n,variant,hand_back", [
    (1, 0, None), (63, 0, None), (64, 0, None), (300, 0, None), (512, 0, None), (1024, 0, None),
    (200, 2, None), (1024, 2, None), (40, 1, None),
    (300, 0, "capw"), (1024, 0, "capw"), (300, 0, "rec_cap"), (1024, 0, "rec_cap"), (300, 0, "entries8")])
def test_bit_stream_batches_at_the_frame_counts_that_change_the_gather_launch(ctx, geom_b, n, variant, hand_back):
    """sfe_extract_points_bits_batch_dev on geometry B (4096 stream words), one chunk.  What gather_shape makes of the frame
    counts (pinned by tests/test_extract_shape_rules.py, not asserted here):
        frames  variant      slices  piece_shift
        1, 63   default      64      0
        64      default      32      1             the record path switches to 32 slices
        300     default      27      1             32 pieces over 27 workgroups: five take two
        512     default      16      2             the bench regime
        1024    default      16      2
        200     2 (canvas)   40      0             64 pieces over 40 workgroups
        1024    2            8       3
        40      1                                  the dense pass for every frame
    capw: tuning extract_capw between the bitmap word counts of the fitting masks -- about half of the fitting frames leave
    the record path for the canvas kernels inside the batch; rec_cap: extract_rec_cap = 64, every frame with a detection
    does; entries8: the 8-byte inverse-map entries.  Masks above the capacity (true count, first cap points) are dealt
    in everywhere."""
    g, S = geom_b
    deal = S.deal(n, seed=100 + n + variant)
    cnt, pts = extract(ctx, g, S, deal, variant, knobs_of(S, hand_back))
    check_points(S, deal, cnt, pts, (n, variant, hand_back))


@pytest.mark.parametrize("n,variant,hand_back", [(1025, 0, None), (1100, 0, None), (2049, 0, None), (1100, 0, "capw"),
                                                 (1025, 2, None)])
def test_bit_stream_batches_of_more_than_one_chunk(ctx, geom_b, n, variant, hand_back):
    """More than ExtractCall::chunk = 1024 frames in one call: begin_chunk runs again with f0 > 0 (the offsets of the bit
    streams, points, counts), with another frame count and hence other slices and another record stride in the same scratch
    (1025: 16 slices, then 1 frame at 64; 1100: then 76 frames at 32; 2049: three chunks), and CleanBitmap carries what
    is known about the canvas bitmap from chunk to chunk.  Straight after each, 4 frames through the canvas kernels
    (variant 2) on the same context: a bit left behind in the bitmap would be a point there."""
    g, S = geom_b
    deal = S.deal(n, seed=200 + n + variant)
    cnt, pts = extract(ctx, g, S, deal, variant, knobs_of(S, hand_back))
    check_points(S, deal, cnt, pts, (n, variant, hand_back))
    after = np.array(S.good[:4])
    cnt, pts = extract(ctx, g, S, after, 2)
    check_points(S, after, cnt, pts, (n, variant, hand_back, "4 frames afterwards"))


@pytest.mark.parametrize("variant", [0, 2, 1])
def test_byte_mask_batches_with_non_binary_frames_beyond_the_dense_grid(ctx, geom_b, variant):
    """sfe_extract_points_batch_dev, 40 frames of geometry B.  Behind the gather the dense pass (extract_bits_kernel) is
    launched with a grid of 8 frames' tiles and strides over the rest, re-staging LDS per frame: frames 8, 17 and 39 are
    not binary (every set byte 255; 1 and 2 mixed; 2 and 255 mixed -- the remap's rounding makes their clouds differ from
    the binary mask's, the reference is the oracle on the byte values), all others are."""
    g, S = geom_b
    fixed = {8: S.index("all 255"), 17: S.index("1 and 2"), 39: S.index("2 and 255")}
    deal = S.deal(40, seed=300, fixed=fixed)
    assert [f for f in range(40) if not S.binary[deal[f]]] == [8, 17, 39]
    cnt, pts = extract(ctx, g, S, deal, variant, byte_masks=True)
    check_points(S, deal, cnt, pts, ("byte masks", variant))


def test_byte_mask_batch_of_two_chunks_on_a_small_geometry(ctx, geom_c):
    """1030 byte masks of geometry C (6 KB each; 192 stream words, so gather_shape is held at 3 slices by the words of a
    frame): non-binary frames at both ends of the dense pass's 8-frame grid, in the middle, and at both ends of both
    chunks -- the mask pointer, the packed bits and the non-binary flags of the second chunk."""
    g, S = geom_c
    assert len(S.good) >= 4 and len(S.over) >= 1, S.count
    nb = [S.index(x) for x in ("all 255", "1 and 2", "2 and 255", "2 only")]
    for m in nb:
        assert not S.binary[m] and 0 < S.count[m] <= S.cap, (S.names[m], S.count[m])
    assert S.count[nb[0]] > S.count[S.index("density 0.03")]
    fixed = {0: nb[0], 7: nb[1], 8: nb[2], 9: nb[3], 500: nb[0], 1023: nb[1], 1024: nb[2], 1029: nb[3]}
    deal = S.deal(1030, seed=400, fixed=fixed)
    assert [f for f in range(1030) if not S.binary[deal[f]]] == sorted(fixed)
    cnt, pts = extract(ctx, g, S, deal, 0, byte_masks=True)
    check_points(S, deal, cnt, pts, "geometry C")


@pytest.mark.parametrize("n", [300, 1100])
def test_staged_hand_over_and_resident_filters_on_large_batches(ctx, geom_b, n):
    """sfe_extract_points_bits_staged_dev -> sfe_cloud_filter_staged_dev(0.5, 1.0, 5) on 300 frames and on 1100 (two chunks:
    p32_out / bbox_out of the second one, cf_header_from_bbox_kernel beyond one block of 256 frames), fitting masks only.
    Every frame's cloud equals the oracle's remove_outlier(downsample(float32 points)) of its mask and what
    sfe_cloud_filter_batch_dev makes of the float64 points of the same batch.  With the extract_capw hand-back about half of
    the frames come through the canvas kernels and extract_stage_fallback_kernel, whose waves stride over the frames of
    both chunks.  want_points64 = 0: the float64 slots of the frames that stayed on the record path keep the sentinel
    (sonarfe.h), the others hold the frame's points; = 1: every frame's points."""
    g, S = geom_b
    cap = S.cap
    deal = S.deal(n, seed=500 + n, pool=S.fit)
    d_bits, d_pts, d_cnt = ctx.alloc(n * S.wpf * 4), ctx.alloc(n * cap * 16), ctx.alloc(n * 4)
    d_out, d_ocnt = ctx.alloc(n * cap * 8), ctx.alloc(n * 4)

    def check_clouds(what):
        ocnt = d_ocnt.download(np.int32, n)
        out = d_out.download(np.float32, n * cap * 2).reshape(n, cap, 2)
        for m in np.unique(deal):
            idx = np.nonzero(deal == m)[0]
            want = S.cloud(m)
            bad = ocnt[idx] != len(want)
            assert not bad.any(), "%s: frame %d (%s): %d points in the cloud, the oracle has %d" % (
                what, idx[bad][0], S.names[m], ocnt[idx[bad][0]], len(want))
            bad = ~((out[idx, :len(want)] == want).all(axis=(1, 2)))
            assert not bad.any(), "%s: frame %d (%s): another cloud than the oracle's" % (what, idx[bad][0], S.names[m])
        return ocnt, out

    try:
        d_bits.upload(S.streams[deal])
        # the unstaged path on the same batch
        d_pts.upload(sentinel(n * cap * 2))
        ctx._check(ctx.lib.sfe_extract_points_bits_batch_dev(ctx.handle, g.handle, d_bits.ptr, n, cap, d_pts.ptr, d_cnt.ptr))
        ctx._check(ctx.lib.sfe_cloud_filter_batch_dev(ctx.handle, d_pts.ptr, d_cnt.ptr, n, cap, 0.5, 1.0, 5, d_out.ptr, d_ocnt.ptr))
        ctx.sync()
        check_points(S, deal, d_cnt.download(np.int32, n), d_pts.download(np.float64, n * cap * 2).reshape(n, cap, 2), "unstaged")
        ref_cnt, ref_out = check_clouds("unstaged")
        for hand_back in (None, "capw"):
            back = (S.words[deal] > S.capw()) if hand_back else np.zeros(n, bool)     # frames that leave the record path
            assert not hand_back or (2 * n // 10 < back.sum() < 8 * n // 10)
            for want64 in (0, 1):
                what = (n, hand_back, want64)
                d_pts.upload(sentinel(n * cap * 2))
                d_out.zero()
                d_ocnt.zero()
                with ctx.tuning(**knobs_of(S, hand_back)):
                    ctx._check(ctx.lib.sfe_extract_points_bits_staged_dev(ctx.handle, g.handle, d_bits.ptr, n, cap, d_pts.ptr,
                                                                          want64, d_cnt.ptr))
                    ctx._check(ctx.lib.sfe_cloud_filter_staged_dev(ctx.handle, n, cap, 0.5, 1.0, 5, d_out.ptr, d_ocnt.ptr))
                    ctx.sync()
                cnt = d_cnt.download(np.int32, n)
                pts = d_pts.download(np.float64, n * cap * 2).reshape(n, cap, 2)
                assert np.array_equal(cnt, S.count[deal]), what
                if want64:
                    check_points(S, deal, cnt, pts, what)
                else:
                    check_points(S, deal, cnt, pts, what, frames=back, untouched=~back)
                ocnt, out = check_clouds(what)
                assert np.array_equal(ocnt, ref_cnt), what
                for f in range(n):
                    assert np.array_equal(out[f, :ocnt[f]], ref_out[f, :ocnt[f]]), (what, f)
    finally:
        for b in (d_bits, d_pts, d_cnt, d_out, d_ocnt):
            b.free()
