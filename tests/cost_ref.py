"""Plain numpy references for the matching-cost kernels (csrc/sfe_cost.hip: the dilated target grid of slam.py:505-527 and the
cost of slam.py:549-562), named WRONG variants of them, and the constructed cases that tests/test_gpu_cost_edges.py runs the
kernels on.  tests/test_cost_ref_host.py checks the references against the oracle and shows, on the CPU, that every case moves
the wrong variant it was built for -- so that a failure of the GPU suite points at a kernel.  No ctypes, no oracle and no
product code in here."""
import numpy as np

F32 = np.float32
LDS_WORDS = 24 * 1024       # COST_LDS_WORDS: grids of more 32-bit words are read through L2
COST_VARIANTS = ("mul_not_div", "half_away", "unfused", "res32_in_f64", "floor_cell")
GRID_VARIANTS = ("no_clip", "box")


# ---- references ---------------------------------------------------------------------------------------------------------------
def ellipse(hs):
    """cv2.getStructuringElement(MORPH_ELLIPSE, (2hs+1, 2hs+1)) as a 0/1 array: row dy of the element spans
    dx = rint(hs * sqrt((hs^2 - dy^2) / hs^2)) cells to either side of the centre (the division as OpenCV writes it, a
    multiplication by 1 / hs^2)."""
    hs = int(hs)
    size = 2 * hs + 1
    k = np.zeros((size, size), np.uint8)
    inv_r2 = 1.0 / (float(hs) * hs) if hs else 0.0
    for i in range(size):
        dy = i - hs
        dx = int(np.rint(hs * np.sqrt((float(hs) * hs - float(dy) * dy) * inv_r2)))
        k[i, max(hs - dx, 0):min(hs + dx + 1, size)] = 1
    return k


def grid(r, c, rows, cols, hs, variant=None):
    """target_grids after cv2.dilate (slam.py:515-527): the element ORed into a padded boolean array at every target, cropped
    -> rows x cols uint8 0 / 255.  The reference clips its targets into the grid first (slam.py:518-519); the C entry point
    takes them as given, so a target may also lie outside the grid here and reach into it with a part of its element.
    Wrong variants: ``no_clip`` drops a target whose element would leave the grid, ``box`` stamps a square element."""
    assert variant in (None,) + GRID_VARIANTS
    r, c = np.asarray(r, np.int64).reshape(-1), np.asarray(c, np.int64).reshape(-1)
    out = max([0] + (-r).tolist() + (r - (rows - 1)).tolist() + (-c).tolist() + (c - (cols - 1)).tolist())
    m = hs + int(out)                                      # the margin that holds every element whole
    el = (np.ones((2 * hs + 1, 2 * hs + 1), bool) if variant == "box" else ellipse(hs).astype(bool))
    pad = np.zeros((rows + 2 * m, cols + 2 * m), bool)
    for pr, pc in zip(r, c):
        if variant == "no_clip" and (pr - hs < 0 or pr + hs >= rows or pc - hs < 0 or pc + hs >= cols):
            continue
        pad[pr + m - hs:pr + m + hs + 1, pc + m - hs:pc + m + hs + 1] |= el
    return np.where(pad[m:m + rows, m:m + cols], 255, 0).astype(np.uint8)


OUTSIDE_SHAPES = ((5, 32, 2), (7, 31, 3), (40, 65, 10), (12, 70, 5), (60, 129, 17))


def outside_targets(rows, cols, hs):
    """targets up to hs + 2 cells OUTSIDE the grid on every side and beyond every corner: some reach in with the rim of their
    element, the farthest with nothing -> (r, c) int32"""
    pts = []
    for k in (1, max(hs - 1, 1), hs, hs + 1, hs + 2):
        pts += [(-k, cols // 4), (rows - 1 + k, cols // 2), (rows // 3, -k), (rows // 2, cols - 1 + k), (-k, -k),
                (rows - 1 + k, cols - 1 + k)]
    pts = np.unique(np.array(pts, np.int32), axis=0)
    return np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])


def cells_of_points(points32, xmin32, ymin32, res, rows, cols):
    """slam.py:514-519 for a float32 target cloud, as costgrid_stamp_points_kernel states it: np.round((p - min) /
    np.float32(res)) in float32, clamped to the grid; a point with a NaN quotient has no cell.  -> (r, c) of the others."""
    p = np.ascontiguousarray(points32, F32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        fc = np.round((p[:, 0] - F32(xmin32)) / F32(res))
        fr = np.round((p[:, 1] - F32(ymin32)) / F32(res))
    assert fc.dtype == F32 and fr.dtype == F32
    ok = ~(np.isnan(fr) | np.isnan(fc))
    r = np.clip(fr[ok], 0, rows - 1).astype(np.int32)
    c = np.clip(fc[ok], 0, cols - 1).astype(np.int32)
    return r, c


def fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays, rounded ONCE.  a * b is exact in double; its sum with c is rounded to odd in double
    (two-sum error term: if the sum is inexact and its last mantissa bit even, step to the neighbour on the error's side),
    after which the rounding to float32 is the correct one (53 >= 24 + 2 bits)."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.atleast_1d(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even.reshape(np.shape(s))
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(F32)


def _round(q, variant):
    if variant == "half_away":
        return np.sign(q) * np.floor(np.abs(q) + q.dtype.type(0.5))
    if variant == "floor_cell":
        return np.floor(q + q.dtype.type(0.5))
    return np.round(q)


def cell_floats(src32, T, xmin32, ymin32, res, f64, variant=None):
    """the rounded cell coordinates (fr, fc), still floats, of every source point under ONE transform T (six float32 numbers
    T00 T01 T02 T10 T11 T12): slam.py:549-556 in the dtype numpy evaluates it in.
      f64: the points and the transform widened to double, (px * T00 + py * T01) + T02, (x - float32 min) / float(res);
      else: float32 throughout, x = fl(fma(py, T01, fl(px * T00))) + T02 (sgemm), (x - min) / float32(res)."""
    assert variant in (None,) + COST_VARIANTS
    p = np.ascontiguousarray(src32, F32).reshape(-1, 2)
    T = np.asarray(T, F32).reshape(6)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if f64:
            px, py = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
            t = T.astype(np.float64)
            x = (px * t[0] + py * t[1]) + t[2]
            y = (px * t[3] + py * t[4]) + t[5]
            dx, dy = x - float(F32(xmin32)), y - float(F32(ymin32))
            if variant == "mul_not_div":
                rinv = 1.0 / float(res)
                qx, qy = dx * rinv, dy * rinv
            else:
                r = float(F32(res)) if variant == "res32_in_f64" else float(res)
                qx, qy = dx / r, dy / r
            assert qx.dtype == np.float64
        else:
            px, py = p[:, 0], p[:, 1]
            if variant == "unfused":
                x = (px * T[0] + py * T[1]) + T[2]
                y = (px * T[3] + py * T[4]) + T[5]
            else:
                x = fma32(py, T[1], px * T[0]) + T[2]
                y = fma32(py, T[4], px * T[3]) + T[5]
            qx, qy = (x - F32(xmin32)) / F32(res), (y - F32(ymin32)) / F32(res)
            assert qx.dtype == F32
        return _round(qy, variant), _round(qx, variant)


def hits(grid_u8, src32, T, xmin32, ymin32, res, f64, variant=None):
    """per source point: inside the grid (decided on the rounded float, so that NaN and huge values fail) and on a set cell"""
    rows, cols = grid_u8.shape
    fr, fc = cell_floats(src32, T, xmin32, ymin32, res, f64, variant)
    with np.errstate(invalid="ignore"):
        inside = (fr >= 0) & (fr < rows) & (fc >= 0) & (fc < cols)
    out = np.zeros(len(fr), bool)
    out[inside] = grid_u8[fr[inside].astype(np.int64), fc[inside].astype(np.int64)] > 0
    return out


def cost(grid_u8, src32, T6, xmin32, ymin32, res, f64, variant=None):
    """slam.py:549-562 for every transform of T6 [n x 6]: minus the number of source points on set cells -> int32 [n]"""
    T6 = np.ascontiguousarray(T6, F32).reshape(-1, 6)
    return np.array([-int(hits(grid_u8, src32, T, xmin32, ymin32, res, f64, variant).sum()) for T in T6], np.int32)


# ---- the constructed cases ----------------------------------------------------------------------------------------------------
def translation(tx, ty):
    return np.array([1, 0, tx, 0, 1, ty], F32)


def rotation(theta, tx=0.0, ty=0.0):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([c, -s, tx, s, c, ty], np.float64).astype(F32)


def checkerboard(rows, cols):
    """hs = 0 and a target on every cell with (r + c) even: any single wrong cell changes the count.
    -> (grid uint8, target rows, target columns)"""
    rr, cc = np.nonzero((np.add.outer(np.arange(rows), np.arange(cols)) & 1) == 0)
    g = np.zeros((rows, cols), np.uint8)
    g[rr, cc] = 255
    return g, rr.astype(np.int32), cc.astype(np.int32)


def _case(name, rows, cols, src, T6, xmin, ymin, res, dtypes, **more):
    g, tr, tc = checkerboard(rows, cols)
    d = dict(name=name, grid=g, tgt_r=tr, tgt_c=tc, rows=rows, cols=cols, hs=0, src=np.ascontiguousarray(src, F32).reshape(-1, 2),
             T6=np.ascontiguousarray(T6, F32).reshape(-1, 6), xmin=F32(xmin), ymin=F32(ymin), res=float(res), dtypes=tuple(dtypes))
    d.update(more)
    return d


def transposed(case):
    """the same case with x and y exchanged (grid, origin, points and transforms)"""
    t = dict(case)
    rows, cols = case["cols"], case["rows"]
    t["grid"], t["tgt_r"], t["tgt_c"] = checkerboard(rows, cols)
    assert np.array_equal(t["grid"], case["grid"].T)
    t.update(name=case["name"] + "_T", rows=rows, cols=cols, src=np.ascontiguousarray(case["src"][:, ::-1]),
             T6=np.ascontiguousarray(case["T6"][:, [4, 3, 5, 1, 0, 2]]), xmin=case["ymin"], ymin=case["xmin"])
    return t


TIE_LATTICE, TIE_DMAX = 1024, 60


def near_tie_lattice(res):
    """the d = k / 1024, 0 < d <= 60, whose quotient d * fl(1 / res) lies within 1e-9 (|q| + 1) of a half-way point (where
    cost_cell_f64 divides), and those for which rint(d * fl(1 / res)) != rint(d / res)  -> (d, differs)"""
    d = np.arange(1, TIE_DMAX * TIE_LATTICE + 1) / float(TIE_LATTICE)
    q = d * (1.0 / res)
    near = np.abs(np.abs(q - np.rint(q)) - 0.5) <= 1e-9 * (np.abs(q) + 1.0)
    differs = np.rint(q) != np.rint(d / res)
    keep = near | differs
    return d[keep], differs[keep]


NEAR_TIE_XMIN, NEAR_TIE_YMIN, NEAR_TIE_ROWS, NEAR_TIE_COLS = -16.0, -1.0, 6, 2051
NEAR_TIE_SHIFTS = (0.0, 0.5, -0.25, 0.125)


def near_tie_case(res):
    """float64 only.  xmin = -16; the source x runs over xmin + d - t for the near-tie lattice points d and the translations t
    of the pose set, each exactly a float32; the source row is one whose cell under the identity is set, so that any point
    moved by one column is lost.  Poses: the identity and dyadic pure translations."""
    d, _ = near_tie_lattice(res)
    dd = np.unique(np.concatenate([d - t for t in NEAR_TIE_SHIFTS]))
    dd = dd[(dd > 0) & (dd <= TIE_DMAX)]
    col = np.round(dd / res).astype(np.int64)
    row = 1 + (col + 1) % 2 + 2 * (np.arange(len(dd)) % 2)           # rows 1 .. 4 of 6, (row + col) even
    src = np.c_[NEAR_TIE_XMIN + dd, NEAR_TIE_YMIN + row * res].astype(F32)
    ty = 2.0 ** -5                                                   # a little more than a cell of 0.03 and less than one of 0.035
    T6 = [translation(0, 0), translation(0.5, 0), translation(-0.25, 0), translation(0.125, 0), translation(0.5, ty),
          translation(-0.25, -ty), translation(0.125, 2 * ty), translation(0, -2 * ty)]
    return _case("near_tie_%g" % res, NEAR_TIE_ROWS, NEAR_TIE_COLS, src, T6, NEAR_TIE_XMIN, NEAR_TIE_YMIN, res, (True,), d=dd)


TRUE_TIE_RES = 2.0 ** -4


def true_tie_case():
    """res = 2^-4 and every point on a k + 0.5 cell in x, in y or in both, -0.5 and rows - 0.5 (cols - 0.5) included: every
    quotient is exact and np.round's half-to-even decides.  An odd number of rows and an even number of columns, so that the
    last half-way point rounds into the grid on one axis and out of it on the other."""
    rows, cols, xmin, ymin, res = 37, 70, -2.0, 3.0, TRUE_TIE_RES
    kc, kr = np.arange(-1, cols), np.arange(-1, rows)
    both = np.stack(np.meshgrid(xmin + (kc + 0.5) * res, ymin + (kr + 0.5) * res), -1).reshape(-1, 2)
    in_x = np.stack(np.meshgrid(xmin + (kc + 0.5) * res, ymin + kr[1::5] * res), -1).reshape(-1, 2)
    in_y = np.stack(np.meshgrid(xmin + kc[1::7] * res, ymin + (kr + 0.5) * res), -1).reshape(-1, 2)
    src = np.concatenate([both, in_x, in_y])
    h = res / 2
    T6 = [translation(0, 0), translation(h, 0), translation(0, h), translation(res, 0), translation(-h, -h), translation(3 * res, h),
          translation(-2 * res, res), np.array([0, -1, 4.0, 1, 0, 2.0], F32), np.array([-1, 0, 1.0, 0, -1, 8.0], F32)]
    return _case("true_tie", rows, cols, src, T6, xmin, ymin, res, (True, False))


def edge_case():
    """points on the cells -1, 0, rows - 1, rows and on the columns -1, 0, 31, 32, 63, 64, cols - 1, cols (the word edges of
    the bit map), up to 0.3 cells off the centre"""
    rows, cols, xmin, ymin, res = 11, 97, -1.5, 2.25, 0.05
    rng = np.random.default_rng(101)
    er, ec = np.array([-1, 0, rows - 1, rows]), np.array([-1, 0, 31, 32, 63, 64, cols - 1, cols])
    cells = np.concatenate([np.stack(np.meshgrid(ec, np.arange(-1, rows + 1)), -1).reshape(-1, 2),
                            np.stack(np.meshgrid(np.arange(-1, cols + 1), er), -1).reshape(-1, 2)])
    cells = np.concatenate([cells, cells, cells]) + rng.uniform(-0.3, 0.3, (3 * len(cells), 2))
    src = np.c_[xmin + cells[:, 0] * res, ymin + cells[:, 1] * res]
    T6 = [translation(0, 0), translation(res, 0), translation(-res, 0), translation(0, res), translation(0, -res),
          translation(32 * res, res), translation(-31 * res, -res), translation(2 * res, 2 * res)]
    return _case("edge_of_grid", rows, cols, src, T6, xmin, ymin, res, (True, False))


NONFINITE = np.array([[np.nan, 1], [np.inf, 0], [1, -np.inf], [3e38, 3e38]], F32)


def nonfinite_case():
    """(nan, 1), (inf, 0), (1, -inf) and (3e38, 3e38) behind a normal cloud; none of them is inside under any pose"""
    rows, cols, xmin, ymin, res = 40, 70, -1.0, -1.0, 0.05
    rng = np.random.default_rng(102)
    src = np.concatenate([np.c_[rng.uniform(-1.2, 2.7, 300), rng.uniform(-1.2, 1.2, 300)].astype(F32), NONFINITE])
    T6 = [translation(0, 0), rotation(0.3, 0.2, -0.1), rotation(-0.7, 0.5, 0.4), translation(0.3, 0.3), rotation(1.5, 1.0, 0.0),
          rotation(3.0, 1.5, 0.5), rotation(0.1)]
    return _case("non_finite", rows, cols, src, T6, xmin, ymin, res, (True, False), n_bad=len(NONFINITE))


FMA_MIN_POINTS = 8


def fma_case():
    """float32 only.  A seeded search: random float32 points that a rotated pose moves into a window far from the origin (where
    an ulp of the sum is a few thousandths of a 1 cm cell); those whose cell differs between fl(fma(py, T01, fl(px * T00))) and
    fl(fl(px * T00) + fl(py * T01)) are kept, per pose, until there are enough of them.  Ordinary points go with them."""
    rows, cols, res = 50, 1000, 0.01
    xmin, ymin = F32(200.0), F32(100.0)
    rng = np.random.default_rng(103)
    T6, src, plain, n_found = [], [], [], []
    for theta in (0.4, -1.1, 2.3, 0.9, -2.6, 1.7):
        T = rotation(theta, 3.0, -2.0)
        A = T.astype(np.float64).reshape(2, 3)
        moved = np.c_[rng.uniform(200.5, 209.5, 100000), rng.uniform(100.05, 100.45, 100000)]
        p = np.linalg.solve(A[:, :2], (moved - A[:, 2]).T).T.astype(F32)
        fr, fc = cell_floats(p, T, xmin, ymin, res, False)
        ur, uc = cell_floats(p, T, xmin, ymin, res, False, "unfused")
        diff = np.nonzero(((fr != ur) ^ (fc != uc)))[0][:16]         # one cell off on exactly one axis: the other colour
        T6.append(T)
        src.append(p[diff])
        plain.append(p[:30 * len(T6)])                               # (only its own pose moves a point into the window)
        n_found.append(len(diff))
    found = np.concatenate(src)
    src = np.concatenate([found] + plain)
    return _case("fma", rows, cols, src, T6, xmin, ymin, res, (False,), n_found=n_found, found=found)


def random_case(seed=104, n=600):
    """an ordinary cloud under ordinary poses on a checkerboard of 3 cm cells (float(float32(0.03)) != 0.03 shows here)"""
    rows, cols, xmin, ymin, res = 700, 900, -12.0, -9.0, 0.03
    rng = np.random.default_rng(seed)
    src = np.c_[rng.uniform(-11, 13, n), rng.uniform(-8, 10, n)].astype(F32)
    T6 = [translation(0, 0)] + [rotation(t, x, y) for t, x, y in rng.uniform(-0.5, 0.5, (8, 3))]
    return _case("random_checkerboard", rows, cols, src, T6, xmin, ymin, res, (True, False))


def cell_cases():
    """every checkerboard case, by name"""
    cases = [near_tie_case(0.03), near_tie_case(0.035), true_tie_case(), edge_case(), nonfinite_case(), fma_case(), random_case()]
    cases += [transposed(cases[0]), transposed(cases[2])]
    return {c["name"]: c for c in cases}


STAMP_SHAPES = ((1, 1, 0), (1, 33, 17), (5, 32, 2), (7, 31, 3), (9, 64, 17), (40, 65, 10), (3, 97, 40), (50, 50, 0), (6, 96, 33))


def stamp_case(rows, cols, hs, sparse=False):
    """targets on all four corners, on the border midpoints and at random interior cells -> (r, c) int32.  With the larger
    elements these fill the small grids completely, so every shape also runs ``sparse``: ONE target in the last row, whose clipped
    element leaves cells unset on every side that the grid has room for."""
    if sparse:
        return np.array([rows - 1], np.int32), np.array([(5 * cols) // 12], np.int32)
    rng = np.random.default_rng(rows * 1000 + cols)
    pts = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (0, cols // 2), (rows - 1, cols // 2), (rows // 2, 0),
           (rows // 2, cols - 1)]
    if rows > 2 and cols > 2:
        n = max(1, min(6, (rows - 2) * (cols - 2) // 40))
        pts += list(zip(rng.integers(1, rows - 1, n), rng.integers(1, cols - 1, n)))
    pts = np.unique(np.array(pts, np.int32), axis=0)
    pts = pts[rng.permutation(len(pts))]
    return np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])


def centres(r, c, xmin, ymin, res):
    """the float32 cloud on the centres of the cells (r, c); exact for a dyadic origin and resolution"""
    return np.c_[xmin + np.asarray(c, np.float64) * res, ymin + np.asarray(r, np.float64) * res].astype(F32)


STAMP_POINTS_ITEMS = 32 * 256      # threads of one costgrid_stamp_points_kernel launch row: one item more takes the stride loop


def stamp_points_cases():
    """float32 target clouds for costgrid_stamp_points_kernel, by name: dicts of pts, xmin, ymin, res, rows, cols, hs"""
    rng = np.random.default_rng(105)
    out = {}
    # a grid tighter than the cloud: points clamp to row and column 0 and to the last row and column
    rows, cols, res, xmin, ymin = 30, 45, 0.05, F32(1.0), F32(-2.0)
    pts = np.c_[rng.uniform(0.5, 1.0 + cols * res + 0.5, 400), rng.uniform(-2.5, -2.0 + rows * res + 0.5, 400)].astype(F32)
    pts = np.concatenate([pts, np.array([[np.inf, -1.5], [2.0, -np.inf], [np.nan, -1.5], [2.0, np.nan]], F32)])
    out["clamped"] = dict(pts=pts, xmin=xmin, ymin=ymin, res=res, rows=rows, cols=cols, hs=3)
    # exact k + 0.5 cells at res = 2^-4
    rows, cols, res, xmin, ymin = 20, 40, TRUE_TIE_RES, F32(-2.0), F32(3.0)
    k = np.stack(np.meshgrid(np.arange(-1, cols, 3), np.arange(-1, rows, 2)), -1).reshape(-1, 2)
    pts = np.c_[xmin + (k[:, 0] + 0.5) * res, ymin + (k[:, 1] + 0.5) * res].astype(F32)
    out["half_cells"] = dict(pts=pts, xmin=xmin, ymin=ymin, res=res, rows=rows, cols=cols, hs=1)
    out["one_point"] = dict(pts=np.array([[0.26, 0.11]], F32), xmin=F32(0), ymin=F32(0), res=0.05, rows=9, cols=33, hs=2)
    out["empty"] = dict(pts=np.zeros((0, 2), F32), xmin=F32(0), ymin=F32(0), res=0.05, rows=9, cols=33, hs=2)
    # 2731 points x 3 element rows = 8193 items
    rows, cols, res = 60, 130, 0.05
    pts = np.c_[rng.uniform(0, (cols - 10) * res, 2731), rng.uniform(0, rows * res, 2731)].astype(F32)
    pts[-1] = ((cols - 3) * res, (rows - 2) * res)       # the last point alone in the empty columns: item 8193 is its last row
    out["8193_items"] = dict(pts=pts, xmin=F32(0), ymin=F32(0), res=res, rows=rows, cols=cols, hs=1)
    return out


def stamp_points_grid(case):
    r, c = cells_of_points(case["pts"], case["xmin"], case["ymin"], case["res"], case["rows"], case["cols"])
    return grid(r, c, case["rows"], case["cols"], case["hs"])


SOURCE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
POSE_COUNTS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 129)


def counts_case():
    """a blob grid (hs = 4), one cloud of 1025 points whose prefixes are the source clouds, 129 poses whose prefixes are the pose
    sets; the LAST point of every prefix lies on a target, so that a lost tail lane shows under the identity"""
    rows, cols, hs, xmin, ymin, res = 90, 150, 4, F32(-3.0), F32(-2.0), 0.05
    rng = np.random.default_rng(106)
    tr, tc = rng.integers(0, rows, 60).astype(np.int32), rng.integers(0, cols, 60).astype(np.int32)
    src = np.c_[rng.uniform(-3, 4.5, 1025), rng.uniform(-2, 2.5, 1025)].astype(F32)
    for k, n in enumerate(SOURCE_SIZES[1:]):
        src[n - 1] = (xmin + tc[k] * res, ymin + tr[k] * res)
    T6 = np.array([translation(0, 0)] + [rotation(t, x, y) for t, x, y in rng.uniform(-0.3, 0.3, (128, 3))], F32)
    return dict(name="counts", grid=grid(tr, tc, rows, cols, hs), tgt_r=tr, tgt_c=tc, rows=rows, cols=cols, hs=hs, src=src, T6=T6,
                xmin=xmin, ymin=ymin, res=res)


LDS_SHAPES = {"lds_exact": (768, 1024), "one_row_more": (769, 1024), "partial_last_word": (768, 1000)}


def lds_case(rows, cols):
    """a few dozen targets with hs = 10, the last row and column among them, and a source cloud of 300 points, a third of it in
    the last rows and columns; 33 poses (the first 9: the small launch)"""
    hs, xmin, ymin, res = 10, F32(-25.0), F32(-19.0), 0.05
    rng = np.random.default_rng(rows * 10000 + cols)
    tr = np.r_[rng.integers(0, rows, 30), rows - 1, rows - 1, rows - 3, rng.integers(rows - 12, rows, 6), rows // 2, 0]
    tc = np.r_[rng.integers(0, cols, 30), cols - 1, cols // 3, cols - 2, rng.integers(0, cols, 6), cols - 1, 0]
    tr, tc = tr.astype(np.int32), tc.astype(np.int32)
    near = rng.integers(0, len(tr), 300)                           # source points around the targets ...
    cell = np.c_[tc[near], tr[near]] + rng.uniform(-14, 14, (300, 2))
    cell[200:250, 1] = rows - 1 - rng.uniform(-1, 12, 50)          # ... and in the last rows and columns
    cell[250:, 0] = cols - 1 - rng.uniform(-1, 12, 50)
    cell[200:250, 0] = tc[31] + rng.uniform(-12, 12, 50)
    cell[250:, 1] = tr[39] + rng.uniform(-12, 12, 50)
    src = np.c_[xmin + cell[:, 0] * res, ymin + cell[:, 1] * res].astype(F32)
    T6 = np.array([translation(0, 0)] + [rotation(t, x, y) for t, x, y in rng.uniform(-0.01, 0.01, (32, 3)) * [1, 20, 20]], F32)
    return dict(name="%dx%d" % (rows, cols), grid=grid(tr, tc, rows, cols, hs), tgt_r=tr, tgt_c=tc, rows=rows, cols=cols, hs=hs,
                src=src, T6=T6, xmin=xmin, ymin=ymin, res=res)
