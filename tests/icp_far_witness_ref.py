"""numpy restatement of the two-level witness grid of the ICP target preparation (sweep_grid_witness and the grid
sizing of icp_sweep_prep_kernel, sfe_icp_sweep_prep.hip), in the kernel's float32 arithmetic.

S is the prepared target as the kernel holds it: the centred cloud in the strip layout, float32 [len + 2, 2], NaN
sentinels included (position 0 is one); a grid cell holds the position of its witness in S, 0 = none.

* geometry(S, nt, gm): the box, the cell size and the cell counts (the fields of StripTab).
* claim(S, geo): every finite point claims its cell; the point nearest to the centre, to the 16 bits of the distance
  that are kept, wins, the lower position among equals.
* dilate_fine(grid, S, geo, chunk): the SW_GRID_SWEEPS sweeps of the fine level.  The kernel sweeps in place: a thread
  reads what threads before it may already have written.  A workgroup of one wave (the 64-thread build) is
  deterministic -- 64 consecutive cells are read together and written together, chunk after chunk: chunk = 64
  restates it exactly.  chunk = None sweeps synchronously: a lower bound of what any order fills.
* coarse_level(grid, S, geo): the second level, from the fine grid after its sweeps -> (shift, cnx, cny, cells, sweeps).
* hand_over(grid, S, geo, level): the coarse witnesses handed to the fine cells that are still empty -> the final grid.
"""
import numpy as np

F32 = np.float32
GRID_SWEEPS = 4        # SW_GRID_SWEEPS
COARSE_SHIFT = 3       # SW_COARSE_SHIFT
COARSE_MAX = 256       # SW_COARSE_MAX
COARSE_SWEEPS = 256    # SW_COARSE_SWEEPS
NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]   # (dx, dy) in the kernel's order


def _dist2(ax, ay, bx, by):
    """fl(fl(dx * dx) + fl(dy * dy)) on float32 arrays"""
    dx = (ax - bx).astype(F32)
    dy = (ay - by).astype(F32)
    return ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)


def geometry(S, nt, gm):
    fin_x = S[np.abs(S[:, 0]) < np.inf, 0]
    fin_y = S[np.abs(S[:, 1]) < np.inf, 1]
    some_x, some_y = len(fin_x) > 0, len(fin_y) > 0
    x0, x1 = (fin_x.min(), fin_x.max()) if some_x else (F32(0), F32(0))
    y0, y1 = (fin_y.min(), fin_y.max()) if some_y else (F32(0), F32(0))
    ex, ey = F32(x1 - x0), F32(y1 - y0)
    tiny = F32(1e-30)
    area = F32(max(ex, tiny) * max(ey, tiny))
    cs = np.sqrt(F32(area / F32(max(nt, 1))))
    cs = max(cs, np.sqrt(F32(area / F32(gm // 2))))
    if not (cs > 0 and cs < np.inf):
        cs = F32(1)
    gnx = int(min(F32(ex / cs), F32(4096))) + 1
    gny = int(min(F32(ey / cs), F32(4096))) + 1
    while gnx * gny > gm:
        if gnx >= gny:
            gnx = (gnx + 1) // 2
        else:
            gny = (gny + 1) // 2
    csz = max(max(F32(ex / F32(gnx)), F32(ey / F32(gny))), tiny)
    with np.errstate(over="ignore"):
        ginv = F32(F32(1) / csz)
    if not ginv < np.inf:
        ginv = F32(0)
    return dict(gx0=F32(x0), gy0=F32(y0), ginv=ginv, gnx=gnx, gny=gny)


def _cs(geo):
    return F32(F32(1) / geo["ginv"]) if geo["ginv"] > 0 else F32(0)


def _centres(geo, shift=0):
    """centres of the cells of the fine grid (shift = 0) or of the coarse level -> (nx, ny, cx [n], cy [n])"""
    nx, ny = ((geo["gnx"] - 1) >> shift) + 1, ((geo["gny"] - 1) >> shift) + 1
    cs = F32(F32(1 << shift) * _cs(geo)) if shift else _cs(geo)
    ix, iy = np.tile(np.arange(nx), ny), np.repeat(np.arange(ny), nx)
    cx = (geo["gx0"] + ((ix.astype(F32) + F32(0.5)) * cs).astype(F32)).astype(F32)
    cy = (geo["gy0"] + ((iy.astype(F32) + F32(0.5)) * cs).astype(F32)).astype(F32)
    return nx, ny, cx, cy


def cell_of(x, y, geo):
    """the cell of a point (a target or a query), as prep and loop kernel compute it; NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        gx = ((np.asarray(x, F32) - geo["gx0"]).astype(F32) * geo["ginv"]).astype(F32)
        gy = ((np.asarray(y, F32) - geo["gy0"]).astype(F32) * geo["ginv"]).astype(F32)
        gx = np.where(gx > 0, np.minimum(gx, F32(geo["gnx"] - 1)), F32(0))      # fminf(fmaxf(v, 0), n - 1), NaN -> 0
        gy = np.where(gy > 0, np.minimum(gy, F32(geo["gny"] - 1)), F32(0))
    return gy.astype(np.int64) * geo["gnx"] + gx.astype(np.int64)


def _claim_min(n, cells, cx, cy, S, pos):
    """per cell the smallest (distance to the centre, top 16 bits) << 16 | position among `pos` -> position, 0 = none"""
    key = (_dist2(cx[cells], cy[cells], S[pos, 0], S[pos, 1]).view(np.uint32) & np.uint32(0xFFFF0000)) | pos.astype(np.uint32)
    best = np.full(n, 0xFFFFFFFF, np.uint32)
    np.minimum.at(best, cells, key)
    return np.where(best == 0xFFFFFFFF, 0, best & 0xFFFF).astype(np.int64)


def claim(S, geo):
    ln = len(S) - 2
    nx, ny, cx, cy = _centres(geo)
    if ln >= 65536:
        return np.zeros(nx * ny, np.int64)
    pos = np.arange(1, ln)
    pos = pos[(np.abs(S[pos, 0]) < np.inf) & (np.abs(S[pos, 1]) < np.inf)]
    return _claim_min(nx * ny, cell_of(S[pos, 0], S[pos, 1], geo), cx, cy, S, pos)


def _sweep(grid, S, nx, ny, cx, cy, cells):
    """one dilation step of `cells` (indices) read from `grid` -> their new values"""
    iy, ix = cells // nx, cells % nx
    out = grid[cells].copy()
    best = np.full(len(cells), np.inf, F32)
    for dx, dy in NEIGHBOURS:
        jx, jy = ix + dx, iy + dy
        ok = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny)
        w = np.where(ok, grid[np.where(ok, jy * nx + jx, 0)], 0)
        d = _dist2(cx[cells], cy[cells], S[w, 0], S[w, 1])
        take = (grid[cells] == 0) & (w != 0) & (d < best)
        best = np.where(take, d, best)
        out = np.where(take, w, out)
    return out


def dilate_fine(grid, S, geo, chunk=None):
    nx, ny, cx, cy = _centres(geo)
    grid = grid.copy()
    n = nx * ny
    step = chunk or n
    for _ in range(GRID_SWEEPS):
        for c0 in range(0, n, step):
            cells = np.arange(c0, min(c0 + step, n))
            grid[cells] = _sweep(grid, S, nx, ny, cx, cy, cells)
    return grid


def coarse_level(grid, S, geo):
    shift = COARSE_SHIFT
    while (((geo["gnx"] - 1) >> shift) + 1) * (((geo["gny"] - 1) >> shift) + 1) > COARSE_MAX:
        shift += 1
    cnx, cny, cx, cy = _centres(geo, shift)
    full = np.flatnonzero(grid)
    cc = ((full // geo["gnx"]) >> shift) * cnx + ((full % geo["gnx"]) >> shift)
    cells = _claim_min(cnx * cny, cc, cx, cy, S, grid[full])
    sweeps = 0
    every = np.arange(cnx * cny)
    for _ in range(COARSE_SWEEPS):
        new = _sweep(cells, S, cnx, cny, cx, cy, every)
        if np.array_equal(new, cells):
            break
        cells = new
        sweeps += 1
    return shift, cnx, cny, cells, sweeps


def hand_over(grid, S, geo, level):
    shift, cnx, _, cells, _ = level
    c = np.arange(len(grid))
    cc = ((c // geo["gnx"]) >> shift) * cnx + ((c % geo["gnx"]) >> shift)
    return np.where(grid != 0, grid, cells[cc])


def two_level(S, geo, chunk=None):
    """the grid the preparation stores -> (final grid, claimed cells, fine level after its sweeps, coarse level)"""
    claimed = claim(S, geo)
    fine = dilate_fine(claimed, S, geo, chunk)
    level = coarse_level(fine, S, geo)
    return hand_over(fine, S, geo, level), claimed, fine, level
