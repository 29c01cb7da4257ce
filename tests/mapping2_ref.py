"""Independent numpy restatement of bruce_slam's point-projection occupancy map (mapping.py:357-439, get_occupancy_grid2)
and of the two OpenCV calls it makes (tests only: the oracle of tests/test_mapping2_host.py and tests/test_gpu_mapping2.py).

  * ``getStructuringElement(MORPH_ELLIPSE, (n, n))`` for odd n = 2 h + 1: row i covers the columns within
    cvRound(h * sqrt((h^2 - (i - h)^2) / h^2)) of the centre (the row spans of OpenCV's ellipse element; h = 0: one cell);
  * ``dilate(mask, element)`` anchored at the centre with a constant border: a cell is set when any set cell lies under the
    element centred on it (the element is symmetric, so the reflection does not matter).

The map itself is written from the semantics, not from the product: the free cells are marked on the image of the map's
box and the known region is read off that image; the product takes the union of the keyframes' boxes instead.
"""
import numpy as np

from mapping_ref import resize_nearest


def ellipse_element(n):
    assert n % 2 == 1 and n >= 1
    h = n // 2
    k = np.zeros((n, n), bool)
    for i in range(n):
        dy = i - h
        dx = int(np.rint(h * np.sqrt((h * h - dy * dy) / float(h * h)))) if h else 0
        k[i, max(h - dx, 0):min(h + dx + 1, n)] = True
    return k


def dilate(mask, element):
    h = element.shape[0] // 2
    rows, cols = mask.shape
    pad = np.zeros((rows + 2 * h, cols + 2 * h), bool)
    pad[h:h + rows, h:h + cols] = mask
    out = np.zeros((rows, cols), bool)
    for i, j in zip(*np.nonzero(element)):
        out |= pad[i:i + rows, j:j + cols]
    return out


def select(point_cloud, frames):
    """the points method 2 projects: x, y of the whole cloud, or of the rows keyed (column 3) by each listed frame, in list
    order, float64"""
    if frames is None:
        return point_cloud[:, :2]
    keys = point_cloud[:, 3].astype(np.uint32)
    rows = [np.nonzero(keys == k)[0] for k in frames]
    idx = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    return point_cloud[idx, :2].astype(np.float64)


def occupancy_grid2(m, cells, point_cloud, remove_outlier, frames=None, resolution=None):
    """``m``: the map's x0, y0, resolution, rmin / rmax / cmin / cmax, dilate_size, outlier_filter_radius / _min_points;
    ``cells[k]``: (r, c) of keyframe k in the grid's current coordinates, None for a missed key.
    -> dict(data int8 [h x w], info = (x, y, width, height, resolution), box = (rmin, rmax, cmin, cmax), points, kept)"""
    points = select(point_cloud, frames)
    occ = np.full((m.rmax - m.rmin + 1, m.cmax - m.cmin + 1), -1, np.int8)
    for k in (range(len(cells)) if frames is None else frames):
        if k < len(cells) and cells[k] is not None:
            r, c = cells[k]
            occ[r.astype(np.int64) - m.rmin, c.astype(np.int64) - m.cmin] = 0
    known_r, known_c = np.nonzero((occ == 0).any(axis=1))[0], np.nonzero((occ == 0).any(axis=0))[0]
    rmin, rmax, cmin, cmax = known_r[0], known_r[-1], known_c[0], known_c[-1]     # IndexError: nothing is known
    occ = occ[rmin:rmax + 1, cmin:cmax + 1].copy()
    rmin, rmax, cmin, cmax = (int(v) for v in (rmin + m.rmin, rmax + m.rmin, cmin + m.cmin, cmax + m.cmin))
    selected = points
    if m.outlier_filter_min_points > 1:
        points = remove_outlier(np.asarray(points, np.float32), m.outlier_filter_radius, m.outlier_filter_min_points)
    x0 = np.float64(m.x0) + cmin * np.float64(m.resolution)
    y0 = np.float64(m.y0) + rmin * np.float64(m.resolution)
    r = np.rint((points[:, 1].astype(np.float64) - y0) / np.float64(m.resolution))
    c = np.rint((points[:, 0].astype(np.float64) - x0) / np.float64(m.resolution))
    inside = (r >= 0) & (r < occ.shape[0]) & (c >= 0) & (c < occ.shape[1])
    mask = np.zeros(occ.shape, bool)
    mask[r[inside].astype(np.int64), c[inside].astype(np.int64)] = True
    occ[dilate(mask, ellipse_element(m.dilate_size))] = 100
    out_res = float(m.resolution)
    if resolution is not None and resolution > 0 and abs(resolution - m.resolution) > m.resolution * 1e-1:
        ratio = m.resolution / resolution
        occ = resize_nearest(occ, ratio)
        out_res = m.resolution / ratio
    return dict(data=occ, info=(float(x0), float(y0), occ.shape[1], occ.shape[0], out_res), box=(rmin, rmax, cmin, cmax),
                points=np.asarray(selected), kept=len(points))
