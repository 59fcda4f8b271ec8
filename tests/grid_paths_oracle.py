"""numpy restatement of the distances of the reference's GridGraph (shortest_paths.pyx:26-114), used by the grid-path tests.

The graph: 8-connected, an edge joins two free cells (grid != 0) inside the grid, straight edges weigh 1 and diagonal ones
float32(sqrt 2).  SPFA accepts fl32(d[u] + w) only when strictly smaller; any sequence of such updates that ends when no edge improves
any label reaches the same labels (per cell, the least left-to-right fp32 sum over paths), so a synchronous (Jacobi) relaxation of all
eight directions, repeated until nothing changes, is an exact oracle.  The source holds 0 even when blocked; cells still at
inf = 2 * rows * cols become -1 (the `>= inf - 1e-6` test of the reference).
"""
import numpy as np

SQRT2 = np.float32(np.sqrt(2))                     # 0x3FB504F3, the `cdef float sqrt_2` of the reference
DIRS = [(0, -1, np.float32(1)), (0, 1, np.float32(1)), (-1, -1, SQRT2), (-1, 0, np.float32(1)), (-1, 1, SQRT2),
        (1, -1, SQRT2), (1, 0, np.float32(1)), (1, 1, SQRT2)]


def distance_image(grid, source):
    """float32 [rows, cols] distances from `source` (i, j); -1 where unreachable."""
    grid = np.asarray(grid)
    R, C = grid.shape
    inf = np.float32(2 * R * C)
    free = np.zeros((R + 2, C + 2), bool)
    free[1:-1, 1:-1] = grid != 0
    d = np.full((R + 2, C + 2), inf, np.float32)
    d[1 + source[0], 1 + source[1]] = 0
    here = free[1:-1, 1:-1]
    # per direction: the cells whose neighbour in that direction is free as well (the edge exists)
    edges = [(di, dj, w, here & free[1 + di:1 + di + R, 1 + dj:1 + dj + C]) for di, dj, w in DIRS]
    for _ in range(R * C + 1):
        cur = d[1:-1, 1:-1]
        new = cur.copy()
        for di, dj, w, ok in edges:
            cand = d[1 + di:1 + di + R, 1 + dj:1 + dj + C] + w           # fp32 + fp32: one rounding
            better = ok & (cand < new)
            new[better] = cand[better]
        if np.array_equal(new, cur):
            break
        d[1:-1, 1:-1] = new
    else:
        raise AssertionError('no fixed point after rows * cols + 1 sweeps')
    out = d[1:-1, 1:-1].copy()
    out[out.astype(np.float64) >= float(inf) - 1e-6] = -1
    return out


def mapper_image(dist, pixels_per_meter, scale):
    """Mapper._create_global_shortest_path_map (envs.py:2294-2299) after OccupancyMap.shortest_path_image (envs.py:2513-2516):
    float32 division, negatives -> the image max, float32 multiply."""
    img = dist / np.float32(pixels_per_meter)
    img[img < 0] = img.max()
    img *= np.float32(scale)
    return img
