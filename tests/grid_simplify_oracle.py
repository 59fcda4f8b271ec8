"""The exact simplification rule of include/simq.h (simq_grid_waypoints) in Python integers, written from the rule's text and not
from simq.approximate_polygon_exact: one point at a time, every squared distance a fraction (numerator, denominator) compared by
cross-multiplication, the segments on the stack of the published algorithm.  `simplify_exact` can record the ties it meets: a largest
distance equal to the tolerance, and a split whose largest distance is attained more than once.

`approximate_polygon_float` restates the published Douglas-Peucker of skimage.measure.approximate_polygon (float64 arctan2 / sin /
cos) with an `eps` switch: values within eps count as equal -- a segment is split iff its largest distance exceeds tolerance + eps,
at the first point within eps of the largest.  eps = 0 is the published algorithm as it stands.

`waypoints` is the pruning of shortest_paths.pyx:142-149 behind the exact rule; `random_walks` the seeded lattice walks of the tests.
"""
import functools

import numpy as np

from intention_maps_oracle import line_points

DIRS = ((0, -1), (0, 1), (-1, -1), (-1, 0), (-1, 1), (1, -1), (1, 0), (1, 1))


def simplify_exact(coords, tolerance, ties=None):
    """coords[kept] by the rule; ties: a dict whose 'tolerance' and 'argmax' counters are raised."""
    pts = [(int(p[0]), int(p[1])) for p in coords]
    n, t2 = len(pts), int(tolerance) ** 2
    keep = [False] * n
    keep[0] = keep[n - 1] = True
    stack = [(0, n - 1)]
    while stack:
        s, e = stack.pop()
        if e <= s + 1:
            continue
        (rs, cs), (re, ce) = pts[s], pts[e]
        dr, dc = re - rs, ce - cs
        L = dr * dr + dc * dc
        best, first, attained = None, -1, 0
        for k in range(s + 1, e):
            rk, ck = pts[k]
            a0 = (rk - rs) * dr + (ck - cs) * dc
            a1 = -(rk - re) * dr - (ck - ce) * dc
            if a0 > 0 and a1 > 0:
                d = (((rk - rs) * dc - (ck - cs) * dr) ** 2, L)
            else:
                d = (min((rk - rs) ** 2 + (ck - cs) ** 2, (rk - re) ** 2 + (ck - ce) ** 2), 1)
            if best is None or d[0] * best[1] > best[0] * d[1]:
                best, first, attained = d, k, 1
            elif d[0] * best[1] == best[0] * d[1]:
                attained += 1
        if ties is not None and best[0] == t2 * best[1]:
            ties['tolerance'] += 1
        if best[0] > t2 * best[1]:
            if ties is not None and attained > 1:
                ties['argmax'] += 1
            keep[first] = True
            stack.append((first, e))
            stack.append((s, first))
    return np.asarray(coords)[np.asarray(keep)]


def approximate_polygon_float(coords, tolerance, eps=0.0):
    """The published algorithm in float64; eps > 0 makes values within eps count as equal."""
    coords = np.asarray(coords)
    n = coords.shape[0]
    chain = np.zeros(n, bool)
    chain[0] = chain[n - 1] = True
    stack = [(0, n - 1)]
    while stack:
        start, end = stack.pop()
        if end <= start + 1:
            continue
        r0, c0 = (float(x) for x in coords[start])
        r1, c1 = (float(x) for x in coords[end])
        dr, dc = r1 - r0, c1 - c0
        angle = -np.arctan2(dr, dc)
        offset = c0 * np.sin(angle) + r0 * np.cos(angle)
        seg = coords[start + 1:end].astype(np.float64)
        dr0, dc0, dr1, dc1 = seg[:, 0] - r0, seg[:, 1] - c0, seg[:, 0] - r1, seg[:, 1] - c1
        perp = np.logical_and(dr0 * dr + dc0 * dc > 0, -dr1 * dr - dc1 * dc > 0)
        dists = np.minimum(np.sqrt(dc0 ** 2 + dr0 ** 2), np.sqrt(dc1 ** 2 + dr1 ** 2))
        dists[perp] = np.abs(seg[perp, 0] * np.cos(angle) + seg[perp, 1] * np.sin(angle) - offset)
        m = dists.max()
        if m > tolerance + eps:
            new = start + 1 + (int(np.argmax(dists)) if eps == 0.0 else int(np.flatnonzero(dists >= m - eps)[0]))
            stack.append((new, end))
            stack.append((start, new))
            chain[new] = True
    return coords[chain]


def waypoints(grid, dense, tolerance=1):
    """GridGraph.shortest_path from the dense path on (shortest_paths.pyx:139-154) with the exact rule as its simplifier: int32
    [m, 2], source first."""
    sparse = exact(dense, tolerance)
    path = [sparse[0]]
    for k in range(1, len(sparse) - 1):
        rr, cc = line_points(*[int(x) for x in path[-1]], *[int(x) for x in sparse[k + 1]])
        if (grid[rr, cc] != 1).any():
            path.append(sparse[k])
    if len(sparse) > 1:
        path.append(sparse[-1])
    return np.asarray(path[::-1], np.int32).reshape(-1, 2)


_SIMPLIFIED = {}


def exact(coords, tolerance):
    """simplify_exact with the signature of the simplify= callables; computed once per (path, tolerance) of a test session."""
    coords = np.asarray(coords)
    key = (coords.dtype.str, coords.shape, coords.tobytes(), int(tolerance))
    if key not in _SIMPLIFIED:
        _SIMPLIFIED[key] = simplify_exact(coords, tolerance)
        _SIMPLIFIED[key].setflags(write=False)
    return _SIMPLIFIED[key]


WALK_ORIGIN, WALK_EXTENT = 130, 260          # every walk stays inside a WALK_EXTENT x WALK_EXTENT grid


@functools.lru_cache(maxsize=None)
def random_walks(count=2000, seed=20250117):
    """`count` seeded 8-connected lattice walks of 3 .. 120 points from (130, 130), free to cross and repeat themselves; every second
    one holds each direction for 4 steps (long axis and diagonal runs).  A tuple of read-only int32 [n, 2] arrays."""
    rng = np.random.RandomState(seed)
    walks = []
    for w in range(count):
        n = int(rng.randint(3, 121))
        hold = 4 if w % 2 else 1
        pts, d = [(WALK_ORIGIN, WALK_ORIGIN)], DIRS[0]
        for k in range(n - 1):
            if k % hold == 0:
                d = DIRS[int(rng.randint(8))]
            pts.append((pts[-1][0] + d[0], pts[-1][1] + d[1]))
        a = np.asarray(pts, np.int32)
        a.setflags(write=False)
        walks.append(a)
    return tuple(walks)


def walk_grids():
    """The two grids of the walks: all ones (every line clear: pruning drops every interior waypoint), and seeded cells of 0, 1 and
    a few 2 (a cell that is free for the search and still not 1 for the line test)."""
    rng = np.random.RandomState(7)
    mixed = (rng.rand(WALK_EXTENT, WALK_EXTENT) < 0.9).astype(np.uint8)
    mixed[rng.rand(WALK_EXTENT, WALK_EXTENT) < 0.01] = 2
    return np.ones((WALK_EXTENT, WALK_EXTENT), np.uint8), mixed
