"""numpy restatement of the reference's shortest-path waypoints, written as the reference is: GridGraph._spfa with its queue and its
swap (shortest_paths.pyx:69-114), the walk over the parents and the pruning of GridGraph.shortest_path (:121-154), and
OccupancyMap.shortest_path around them (envs.py:2477-2504).  `spfa` also counts what decides whether a test input can tell a right
emulation from a wrong one: pops, pushes, swaps, relaxations of vertices that are already queued, and the order-sensitive pushes --
those whose swap comes out differently when it is decided against the front's distance as it stands after the pop's last edge
instead of at the pushing edge.
"""
import os

import numpy as np

from intention_maps_oracle import line_points, position_to_pixel_indices

DIRS = ((0, -1), (0, 1), (-1, -1), (-1, 0), (-1, 1), (1, -1), (1, 0), (1, 1))             # shortest_paths.pyx:30
SQRT_2 = np.float32(np.sqrt(2))
WEIGHTS = tuple(np.float32(w) for w in (1, 1, SQRT_2, 1, SQRT_2, SQRT_2, 1, SQRT_2))
PIXELS_PER_METER = 96


def spfa(grid, source):
    """(dists float32 [rows, cols] with -1 where unreachable, parents int32 [rows, cols] of ravelled indices with -1 where none,
    counters) of GridGraph(grid)._spfa(*source)."""
    rows, cols = grid.shape
    n = rows * cols
    free = (grid != 0).reshape(-1).tolist()
    inf = np.float32(2 * n)
    dists = [inf] * n
    parents = [-1] * n
    queue = [0] * (n * 8)
    in_queue = [0] * n
    count = dict(pops=0, pushes=0, swaps=0, order_sensitive=0, queued_relaxations=0)
    head, tail = 0, 0
    s = source[0] * cols + source[1]
    dists[s] = np.float32(0)
    tail += 1
    queue[tail] = s
    in_queue[s] = 1
    while head < tail:
        head += 1
        u = queue[head]
        in_queue[u] = 0
        count['pops'] += 1
        if not free[u]:
            continue                                                   # edges leave a free cell only
        ui, uj = divmod(u, cols)
        pushed = []                                                    # (front vertex at the push, pushed distance, swapped)
        for (di, dj), w in zip(DIRS, WEIGHTS):
            ip, jp = ui + di, uj + dj
            if ip < 0 or jp < 0 or ip >= rows or jp >= cols:
                continue
            v = ip * cols + jp
            if not free[v]:
                continue
            new_dist = np.float32(dists[u] + w)
            if new_dist < dists[v]:
                parents[v] = u
                dists[v] = new_dist
                if not in_queue[v]:
                    tail += 1
                    queue[tail] = v
                    in_queue[v] = 1
                    count['pushes'] += 1
                    front = queue[head + 1]
                    swapped = bool(dists[queue[tail]] < dists[front])
                    pushed.append((front, new_dist, swapped))
                    if swapped:
                        queue[tail], queue[head + 1] = queue[head + 1], queue[tail]
                        count['swaps'] += 1
                else:
                    count['queued_relaxations'] += 1
        # a push is order-sensitive when the front's distance after the pop's last edge decides its swap the other way: what
        # "all eight updates first, the pushes afterwards" would get wrong
        for front, nd, swapped in pushed:
            if bool(nd < dists[front]) != swapped:
                count['order_sensitive'] += 1
    d = np.asarray(dists, np.float32)
    d[d >= inf - 1e-6] = -1
    return d.reshape(rows, cols), np.asarray(parents, np.int32).reshape(rows, cols), count


def dense_path(parents, source, target):
    """The dense path of GridGraph.shortest_path (:126-137): int32 [n, 2], target first."""
    cols = parents.shape[1]
    flat = parents.reshape(-1)
    u = source[0] * cols + source[1]
    v = target[0] * cols + target[1]
    path = [[v // cols, v % cols]]
    while not v == u:
        v = int(flat[v])
        if v < 0:
            break
        path.append([v // cols, v % cols])
    return np.asarray(path, np.int32)


def identity(coords, tolerance):
    return coords


def every_third(coords, tolerance):
    """Stand-in simplifier of the fixtures: the first point, every third one after it, the last."""
    keep = sorted(set(range(0, len(coords), 3)) | {len(coords) - 1})
    return coords[keep]


def prune(grid, dense, simplify):
    """GridGraph.shortest_path from the dense path on (:139-154): simplify, drop the waypoints a clear line makes unnecessary, reverse."""
    sparse_path = simplify(np.array(dense), tolerance=1)
    path = [sparse_path[0]]
    for k in range(1, sparse_path.shape[0] - 1):
        rr, cc = line_points(*[int(x) for x in path[-1]], *[int(x) for x in sparse_path[k + 1]])
        if (1 - grid[rr, cc]).sum() > 0:
            path.append(sparse_path[k])
    if len(sparse_path) > 1:
        path.append(sparse_path[-1])
    return path[::-1]


def pixel_indices_to_position(pixel_i, pixel_j, image_shape):
    """envs.py:2399-2402."""
    position_x = ((pixel_j + 0.5) - image_shape[1] / 2) / PIXELS_PER_METER
    position_y = (image_shape[0] / 2 - (pixel_i + 0.5)) / PIXELS_PER_METER
    return position_x, position_y


def is_straight(cspace_thin, source_pixel, target_pixel):
    rr, cc = line_points(*source_pixel, *target_pixel)
    return bool((1 - cspace_thin[rr, cc]).sum() == 0)


def occupancy_shortest_path(cspace, cspace_thin, closest, source_position, target_position, simplify, cache=None):
    """OccupancyMap.shortest_path (envs.py:2477-2504); `cache`: {source pixel: parents} shared between calls on one map."""
    shape = cspace.shape
    source = position_to_pixel_indices(source_position[0], source_position[1], shape)
    target = position_to_pixel_indices(target_position[0], target_position[1], shape)
    if is_straight(cspace_thin, source, target):
        return [source_position, target_position]
    source = (int(closest[0][source]), int(closest[1][source]))
    target = (int(closest[0][target]), int(closest[1][target]))
    cache = {} if cache is None else cache
    if source not in cache:
        cache[source] = spfa(cspace, source)[1]
    path_pixel_indices = prune(cspace, dense_path(cache[source], source, target), simplify)
    path = []
    for i, j in path_pixel_indices:
        position_x, position_y = pixel_indices_to_position(i, j, shape)
        path.append((position_x, position_y, 0))
    if len(path) < 2:
        path = [source_position, target_position]
    else:
        path[0] = source_position
        path[-1] = target_position
    return path


def random_grids():
    """The 60 seeded grids of the GPU test: 8 x 8 to 60 x 70, 10-35 % of the cells blocked at random plus a few blocked rectangles;
    returns [(grid, source, target)]."""
    rng = np.random.RandomState(20240613)
    cases = []
    for _ in range(60):
        rows, cols = int(rng.randint(8, 61)), int(rng.randint(8, 71))
        grid = (rng.rand(rows, cols) >= rng.uniform(0.10, 0.35)).astype(np.uint8)
        for _ in range(rng.randint(0, 4)):
            i, j = rng.randint(rows), rng.randint(cols)
            grid[i:i + rng.randint(1, 6), j:j + rng.randint(1, 12)] = 0
        ii, jj = np.nonzero(grid)
        a, b = rng.randint(ii.size, size=2)
        cases.append((grid, (int(ii[a]), int(jj[a])), (int(ii[b]), int(jj[b]))))
    return cases


def free_box(grid):
    """(i0, j0, rows, cols) of the bounding box of the free cells, (0, 0, 0, 0) when there is none."""
    ii, jj = np.nonzero(grid)
    if ii.size == 0:
        return 0, 0, 0, 0
    return int(ii.min()), int(jj.min()), int(ii.max() - ii.min() + 1), int(jj.max() - jj.min() + 1)


def occupancy_problems(golden_dir, room, per_kind=18):
    """(cspace, thin, closest, [(map, source position, target position)]) over the maps of an occupancy fixture that have free cells:
    seeded pose pairs, drawn until `per_kind` of them are straight by the reference's test and `per_kind` are not, interleaved."""
    z = np.load(os.path.join(golden_dir, 'occupancy_maps_%s.npz' % room))
    cspace, thin, closest = z['configuration_space'], z['cspace_thin'], z['closest']
    usable = [m for m in range(len(cspace)) if cspace[m].any()]
    shape = cspace.shape[1:]
    half_x, half_y = shape[1] / 2 / PIXELS_PER_METER, shape[0] / 2 / PIXELS_PER_METER
    rng = np.random.RandomState(5 + shape[1])
    kinds = {True: [], False: []}
    for k in range(20000):
        if min(len(v) for v in kinds.values()) >= per_kind:
            break
        m = usable[k % len(usable)]
        a = (float(rng.uniform(-half_x, half_x)), float(rng.uniform(-half_y, half_y)), float(rng.uniform(-3, 3)))
        b = (float(rng.uniform(-half_x, half_x)), float(rng.uniform(-half_y, half_y)), 0.0)
        straight = is_straight(thin[m], position_to_pixel_indices(a[0], a[1], shape), position_to_pixel_indices(b[0], b[1], shape))
        if len(kinds[straight]) < per_kind:
            kinds[straight].append((m, a, b))
    assert min(len(v) for v in kinds.values()) >= per_kind
    return cspace, thin, closest, [q for pair in zip(kinds[True], kinds[False]) for q in pair]
