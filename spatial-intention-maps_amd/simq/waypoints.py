"""Shortest-path waypoints on the GPU: the navigation half of the reference's ``shortest_paths.GridGraph``.

``GridGraph.shortest_path`` (shortest_paths.pyx:121-154) walks the parents its SPFA recorded from the target back to the source,
simplifies that dense path with ``skimage.measure.approximate_polygon`` and drops the waypoints a clear line makes unnecessary;
``OccupancyMap.shortest_path`` (envs.py:2477-2504) puts a straight-line test and the snap to the closest free cells in front and the
conversion to positions behind.  SPFA's parents depend on the order of its queue, so ``simq_grid_paths`` (csrc/grid_waypoints.hip)
emulates the search itself, one problem per wavefront, and returns parents, distances and dense paths that equal the reference's bit
for bit.  The default simplification stays on the host: it is float64 trigonometry whose ties are libm noise.
simplify='exact' is the same algorithm with every comparison decided in integers (the rule of include/simq.h): on the host
approximate_polygon_exact, on the device ``simq_grid_waypoints`` (csrc/grid_simplify.hip), which simplifies and prunes the dense paths
where the search left them, so that only the waypoints come back.  The search keeps its state in LDS, which bounds the box of a
grid's free cells; large_windows=True sends the problems over that bound to ``simq_grid_paths_large``, the same search with its state in
a workspace in device memory.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _batch
from ._lib import SimqError, lib, ptr, stream_ptr
from .grid_paths import GridGraph, index_grids, pixel
from .local_maps import PIXELS_PER_METER, position_to_pixel_indices

MAX_BOX_CELLS = 20000            # SIMQ_GRID_PATH_MAX_BOX_CELLS of include/simq.h
TRACED, STRAIGHT, BAD_DESCRIPTOR, CAPACITY = 0, 1, 2, 3


class GridPathProblem(ctypes.Structure):
    """simq_grid_path_problem of include/simq.h."""
    _fields_ = [(n, ctypes.c_int64) for n in ('grid_offset', 'thin_offset', 'closest_offset', 'path_offset', 'parents_offset',
                                              'dist_offset')] + \
               [(n, ctypes.c_int32) for n in ('path_capacity', 'rows', 'cols', 'src_i', 'src_j', 'tgt_i', 'tgt_j', 'box_i0', 'box_j0',
                                              'box_rows', 'box_cols', 'reserved_')]


class GridPathLargeProblem(ctypes.Structure):
    """simq_grid_path_large_problem of include/simq.h: GridPathProblem's fields plus work_offset."""
    _fields_ = [(n, ctypes.c_int64) for n in ('grid_offset', 'thin_offset', 'closest_offset', 'path_offset', 'parents_offset',
                                              'dist_offset', 'work_offset')] + GridPathProblem._fields_[6:]


def large_work_bytes(box_rows, box_cols):
    """simq_grid_paths_large_work_bytes of include/simq.h restated: fp32 distances, one-byte parents and flags over the window plus
    its halo, a ring of window cells + 1 32-bit entries, rounded up to 16."""
    cells = (box_rows + 2) * (box_cols + 2)
    return (6 * cells + 4 * (box_rows * box_cols + 1) + 15) // 16 * 16


def split_by_window(boxes):
    """(fit, over): the problems whose window (i0, j0, rows, cols) plus its halo has at most MAX_BOX_CELLS cells -- simq_grid_paths
    takes them, its search state in LDS -- and the others, for simq_grid_paths_large; both ascending."""
    fit = [p for p, b in enumerate(boxes) if (b[2] + 2) * (b[3] + 2) <= MAX_BOX_CELLS]
    over = [p for p, b in enumerate(boxes) if (b[2] + 2) * (b[3] + 2) > MAX_BOX_CELLS]
    return fit, over


def entry_calls(n_fit, n):
    """The entry points a call over n problems makes when the first n_fit fit the LDS cap: [(name, first, last + 1)], an empty part
    left out."""
    return [c for c in (('simq_grid_paths', 0, n_fit), ('simq_grid_paths_large', n_fit, n)) if c[2] > c[1]]


def restore_order(order, items):
    """items[k] belongs to problem order[k]: the list in problem order."""
    out = [None] * len(order)
    for k, p in enumerate(order):
        out[p] = items[k]
    return out


def _check_large_windows(large_windows):
    if not isinstance(large_windows, bool):
        raise ValueError('large_windows must be True or False, got %r' % (large_windows,))
    return large_windows


def _window_order(descs, large_windows):
    """(order, n_fit): the problems in the order they are launched -- with large_windows those over the LDS cap behind the others,
    descs[order[n_fit:]] for simq_grid_paths_large; without it all as they come, for simq_grid_paths to take or refuse."""
    if not large_windows:
        return list(range(len(descs))), len(descs)
    fit, over = split_by_window([d['box'] for d in descs])
    return fit + over, len(fit)


class GridWaypointProblem(ctypes.Structure):
    """simq_grid_waypoint_problem of include/simq.h."""
    _fields_ = [(n, ctypes.c_int64) for n in ('grid_offset', 'path_offset', 'way_offset')] + \
               [(n, ctypes.c_int32) for n in ('rows', 'cols', 'way_capacity', 'tolerance')]


DensePaths = collections.namedtuple('DensePaths', 'paths status endpoints parents distances')
Waypoints = collections.namedtuple('Waypoints', 'waypoints status endpoints')
WAY_CAPACITY = 64                # pairs per problem in the first read-back; a longer list is fetched with the second


def line(r0, c0, r1, c1):
    """skimage.draw.line in closed form (the rule of simq_intention_maps, include/simq.h): with n = max(|dr|, |dc|) and m = min(|dr|,
    |dc|), point i is i steps along the major axis and (2 * m * i + n) // (2 * n) along the minor one."""
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sr, sc = (1 if r1 > r0 else -1), (1 if c1 > c0 else -1)
    n, m = max(dr, dc), min(dr, dc)
    i = np.arange(n + 1, dtype=np.int64)
    minor = (2 * m * i + n) // (2 * n) if n > 0 else np.zeros(1, np.int64)
    if dr > dc:
        return r0 + sr * i, c0 + sc * minor
    return r0 + sr * minor, c0 + sc * i


def pixel_indices_to_position(pixel_i, pixel_j, image_shape):
    """Mapper.pixel_indices_to_position (envs.py:2399-2402)."""
    position_x = ((pixel_j + 0.5) - image_shape[1] / 2) / PIXELS_PER_METER
    position_y = (image_shape[0] / 2 - (pixel_i + 0.5)) / PIXELS_PER_METER
    return position_x, position_y


def _default_simplify():
    try:
        from skimage.measure import approximate_polygon      # pylint: disable=import-outside-toplevel
    except ImportError:
        raise SimqError('shortest_path simplifies the dense path with skimage.measure.approximate_polygon and scikit-image is not '
                        "installed: install it, pass simplify='exact' (the same algorithm decided in integers, no dependency) or pass "
                        'simplify=callable(coords, tolerance) (dense_path needs neither)') from None
    return approximate_polygon


def approximate_polygon_exact(coords, tolerance):
    """skimage.measure.approximate_polygon on integer pixels with every comparison decided exactly (the rule of include/simq.h): a
    segment (s, e) is split at the first interior point of largest distance iff that distance exceeds the tolerance, distances being
    squared and kept as fractions over the segment's squared length.  coords: integer [n, 2], n >= 1; tolerance: an integer in
    [1, 255].  Returns coords[kept].  Integer arithmetic throughout: int64 while the coordinates span less than 2^15, Python integers
    beyond.  The kept set is that of simq_grid_waypoints before its pruning."""
    coords = np.asarray(coords)
    if coords.ndim != 2 or coords.shape[1] != 2 or coords.shape[0] < 1 or coords.dtype.kind not in 'iu':
        raise ValueError('approximate_polygon_exact takes an integer [n, 2] array with n >= 1, got %s %s' % (coords.dtype, coords.shape))
    if isinstance(tolerance, bool) or int(tolerance) != tolerance or not 1 <= int(tolerance) <= 255:
        raise ValueError('approximate_polygon_exact takes an integer tolerance in [1, 255], got %r' % (tolerance,))
    n, t2 = coords.shape[0], int(tolerance) ** 2
    wide = int(coords.max()) - int(coords.min()) >= 1 << 15
    pts = coords.astype(object) if wide else coords.astype(np.int64)
    r, c = pts[:, 0], pts[:, 1]
    keep = np.zeros(n, bool)
    keep[0] = keep[n - 1] = True
    stack = [(0, n - 1)]
    while stack:
        s, e = stack.pop()
        if e <= s + 1:
            continue
        dr, dc = r[e] - r[s], c[e] - c[s]
        L = dr * dr + dc * dc
        r0, c0, r1, c1 = r[s + 1:e] - r[s], c[s + 1:e] - c[s], r[s + 1:e] - r[e], c[s + 1:e] - c[e]
        perp = (r0 * dr + c0 * dc > 0) & (-r1 * dr - c1 * dc > 0)
        cross, e0, e1 = r0 * dc - c0 * dr, r0 * r0 + c0 * c0, r1 * r1 + c1 * c1
        scale = L if L else 1                                  # both ends on one pixel: no distance is perpendicular
        v = np.where(perp, cross * cross, np.where(e1 < e0, e1, e0) * scale)          # every distance over the one denominator
        m = v.max()
        if m > t2 * scale:
            k = s + 1 + int(np.flatnonzero(v == m)[0])
            keep[k] = True
            stack.append((k, e))
            stack.append((s, k))
    return coords[keep]


def _simplifier(simplify):
    """The callable behind a simplify= argument: None -> scikit-image, 'exact' -> approximate_polygon_exact, a callable -> itself."""
    if simplify is None:
        return _default_simplify()
    if isinstance(simplify, str):
        if simplify != 'exact':
            raise ValueError("simplify=%r: the only named simplifier is 'exact' (None: skimage.measure.approximate_polygon, or a "
                             'callable(coords, tolerance))' % simplify)
        return approximate_polygon_exact
    return simplify


def walk(parents, source, target):
    """The dense path of shortest_paths.pyx:126-137 over a host parent image: int32 [n, 2], target first."""
    cols = parents.shape[1]
    flat = parents.reshape(-1)
    u = source[0] * cols + source[1]
    v = target[0] * cols + target[1]
    path = [(v // cols, v % cols)]
    while v != u:
        v = int(flat[v])
        if v < 0:
            break
        path.append((v // cols, v % cols))
    return np.asarray(path, np.int32)


def prune(grid, dense, simplify):
    """shortest_paths.pyx:139-154 on a host grid: simplify(dense, tolerance=1), keep a waypoint only where the line from the last kept
    one to its successor crosses a cell that is not 1 (the reference's uint8 `1 - grid`), reverse.  Returns [(i, j)] source first."""
    sparse = np.asarray(simplify(np.array(dense), tolerance=1))
    path = [sparse[0]]
    for k in range(1, sparse.shape[0] - 1):
        rr, cc = line(int(path[-1][0]), int(path[-1][1]), int(sparse[k + 1][0]), int(sparse[k + 1][1]))
        if (1 - grid[rr, cc]).sum() > 0:
            path.append(sparse[k])
    if len(sparse) > 1:
        path.append(sparse[-1])
    return [(int(q[0]), int(q[1])) for q in path[::-1]]


def _check_closest(c, what):
    ok = isinstance(c, (np.ndarray, torch.Tensor)) and c.ndim == 3 and c.shape[0] == 2 and \
        (c.dtype == torch.int32 and c.is_contiguous() if isinstance(c, torch.Tensor) else c.dtype == np.int32 and c.flags['C_CONTIGUOUS'])
    if not ok:
        raise ValueError('%s must be a contiguous int32 [2, rows, cols] array or tensor (closest_cspace_indices)' % what)
    return c


def _boxes(grids, used, dev):
    """{k: (i0, j0, rows, cols)}: the bounding box of the free cells of each used grid; device grids are reduced there and the boxes
    of all of them downloaded at once."""
    boxes, rows_on_dev, keys = {}, [], []
    for k in used:
        g = grids[k]
        if isinstance(g, torch.Tensor) and g.device.type == 'cuda':
            R, C = g.shape
            ri, ci = torch.arange(R, device=g.device), torch.arange(C, device=g.device)
            fr, fc = (g != 0).any(1), (g != 0).any(0)
            rows_on_dev.append(torch.stack([torch.where(fr, ri, R).min(), torch.where(fr, ri, -1).max(),
                                            torch.where(fc, ci, C).min(), torch.where(fc, ci, -1).max()]))
            keys.append(k)
        else:
            g = g.numpy() if isinstance(g, torch.Tensor) else g
            ii, jj = np.nonzero(g)
            boxes[k] = (0, 0, 0, 0) if ii.size == 0 else (int(ii.min()), int(jj.min()), int(ii.max() - ii.min() + 1),
                                                         int(jj.max() - jj.min() + 1))
    if keys:
        for k, (i0, i1, j0, j1) in zip(keys, torch.stack(rows_on_dev).cpu().tolist()):
            boxes[k] = (0, 0, 0, 0) if i1 < 0 else (i0, j0, i1 - i0 + 1, j1 - j0 + 1)
    return boxes


def _launch(dev, packed, closest_buf, descs, parents, distances, n_fit=None):
    """The search over `descs` (_enqueue) and the read-back of its lengths, status words and end pixels."""
    P = len(descs)
    small = torch.empty((P, 6), dtype=torch.int32, device=dev)          # lengths | status | end pixels
    paths, par, dist = _enqueue(dev, packed, closest_buf, descs, parents, distances, small.view(-1), n_fit)
    host = small.cpu().numpy().reshape(-1)
    return paths, host[:P].copy(), host[P:2 * P].copy(), host[2 * P:].reshape(P, 4).copy(), par, dist


def _enqueue(dev, packed, closest_buf, descs, parents, distances, small, n_fit=None):
    """Queues the search over `descs`: dicts with the descriptor's grid / thin / closest offsets, shape, pixels, box and capacity.  The
    first n_fit of them (all when None) go to simq_grid_paths, the others to simq_grid_paths_large with a workspace allocated here;
    both calls write the same buffers, each its own problems' ranges.  small: int32 device tensor whose first 6 P entries receive
    lengths | status | end pixels.  Nothing is read back."""
    P = len(descs)
    n_fit = P if n_fit is None else n_fit
    po = io = 0
    fields = []
    for d in descs:
        fields.append(([d['grid'], d['thin'], d['closest'], po, io if parents else -1, io if distances else -1],
                       [d['capacity'], d['rows'], d['cols'], d['src'][0], d['src'][1], d['tgt'][0], d['tgt'][1], *d['box'], 0]))
        po += d['capacity']
        io += d['rows'] * d['cols']
    paths = torch.empty((po, 2), dtype=torch.int32, device=dev)
    lengths, status, ends = small[:P], small[P:2 * P], small[2 * P:6 * P]
    par = torch.empty(io, dtype=torch.int32, device=dev) if parents else None
    dist = torch.empty(io, dtype=torch.float32, device=dev) if distances else None
    for name, a, b in entry_calls(n_fit, P):
        extra = ()
        if name == 'simq_grid_paths':
            probs = (GridPathProblem * (b - a))(*[GridPathProblem(*offsets, *ints) for offsets, ints in fields[a:b]])
        else:
            need = [large_work_bytes(d['box'][2], d['box'][3]) for d in descs[a:b]]
            at = np.concatenate([[0], np.cumsum(need)]).tolist()
            probs = (GridPathLargeProblem * (b - a))(*[GridPathLargeProblem(*offsets, at[k], *ints)
                                                       for k, (offsets, ints) in enumerate(fields[a:b])])
            work = torch.empty(at[-1], dtype=torch.uint8, device=dev)
            extra = (ptr(work), ctypes.c_int64(at[-1]))
        d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
        lib.call(name, ptr(packed), ctypes.c_int64(packed.numel()), ptr(closest_buf),
                 ctypes.c_int64(0 if closest_buf is None else closest_buf.numel()), probs, b - a, ptr(d_probs), ptr(paths), ctypes.c_int64(po),
                 ptr(lengths[a:b]), ptr(ends[4 * a:4 * b]), ptr(par), ctypes.c_int64(io), ptr(dist), ctypes.c_int64(io), ptr(status[a:b]),
                 *extra, stream_ptr(dev))
    return paths, par, dist


def grid_dense_paths(grids, sources, targets, grid_index=None, parents=False, distances=False, thin=None, closest=None,
                     large_windows=False):
    """The dense paths of P (grid, source, target) problems in one launch: SPFA from the source, then the walk over its parents from
    the target (shortest_paths.pyx:69-137), bit for bit.

    grids, grid_index: as grid_distance_images (2-D uint8 numpy arrays or device tensors, or one [G, rows, cols] array / tensor; free
    where nonzero; problem p uses grids[grid_index[p]], grid p when omitted).  sources, targets: P pixels (i, j) each.  thin, closest:
    the front half of OccupancyMap.shortest_path (envs.py:2483-2489), one entry per grid: with thin[k] (uint8, cspace_thin) a problem
    whose skimage.draw.line from source to target crosses only cells equal to 1 ends as STRAIGHT without a search; with closest[k]
    (int32 [2, rows, cols], closest_cspace_indices) source and target are replaced by closest[:, i, j] before the search (the line is
    tested on the pixels as given).

    Returns DensePaths(paths, status, endpoints, parents, distances): paths, a list of P int32 numpy arrays [n, 2], target first (n = 1,
    the target alone, for an unreachable target, a blocked source and target == source; n = 0 for a STRAIGHT problem); status, int32
    numpy [P] of TRACED / STRAIGHT; endpoints, int32 numpy [P, 4], the (source, target) pixels the search used; parents (when asked),
    a list of P int32 device tensors [rows, cols] holding the ravelled index of each cell's parent, -1 where none; distances (when
    asked), P float32 device tensors [rows, cols], -1 where unreachable.  The images of a STRAIGHT problem are not written.

    The search state lives in LDS over the bounding box of the grid's free cells: a box of more than MAX_BOX_CELLS cells with its
    one-cell halo is refused (SimqError, nothing launched) unless large_windows is True.  Then the problems over the cap go to
    simq_grid_paths_large, whose state lies in a workspace in device memory allocated here (10 bytes a cell of the box), the others
    to simq_grid_paths as before, both queued before the one read-back; the results are the same and come in problem order, and a
    search over the cap costs a few times what one in LDS costs per cell.  A path longer than the first buffer is fetched with one
    more launch."""
    _check_large_windows(large_windows)
    dev, packed, closest_buf, descs = _prepare(grids, sources, targets, grid_index, thin, closest)
    order, n_fit = _window_order(descs, large_windows)   # (the launches, and everything up to the return, in this order)
    descs = [descs[p] for p in order]
    paths, lengths, status, ends, par, dist = _launch(dev, packed, closest_buf, descs, parents, distances, n_fit)
    _raise_for(status)
    starts = np.concatenate([[0], np.cumsum([d['capacity'] for d in descs])])
    host = paths.cpu().numpy()
    out = [host[starts[p]:starts[p] + min(lengths[p], descs[p]['capacity'])].copy() for p in range(len(descs))]
    short = np.flatnonzero(status == CAPACITY)
    if short.size:                                       # a longer buffer for those problems, once; no image is written again
        paths2, lengths2, status2, _, _, _ = _launch(dev, packed, None, _again(descs, short, lengths, ends), False, False,
                                                     int((short < n_fit).sum()))
        _raise_for(status2, allow_capacity=False)
        host2, o = paths2.cpu().numpy(), 0
        for p, n in zip(short, lengths2):
            out[p] = host2[o:o + n].copy()
            o += int(lengths[p])
            status[p] = TRACED
    shapes = [(d['rows'], d['cols']) for d in descs]
    images = [None if flat is None else restore_order(order, _batch.views(flat, shapes)) for flat in (par, dist)]
    back = np.argsort(order)
    return DensePaths(restore_order(order, out), status[back], ends[back], *images)


def _again(descs, problems, lengths, ends):
    """The descriptors of `problems` for a second search whose path buffer holds the whole dense path: the pixels the first search
    used, no straight-line test, no snap."""
    return [dict(descs[p], capacity=int(lengths[p]), thin=-1, closest=-1, src=tuple(int(x) for x in ends[p, :2]),
                 tgt=tuple(int(x) for x in ends[p, 2:])) for p in problems]


def _prepare(grids, sources, targets, grid_index, thin, closest):
    """What grid_dense_paths and grid_waypoints share: arguments checked, the used grids (then their thin maps) and closest cells packed
    on the device, one descriptor dict per problem.  Returns (device, packed uint8 buffer, closest buffer or None, descriptors)."""
    grids, _ = _batch.as_maps(grids, 'grids')
    srcs, tgts = [pixel(s) for s in sources], [pixel(t) for t in targets]
    if not grids or not srcs:
        raise ValueError('grid_dense_paths needs at least one grid and one source')
    if len(srcs) != len(tgts):
        raise ValueError('%d sources but %d targets' % (len(srcs), len(tgts)))
    grid_index = index_grids(grid_index, len(grids), len(srcs))
    if thin is not None:
        thin, _ = _batch.as_maps(thin, 'thin')
    if closest is not None:
        closest, _ = _batch.as_maps(closest, 'closest', _check_closest)
    used = sorted(set(grid_index))
    for name, extra in (('thin', thin), ('closest', closest)):
        if extra is not None:
            if len(extra) != len(grids):
                raise ValueError('%s must hold one map per grid (%d), got %d' % (name, len(grids), len(extra)))
            for k in used:
                if tuple(extra[k].shape[-2:]) != tuple(grids[k].shape):
                    raise ValueError('%s[%d] is %s but grids[%d] is %s' % (name, k, tuple(extra[k].shape), k, tuple(grids[k].shape)))
    dev = _batch.device('grid distance images')

    # the grids the problems use, then their thin maps, in one uint8 buffer; offsets kept multiples of 16 elements (the kernel reads a
    # grid 16 bytes at a time where it is aligned)
    packed, offsets = _batch.pack([grids[k] for k in used] + ([thin[k] for k in used] if thin is not None else []), torch.uint8, dev, align=16)
    goff, toff = dict(zip(used, offsets)), dict(zip(used, offsets[len(used):]))
    closest_buf, coff = None, {}
    if closest is not None:
        closest_buf, offsets = _batch.pack([closest[k] for k in used], torch.int32, dev, align=16)
        coff = dict(zip(used, offsets))
    boxes = _boxes(grids, used, dev)
    descs = []
    for k, s, t in zip(grid_index, srcs, tgts):
        rows, cols = grids[k].shape
        box = boxes[k]
        descs.append(dict(grid=goff[k], thin=toff.get(k, -1), closest=coff.get(k, -1), rows=rows, cols=cols, src=s,
                          tgt=t, box=box, capacity=max(1, min(box[2] * box[3], 2 * (box[2] + box[3]) + 8))))
    return dev, packed, closest_buf, descs


def _enqueue_waypoints(dev, packed, paths, descs, capacities, tolerance, small, base):
    """Queues one simq_grid_waypoints call behind the search that filled `paths` and small[:6 P]: its status words, counts and
    waypoints go to small[base:], problem p's waypoints at pair sum(capacities[:p]).  Nothing is read back."""
    P = len(descs)
    probs = (GridWaypointProblem * P)()
    po = wo = 0
    for p, d in enumerate(descs):
        probs[p] = GridWaypointProblem(d['grid'], po, wo, d['rows'], d['cols'], capacities[p], tolerance)
        po += d['capacity']
        wo += capacities[p]
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    lib.call('simq_grid_waypoints', ptr(packed), ctypes.c_int64(packed.numel()), ptr(paths), ctypes.c_int64(po), ptr(small[:P]),
             ptr(small[P:2 * P]), probs, P, ptr(d_probs), ptr(small[base + 2 * P:]), ctypes.c_int64(wo), ptr(small[base + P:base + 2 * P]),
             ptr(small[base:base + P]), stream_ptr(dev))


def _search_and_simplify(dev, packed, closest_buf, descs, capacities, tolerance, n_fit=None):
    """The search (_enqueue: simq_grid_paths, simq_grid_paths_large or both) and simq_grid_waypoints back to back on the same device buffers and the one read-back of both: (lengths, path
    status, end pixels [P, 4], waypoint status, counts, the waypoint buffer [pairs, 2]) as host arrays."""
    P = len(descs)
    base = 6 * P + (6 * P) % 2                           # the waypoints start on an 8-byte boundary
    small = torch.empty(base + 2 * P + 2 * sum(capacities), dtype=torch.int32, device=dev)
    paths, _, _ = _enqueue(dev, packed, closest_buf, descs, False, False, small, n_fit)
    _enqueue_waypoints(dev, packed, paths, descs, capacities, tolerance, small, base)
    host = small.cpu().numpy()
    return (host[:P], host[P:2 * P], host[2 * P:6 * P].reshape(P, 4), host[base:base + P], host[base + P:base + 2 * P],
            host[base + 2 * P:].reshape(-1, 2))


def grid_waypoints(grids, sources, targets, grid_index=None, thin=None, closest=None, tolerance=1, large_windows=False):
    """The waypoints of P (grid, source, target) problems without a dense path on the host: simq_grid_paths as in grid_dense_paths (same
    arguments), and right behind it simq_grid_waypoints, which simplifies each dense path by the exact rule of include/simq.h
    (approximate_polygon_exact, integer tolerance in [1, 255]) and prunes it against its grid as shortest_paths.pyx:142-149 does.  One
    array comes back for the call: status words, counts, end pixels and waypoints; a problem whose dense path did not fit its first
    buffer, or that has more than WAY_CAPACITY waypoints, is finished by one more pair of launches and one more read-back.
    large_windows: as for grid_dense_paths; simq_grid_waypoints then simplifies the paths of both searches in its one launch, and a
    dense path of more than SIMQ_GRID_WAYPOINTS_MAX_PATH points stays its refusal.

    Returns Waypoints(waypoints, status, endpoints): waypoints, a list of P int32 numpy arrays [m, 2], source first -- what
    prune(grid, dense, approximate_polygon_exact) returns -- and empty for a STRAIGHT problem; status, int32 numpy [P] of TRACED /
    STRAIGHT; endpoints, int32 numpy [P, 4], the (source, target) pixels the search used."""
    if isinstance(tolerance, bool) or int(tolerance) != tolerance or not 1 <= int(tolerance) <= 255:
        raise ValueError('grid_waypoints takes an integer tolerance in [1, 255], got %r' % (tolerance,))
    tolerance = int(tolerance)
    _check_large_windows(large_windows)
    dev, packed, closest_buf, descs = _prepare(grids, sources, targets, grid_index, thin, closest)
    order, n_fit = _window_order(descs, large_windows)   # (the launches, and everything up to the return, in this order)
    descs = [descs[p] for p in order]
    capacities = [min(d['capacity'], WAY_CAPACITY) for d in descs]
    lengths, status, ends, wstatus, counts, ways = _search_and_simplify(dev, packed, closest_buf, descs, capacities, tolerance, n_fit)
    _raise_for(status)
    _raise_for_waypoints(wstatus)
    status, ends = status.copy(), ends.copy()
    starts = np.concatenate([[0], np.cumsum(capacities)])
    out = [ways[starts[p]:starts[p] + max(0, min(counts[p], capacities[p]))].copy() for p in range(len(descs))]
    short = np.flatnonzero((status == CAPACITY) | (wstatus == CAPACITY))
    if short.size:                                       # buffers that hold the whole dense path and every waypoint, once
        again = _again(descs, short, lengths, ends)
        capacities2 = [int(counts[p]) if status[p] == TRACED else int(lengths[p]) for p in short]
        _, status2, _, wstatus2, counts2, ways2 = _search_and_simplify(dev, packed, None, again, capacities2, tolerance,
                                                                       int((short < n_fit).sum()))
        _raise_for(status2, allow_capacity=False)
        _raise_for_waypoints(wstatus2, allow_capacity=False)
        o = 0
        for p, n, cap in zip(short, counts2, capacities2):
            out[p] = ways2[o:o + n].copy()
            o += cap
            status[p] = TRACED
    back = np.argsort(order)
    return Waypoints(restore_order(order, out), status[back], ends[back])


def _raise_for_waypoints(status, allow_capacity=True):
    bad, codes = _batch.bad_problems(status, (0, 1, CAPACITY) if allow_capacity else (0,))
    if bad.size:
        raise SimqError('simq_grid_waypoints: %d problem(s) failed (status %s at problems %s; 2: a bad length, path status or a point '
                        'outside its grid, 3: waypoint buffer, 4: loop bound)' % (bad.size, codes[:8].tolist(), bad[:8].tolist()))


def _raise_for(status, allow_capacity=True):
    bad, codes = _batch.bad_problems(status, (TRACED, STRAIGHT, CAPACITY) if allow_capacity else (TRACED, STRAIGHT))
    if bad.size:
        raise SimqError('simq_grid_paths: %d problem(s) failed (status %s at problems %s; 2: a free cell outside the declared box or a '
                        'closest cell outside the grid, 3: path buffer, 4: pop cap)' % (bad.size, codes[:8].tolist(), bad[:8].tolist()))


class WaypointGraph(GridGraph):
    """shortest_paths.GridGraph with its waypoints: GridGraph's distance methods plus dense_path and shortest_path.

    Results are cached per source, as _spfa_with_cache does: the parent and distance images come back as host arrays from one launch,
    and every further target from that source is a host walk with no launch.  shortest_path_image of a source already searched for a
    path returns that search's distance image."""

    #: replaces the device search when set: callable(grid, source) -> (distances float32 [rows, cols], parents int32 [rows, cols]);
    #: the tests pin the host half (walk, pruning, reversal) through it without a device
    search = None

    def __init__(self, grid, large_windows=False):
        """large_windows: as for grid_dense_paths -- a grid whose free cells span a box over the LDS cap is searched in device memory
        instead of being refused."""
        super().__init__(grid)
        self.large_windows = _check_large_windows(large_windows)
        self.parents = {}

    def _parents(self, source):
        if source not in self.parents:
            if self.search is not None:
                dist, par = self.search(self.grid, source)
            else:
                if self._dev_grid is None:
                    self._dev_grid = torch.from_numpy(self.grid).to(_batch.device('grid distance images'))
                got = grid_dense_paths([self._dev_grid], [source], [source], parents=True, distances=True,
                                       large_windows=self.large_windows)
                par, dist = got.parents[0].cpu().numpy(), got.distances[0].cpu().numpy()
            self.parents[source] = np.asarray(par, np.int32)
            self.cache.setdefault(source, np.asarray(dist, np.float32))
        return self.parents[source]

    def dense_path(self, source, target):
        """The dense path of shortest_paths.pyx:126-137 as an int32 array [n, 2], target first."""
        source, target = self._pixel_in_grid(source, 'source'), self._pixel_in_grid(target, 'target')
        return walk(self._parents(source), source, target)

    def shortest_path(self, source, target, simplify=None):
        """The waypoints of GridGraph.shortest_path (shortest_paths.pyx:121-154) as a list of (i, j), source first.  simplify:
        callable(coords, tolerance) standing in for skimage.measure.approximate_polygon (the default, imported here), or 'exact' for
        approximate_polygon_exact -- on the host here: this object's paths are host walks over cached parents."""
        simplify = _simplifier(simplify)
        return prune(self.grid, self.dense_path(source, target), simplify)


def shortest_paths(cspace, cspace_thin, closest, source_positions, target_positions, map_index=None, simplify=None,
                   large_windows=False):
    """OccupancyMap.shortest_path (envs.py:2477-2504) for P robots in one launch, on the device tensors simq.occupancy_maps returned.

    cspace, cspace_thin: M uint8 maps each ([M, rows, cols] tensor or a list), closest: M int32 [2, rows, cols]; source_positions,
    target_positions: P positions (x, y[, z]); map_index: the map of each problem (problem p uses map p when omitted).  Positions
    become pixels and pixels positions on the host, in float64 as the reference's scalars; the straight-line test, the snap to the
    closest free cells, the search and the walk run on the device; simplification (simplify, default
    skimage.measure.approximate_polygon) and pruning run on the host, over the free-cell boxes of the maps that had a problem that was
    not straight -- nothing else of a configuration space is downloaded.  With simplify='exact' they run on the device as well
    (grid_waypoints): one small array of status words, counts, end pixels and waypoints is read back, no dense path and no map.
    large_windows: as for grid_dense_paths, for maps whose free cells span a box over the LDS cap.
    Returns P lists of positions: the two given tuples when the line is clear or the path has fewer than two waypoints, otherwise
    (x, y, 0) tuples with the given tuples at both ends."""
    if isinstance(simplify, str):
        _simplifier(simplify)                                 # (an unknown name is refused before anything is queued)
    _check_large_windows(large_windows)
    maps, _ = _batch.as_maps(cspace, 'cspace')
    P = len(source_positions)
    if len(target_positions) != P or P < 1:
        raise ValueError('%d source positions but %d target positions' % (P, len(target_positions)))
    map_index = _batch.problem_index(map_index, len(maps), P, '%d maps but %d positions (map_index shares maps between problems)' % (len(maps), P),
                                     'map_index must name one of the %d maps for each of the %d positions' % (len(maps), P))
    srcs = [position_to_pixel_indices(s[0], s[1], tuple(maps[k].shape)) for s, k in zip(source_positions, map_index)]
    tgts = [position_to_pixel_indices(t[0], t[1], tuple(maps[k].shape)) for t, k in zip(target_positions, map_index)]
    on_device = isinstance(simplify, str)
    large = {'large_windows': True} if large_windows else {}          # (the default call is the call as it was)
    if on_device:
        got = grid_waypoints(maps, srcs, tgts, grid_index=map_index, thin=cspace_thin, closest=closest, **large)
    else:
        got = grid_dense_paths(maps, srcs, tgts, grid_index=map_index, thin=cspace_thin, closest=closest, **large)
        if (got.status == TRACED).any():
            simplify = _simplifier(simplify)
    host_maps, result = {}, []
    for p, k in enumerate(map_index):
        source_position, target_position = source_positions[p], target_positions[p]
        if got.status[p] == STRAIGHT:
            result.append([source_position, target_position])
            continue
        if on_device:
            pixels = got.waypoints[p].tolist()
        else:
            if k not in host_maps:
                host_maps[k] = _download_box(maps[k], got.paths, [q for q in range(P) if map_index[q] == k and got.status[q] == TRACED])
            pixels = prune(host_maps[k], got.paths[p], simplify)
        shape = tuple(maps[k].shape)
        path = []
        for i, j in pixels:
            position_x, position_y = pixel_indices_to_position(i, j, shape)
            path.append((position_x, position_y, 0))
        if len(path) < 2:
            path = [source_position, target_position]
        else:
            path[0] = source_position
            path[-1] = target_position
        result.append(path)
    return result


def _download_box(grid, paths, problems):
    """A host grid of zeros holding the cells of `grid` over the box that the dense paths of `problems` span: every line the pruning
    draws joins two cells of one path, so it stays inside that box."""
    pts = np.concatenate([paths[q] for q in problems])
    i0, j0, i1, j1 = int(pts[:, 0].min()), int(pts[:, 1].min()), int(pts[:, 0].max()) + 1, int(pts[:, 1].max()) + 1
    host = np.zeros(tuple(grid.shape), np.uint8)
    part = grid[i0:i1, j0:j1]
    host[i0:i1, j0:j1] = part.cpu().numpy() if isinstance(part, torch.Tensor) else part
    return host
