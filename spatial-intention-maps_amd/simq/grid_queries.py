"""Shortest-path distance queries on the GPU: the point form of ``simq.grid_distance_images``.

Every partial reward of the reference (envs.py:1082-1087, 1210-1215, 1331-1335) is a difference of two
``Mapper.distance_to_receptacle`` values (envs.py:2189-2194), each an ``OccupancyMap.shortest_path_distance`` (envs.py:2506-2511):
positions to pixels, both pixels through ``closest_cspace_indices``, ``GridGraph.shortest_path_distance`` from the receptacle, divided
by the pixels per metre.  ``simq_grid_distance_queries`` (csrc/grid_queries.hip) answers many (source, targets) problems in one
launch -- the snap, the search of ``simq_grid_distance_images`` and the lookups -- on the configuration spaces and closest cells that
``simq.occupancy_maps`` left on the device, and returns one packed array of raw fp32 distances.  The division stays on the host, in
float64 as the reference's Python floats.
"""
import ctypes
import math

import numpy as np
import torch

from . import _batch
from ._lib import SimqError, lib, ptr, stream_ptr
from .grid_paths import index_grids, pixel
from .local_maps import PIXELS_PER_METER, position_to_pixel_indices
from .waypoints import _check_closest


class GridQueryProblem(ctypes.Structure):
    """simq_grid_query_problem of include/simq.h."""
    _fields_ = [(n, ctypes.c_int64) for n in ('grid_offset', 'closest_offset', 'work_offset', 'target_offset')] + \
               [(n, ctypes.c_int32) for n in ('n_targets', 'rows', 'cols', 'src_i', 'src_j', 'reserved_')]


def _pixels(targets, what):
    try:
        return [[pixel(t) for t in ts] for ts in targets]
    except TypeError:
        raise ValueError('%s holds one sequence of pixels (i, j) per problem' % what) from None


def _launch(grids, srcs, tgts, grid_index, closest, images):
    """One simq_grid_distance_queries call.  Returns (small, counts, work, shapes): `small`, one float32 device buffer holding the
    packed distances and behind them the int32 status words of the P problems; the number of targets of each problem; the packed
    working images.  Nothing is read back here."""
    used = sorted(set(grid_index))
    if closest is not None:
        if len(closest) != len(grids):
            raise ValueError('closest must hold one map per grid (%d), got %d' % (len(grids), len(closest)))
        for k in used:
            if closest[k] is not None and tuple(closest[k].shape[-2:]) != tuple(grids[k].shape):
                raise ValueError('closest[%d] is %s but grids[%d] is %s' % (k, tuple(closest[k].shape), k, tuple(grids[k].shape)))
    dev = _batch.device('grid distance queries')         # (after the argument checks: those need no device)

    packed, offsets = _batch.pack([grids[k] for k in used], torch.uint8, dev)
    goff = dict(zip(used, offsets))
    closest_buf, coff = None, {}
    if closest is not None:
        snapped = [k for k in used if closest[k] is not None]
        closest_buf, offsets = _batch.pack([closest[k] for k in snapped], torch.int32, dev)
        coff = dict(zip(snapped, offsets))
    P = len(srcs)
    shapes = [tuple(grids[k].shape) for k in grid_index]
    counts = [len(ts) for ts in tgts]
    total = sum(counts)
    probs = (GridQueryProblem * P)()
    wo = to = 0
    for p, (k, (r, c), (i, j), q) in enumerate(zip(grid_index, shapes, srcs, counts)):
        probs[p] = GridQueryProblem(goff[k], coff.get(k, -1), wo, to, q, r, c, i, j, 0)
        wo += r * c
        to += q
    flat = np.asarray([t for ts in tgts for t in ts], np.int32).reshape(-1, 2)
    desc = torch.empty(ctypes.sizeof(probs) + 8 * total, dtype=torch.uint8, device=dev)
    work = torch.empty(wo, dtype=torch.float32, device=dev)
    small = torch.empty(total + P, dtype=torch.float32, device=dev)                 # distances | status
    out, status = small[:total], small[total:].view(torch.int32)
    lib.call('simq_grid_distance_queries', ptr(packed), ctypes.c_int64(packed.numel()), ptr(closest_buf),
             ctypes.c_int64(0 if closest_buf is None else closest_buf.numel()), probs, P,
             flat.ctypes.data_as(ctypes.c_void_p) if total else None, ctypes.c_int64(total), ptr(desc), ptr(work), ctypes.c_int64(wo),
             int(bool(images)), ptr(out) if total else None, ctypes.c_int64(total), ptr(status), stream_ptr(dev))
    return small, counts, work, shapes


def _raise_for(status):
    bad, codes = _batch.bad_problems(status)
    if bad.size:
        raise SimqError('simq_grid_distance_queries: %d problem(s) failed (status %s at problems %s; 1: pass cap, 2: a closest cell '
                        'outside the grid)' % (bad.size, codes[:8].tolist(), bad[:8].tolist()))


def _split(flat, counts):
    out, o = [], 0
    for q in counts:
        out.append(flat[o:o + q])
        o += q
    return out


def _check_problems(grids, srcs, tgts, grid_index, what):
    if not grids or not srcs:
        raise ValueError('%s needs at least one grid and one source' % what)
    if len(tgts) != len(srcs):
        raise ValueError('%d sources but %d target lists' % (len(srcs), len(tgts)))
    return index_grids(grid_index, len(grids), len(srcs))


def grid_distance_queries(grids, sources, targets, grid_index=None, closest=None, images=False):
    """The shortest-path distances from P sources to their targets in one launch: GridGraph.shortest_path_distance
    (shortest_paths.pyx:150-158) behind the snap of OccupancyMap.shortest_path_distance (envs.py:2509-2510).

    grids, grid_index: as grid_distance_images (2-D uint8 numpy arrays or device tensors, or one [G, rows, cols] array / tensor; free
    where nonzero; problem p uses grids[grid_index[p]], grid p when omitted).  sources: P pixels (i, j).  targets: P sequences of
    pixels, of any lengths, empty ones included.  closest: one int32 [2, rows, cols] per grid (closest_cspace_indices, as
    simq.occupancy_maps returns it), or None for a grid whose problems are not snapped; with it the source and every target are
    replaced by closest[:, i, j] before the search; a device tensor stays on the device.

    Returns a list of P float32 device tensors, views into one packed tensor: the raw distance to each target, -1 where it is
    unreachable.  With images=True returns (distances, images): images is a list of P float32 [rows, cols] device views, each what
    grid_distance_images gives for the snapped source.  Raises SimqError for what the library refuses (a pixel outside its grid, ...;
    nothing is launched) and for a problem whose closest cells lie outside the grid."""
    grids, _ = _batch.as_maps(grids, 'grids')
    srcs, tgts = [pixel(s) for s in sources], _pixels(targets, 'targets')
    grid_index = _check_problems(grids, srcs, tgts, grid_index, 'grid_distance_queries')
    if closest is not None:
        closest, _ = _batch.as_maps(closest, 'closest', lambda c, what: c if c is None else _check_closest(c, what))
    small, counts, work, shapes = _launch(grids, srcs, tgts, grid_index, closest, images)
    total = sum(counts)
    _raise_for(small[total:].view(torch.int32))
    dists = _split(small[:total], counts)
    return (dists, _batch.views(work, shapes)) if images else dists


def _position(p, what):
    try:
        return float(p[0]), float(p[1])
    except (TypeError, ValueError, IndexError):
        raise ValueError('%s is a position (x, y[, z]), got %r' % (what, p)) from None


def _position_lists(positions, P, what):
    try:
        lists = [list(ps) for ps in positions]
    except TypeError:
        raise ValueError('%s holds one sequence of positions (x, y[, z]) per problem' % what) from None
    if len(lists) != P:
        raise ValueError('%d source positions but %d lists of %s' % (P, len(lists), what))
    return [[_position(q, '%s[%d][%d]' % (what, p, k)) for k, q in enumerate(ps)] for p, ps in enumerate(lists)]


def shortest_path_distances(cspace, closest, source_positions, target_positions, map_index=None, pixels_per_meter=PIXELS_PER_METER):
    """OccupancyMap.shortest_path_distance (envs.py:2506-2511) for P sources and all their targets in one launch, on the device
    tensors simq.occupancy_maps returned.

    cspace: M uint8 maps ([M, rows, cols] tensor or a list), closest: M int32 [2, rows, cols]; source_positions: P positions
    (x, y[, z]); target_positions: P sequences of positions; map_index: the map of each problem (problem p uses map p when omitted).
    Positions become pixels on the host (Mapper.position_to_pixel_indices, in float64 as the reference's scalars); snap, search and
    lookups run on the device; the packed fp32 distances are read back once and divided by pixels_per_meter in float64, as the
    reference divides a Python float by a Python float.  Returns P float64 numpy arrays, one value per target; an unreachable target
    gives -1 / pixels_per_meter, as there."""
    maps, _ = _batch.as_maps(cspace, 'cspace')
    try:
        P = len(source_positions)
    except TypeError:
        raise ValueError('source_positions holds one position (x, y[, z]) per problem') from None
    if P < 1 or not maps:
        raise ValueError('shortest_path_distances needs at least one map and one source position')
    srcs = [_position(s, 'source_positions[%d]' % p) for p, s in enumerate(source_positions)]
    tgts = _position_lists(target_positions, P, 'target_positions')
    ppm = float(pixels_per_meter)
    if not (ppm > 0 and math.isfinite(ppm)):
        raise ValueError('pixels_per_meter = %r (> 0, finite)' % (pixels_per_meter,))
    map_index = _batch.problem_index(map_index, len(maps), P, '%d maps but %d positions (map_index shares maps between problems)' % (len(maps), P),
                                     'map_index must name one of the %d maps for each of the %d positions' % (len(maps), P))
    if closest is None:
        raise ValueError('closest is the closest_cspace_indices of every map (simq.occupancy_maps returns them), got None')
    closest, _ = _batch.as_maps(closest, 'closest', _check_closest)
    shapes = [tuple(maps[k].shape) for k in map_index]
    src_px = [position_to_pixel_indices(x, y, shape) for (x, y), shape in zip(srcs, shapes)]
    tgt_px = [[position_to_pixel_indices(x, y, shape) for x, y in ts] for ts, shape in zip(tgts, shapes)]
    small, counts, _, _ = _launch(maps, src_px, tgt_px, map_index, closest, False)
    host = small.cpu().numpy()                                                      # the one read-back: distances and status words
    total = sum(counts)
    _raise_for(host[total:].view(np.int32))
    return _split(host[:total].astype(np.float64) / ppm, counts)


def distances_to_receptacle(cspace, closest, receptacle_positions, positions, map_index=None, shortest_path=True):
    """Mapper.distance_to_receptacle (envs.py:2189-2194) for the cubes of P robots in one launch.

    receptacle_positions: P positions, the receptacle of each problem's environment; positions: P sequences of positions (the cubes'
    before and after a step, say).  With shortest_path (use_shortest_path_partial_rewards) the receptacle is the source, as in the
    reference, so one search serves all positions of a problem: shortest_path_distances(cspace, closest, receptacle_positions,
    positions, map_index).  Without it the result is the reference's distance(position, receptacle_position) (envs.py:2556-2557),
    computed on the host in float64 in its order of operations; cspace, closest and map_index are not looked at.  Returns P float64
    numpy arrays."""
    if shortest_path:
        return shortest_path_distances(cspace, closest, receptacle_positions, positions, map_index)
    try:
        P = len(receptacle_positions)
    except TypeError:
        raise ValueError('receptacle_positions holds one position (x, y[, z]) per problem') from None
    recs = [_position(s, 'receptacle_positions[%d]' % p) for p, s in enumerate(receptacle_positions)]
    lists = _position_lists(positions, P, 'positions')
    return [np.asarray([math.sqrt((p2[0] - p1[0])**2 + (p2[1] - p1[1])**2) for p1 in ps], np.float64) for p2, ps in zip(recs, lists)]
