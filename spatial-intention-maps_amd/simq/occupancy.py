"""Occupancy maps on the GPU: what the reference's ``OccupancyMap.update`` derives from the occupancy map.

The reference (envs.py:2452-2455) recomputes, per robot per step, the configuration space (the room minus the occupied cells dilated
with a disk of the robot's radius), the closest free cell of every pixel (``scipy.ndimage.distance_transform_edt(...,
return_indices=True)``, through which every shortest-path source pixel goes, envs.py:2522-2523) and a thin configuration space for the
straight-line test.  ``simq_occupancy_maps`` (csrc/occupancy_maps.hip) computes the three for many maps in one launch, element for
element equal to that sequence; the rules and scipy's tie rule are stated in include/simq.h.  A row of the configuration space is a
grid ``simq.grid_distance_images`` takes as it is.  The kernel keeps its planes in LDS, which bounds a map's sides by MAX_DIM;
large_maps=True sends the maps over that bound to ``simq_occupancy_maps_large``, the same passes with the plane in a workspace in
device memory.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _batch
from ._lib import SimqError, lib, ptr, stream_ptr

MAX_DIM = 256                    # SIMQ_OCCUPANCY_MAX_DIM of include/simq.h
LARGE_MAX_DIM = 2048             # SIMQ_OCCUPANCY_LARGE_MAX_DIM
MAX_RADIUS = 16                  # SIMQ_OCCUPANCY_MAX_RADIUS

OccupancyMaps = collections.namedtuple('OccupancyMaps', ('configuration_space', 'cspace_thin', 'closest_cspace_indices'))


class OccupancyProblem(ctypes.Structure):
    """simq_occupancy_problem of include/simq.h."""
    _fields_ = [('occupancy_offset', ctypes.c_int64), ('mask_offset', ctypes.c_int64), ('out_offset', ctypes.c_int64),
                ('rows', ctypes.c_int32), ('cols', ctypes.c_int32), ('radius', ctypes.c_int32), ('thin_radius', ctypes.c_int32)]


class OccupancyLargeProblem(ctypes.Structure):
    """simq_occupancy_large_problem of include/simq.h: OccupancyProblem's fields plus work_offset."""
    _fields_ = OccupancyProblem._fields_[:3] + [('work_offset', ctypes.c_int64)] + OccupancyProblem._fields_[3:]


MAPS = 'a sequence of 2-D uint8 maps or one [G, rows, cols] array'


def large_work_bytes(rows, cols):
    """simq_occupancy_maps_large_work_bytes of include/simq.h restated: one uint16 per cell, rounded up to 16."""
    return (2 * rows * cols + 15) // 16 * 16


def split_by_shape(shapes):
    """(fit, over): the problems whose map (rows, cols) has both sides within MAX_DIM -- simq_occupancy_maps takes them, its planes
    in LDS -- and the others, for simq_occupancy_maps_large; both ascending."""
    fit = [p for p, s in enumerate(shapes) if s[0] <= MAX_DIM and s[1] <= MAX_DIM]
    over = [p for p, s in enumerate(shapes) if s[0] > MAX_DIM or s[1] > MAX_DIM]
    return fit, over


def entry_calls(n_fit, n):
    """The entry points a call over n problems makes when the first n_fit fit the LDS cap: [(name, first, last + 1)], an empty part
    left out."""
    return [c for c in (('simq_occupancy_maps', 0, n_fit), ('simq_occupancy_maps_large', n_fit, n)) if c[2] > c[1]]


def _check_large_maps(large_maps):
    if not isinstance(large_maps, bool):
        raise ValueError('large_maps must be True or False, got %r' % (large_maps,))
    return large_maps


def launch_order(shapes, large_maps):
    """(order, n_fit): the problems in the order they are launched -- with large_maps those over the LDS cap behind the others, for
    simq_occupancy_maps_large; without it all as they come, for simq_occupancy_maps to take or refuse."""
    if not large_maps:
        return list(range(len(shapes))), len(shapes)
    fit, over = split_by_shape(shapes)
    return fit + over, len(fit)


def call_entries(fields, n_fit, maps, outs, status, dev, work=None, work_at=None):
    """Queues the call over `fields`, one (occupancy_offset, mask_offset, out_offset, rows, cols, radius, thin_radius) per problem in
    launch order: the first n_fit through simq_occupancy_maps, the others through simq_occupancy_maps_large; both read `maps`, write
    their own problems' ranges of the three tensors `outs` and their own words of `status` (int32 [len(fields)], launch order).
    work, work_at: the workspace of the large part and each of its problems' byte offset in it; allocated here when omitted."""
    cspace, thin, closest = outs
    for name, a, b in entry_calls(n_fit, len(fields)):
        extra = ()
        if name == 'simq_occupancy_maps':
            probs = (OccupancyProblem * (b - a))(*[OccupancyProblem(*f) for f in fields[a:b]])
        else:
            if work is None:
                need = [large_work_bytes(f[3], f[4]) for f in fields[a:b]]
                work_at = np.concatenate([[0], np.cumsum(need)]).astype(np.int64).tolist()
                work = torch.empty(work_at[-1], dtype=torch.uint8, device=dev)
            probs = (OccupancyLargeProblem * (b - a))(*[OccupancyLargeProblem(*f[:3], int(work_at[k]), *f[3:])
                                                        for k, f in enumerate(fields[a:b])])
            extra = (ptr(work), ctypes.c_int64(work.numel()))
        d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
        lib.call(name, ptr(maps), ctypes.c_int64(maps.numel()), probs, b - a, ptr(d_probs), ptr(cspace), ptr(thin),
                 ctypes.c_int64(min(cspace.numel(), thin.numel())), ptr(closest), ctypes.c_int64(closest.numel()), ptr(status[a:b]), *extra,
                 stream_ptr(dev))


def _radii(radius, P, what):
    try:
        values = [radius] * P if isinstance(radius, (int, np.integer)) and not isinstance(radius, bool) else list(radius)
    except TypeError:
        raise ValueError('%s = %r (a whole number in 0 .. %d, or one per problem)' % (what, radius, MAX_RADIUS)) from None
    if len(values) != P:
        raise ValueError('%d values of %s for %d problems' % (len(values), what, P))
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= MAX_RADIUS:
            raise ValueError('%s = %r (a whole number in 0 .. %d)' % (what, v, MAX_RADIUS))
    return [int(v) for v in values]


def _enqueue(occupancy, room_masks, radius, thin_radius, room_index=None, out=None, large_maps=False):
    """occupancy_maps without its status read-back: checks, uploads and queues the launch (with large_maps the two of
    launch_order), and returns (out, status, uniform, shapes) with `out` the three output tensors and `status` the int32 device
    tensor of the status words in problem order."""
    _check_large_maps(large_maps)
    occupancy, occupancy_block = _batch.as_maps(occupancy, 'occupancy', expects=MAPS)
    room_masks, _ = _batch.as_maps(room_masks, 'room_masks', expects=MAPS)
    P = len(occupancy)
    if P < 1 or not room_masks:
        raise ValueError('occupancy_maps needs at least one occupancy map and one room mask')
    room_index = _batch.problem_index(
        room_index, len(room_masks), P, '%d occupancy maps but %d room masks (room_index shares masks between problems)' % (P, len(room_masks)),
        'room_index must name one of the %d room masks for each of the %d occupancy maps' % (len(room_masks), P))
    shapes = [tuple(m.shape) for m in occupancy]
    for p, k in enumerate(room_index):
        if tuple(room_masks[k].shape) != shapes[p]:
            raise ValueError('occupancy[%d] is %s but its room mask room_masks[%d] is %s' % (p, shapes[p], k, tuple(room_masks[k].shape)))
    radii, thin_radii = _radii(radius, P, 'radius'), _radii(thin_radius, P, 'thin_radius')
    dev = _batch.device('occupancy maps')       # (after the argument checks: those need no device)

    # one packed uint8 buffer: the occupancy maps (one contiguous block with one copy), then each room mask the problems use once
    used = sorted(set(room_index))
    offsets, n_cells = [], 0
    for r, c in shapes:
        offsets.append(n_cells)
        n_cells += r * c
    packed, at = _batch.pack(([occupancy_block] if occupancy_block is not None else occupancy) + [room_masks[k] for k in used], torch.uint8, dev)
    moff = dict(zip(used, at[len(at) - len(used):]))

    uniform = len(set(shapes)) == 1
    want = [(P,) + shapes[0], (P,) + shapes[0], (P, 2) + shapes[0]] if uniform else [(n_cells,), (n_cells,), (2 * n_cells,)]
    dtypes = [torch.uint8, torch.uint8, torch.int32]
    if out is None:
        out = [torch.empty(w, dtype=d, device=dev) for w, d in zip(want, dtypes)]
    else:
        try:
            out = list(out)
        except TypeError:
            out = [out]
        names = OccupancyMaps._fields
        if len(out) != 3:
            raise ValueError('out must be three tensors (%s)' % ', '.join(names))
        for t, w, d, name in zip(out, want, dtypes, names):
            if not _batch.out_fits(t, d, dev, w if uniform else None, w[0]):
                raise ValueError('out: %s must be a contiguous %s tensor on %s of %s' % (
                    name, str(d).replace('torch.', ''), dev, 'shape %s' % (w,) if uniform else 'at least %d elements' % w[0]))
    order, n_fit = launch_order(shapes, large_maps)
    fields = [(offsets[p], moff[room_index[p]], offsets[p], shapes[p][0], shapes[p][1], radii[p], thin_radii[p]) for p in order]
    status = torch.empty(P, dtype=torch.int32, device=dev)
    call_entries(fields, n_fit, packed, out, status, dev)
    if order != list(range(P)):                 # (the words back in problem order)
        status = status[torch.as_tensor(np.argsort(order), dtype=torch.int64).to(dev)]
    return out, status, uniform, shapes


def occupancy_maps(occupancy, room_masks, radius, thin_radius, room_index=None, out=None, large_maps=False):
    """The configuration spaces, thin configuration spaces and closest free cells of P occupancy maps in one launch, on the device.

    occupancy: P 2-D uint8 maps (C-contiguous numpy arrays or contiguous uint8 device tensors, read with a device copy), or one
    [P, rows, cols] array / tensor; a cell is occupied where nonzero (OccupancyMap.occupancy_map).  room_masks: the same for the room
    masks (OccupancyMap.room_mask: nonzero inside the room).  room_index: P indices into `room_masks` (several problems may share one
    mask); omitted, problem p uses mask p.  radius: floor(robot.RADIUS * 96) of envs.py:2420, thin_radius: ceil(Robot.HALF_WIDTH * 96)
    of envs.py:2428 -- ints, or one per problem.

    Returns the named triple (configuration_space, cspace_thin, closest_cspace_indices) of envs.py:2453-2455: uint8 [P, rows, cols]
    twice and int32 [P, 2, rows, cols] (scipy's return_indices layout) device tensors when every problem has the same shape, otherwise
    three lists of P views ([rows_p, cols_p] twice, [2, rows_p, cols_p]) into packed buffers.  out: three contiguous device tensors to
    write into, of those shapes (mixed shapes: uint8 of at least sum(rows_p * cols_p) elements twice and int32 of at least twice as
    many); every element is written.

    A map with a side over MAX_DIM is refused (SimqError, nothing launched) unless large_maps is True.  Then the problems within
    MAX_DIM x MAX_DIM go to simq_occupancy_maps as before and the others, sides up to LARGE_MAX_DIM, to simq_occupancy_maps_large with a
    workspace allocated here (2 bytes a cell); both write their own ranges of the same outputs, and the results come in problem order.

    Raises ValueError for a wrong dtype, rank or contiguity, SimqError for what the library refuses (launching nothing) and for the
    problems whose configuration space has no free cell (their closest cells are undefined)."""
    out, status, uniform, shapes = _enqueue(occupancy, room_masks, radius, thin_radius, room_index, out, large_maps)
    bad, codes = _batch.bad_problems(status)
    if bad.size:
        if (codes == 1).all():
            raise SimqError('simq_occupancy_maps: the configuration space of %d problem(s) has no free cell, their closest cells are '
                            'undefined (problems %s)' % (bad.size, bad[:8].tolist()))
        raise SimqError('simq_occupancy_maps: %d problem(s) failed (status %s at problems %s)' % (bad.size, codes[:8].tolist(), bad[:8].tolist()))
    if uniform:
        return OccupancyMaps(*out)
    return OccupancyMaps(_batch.views(out[0].view(-1), shapes), _batch.views(out[1].view(-1), shapes),
                         _batch.views(out[2].view(-1), [(2,) + s for s in shapes]))


def configuration_space(occupancy_map, room_mask, radius, thin_radius, large_maps=False):
    """The three results of OccupancyMap.update (envs.py:2453-2455) for one map, as numpy arrays: (configuration_space uint8
    [rows, cols], cspace_thin uint8 [rows, cols], closest_cspace_indices int32 [2, rows, cols]).  large_maps: as for occupancy_maps."""
    got = occupancy_maps([occupancy_map], [room_mask], radius, thin_radius, large_maps=large_maps)
    return OccupancyMaps(*[t[0].cpu().numpy() for t in got])
