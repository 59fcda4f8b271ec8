"""Global intention and history maps on the GPU: the line-drawing stage of the reference's ``Mapper.get_state``.

The reference (envs.py:2301-2346) draws, per robot per step, the paths of the other robots into a zero map of the padded-room shape
with ``skimage.draw.line`` -- a constant (``binary``, ``line``, ``circle``) or a ramp that falls from 1 along the path (``ramp``,
``history``) -- and thickens the result with ``dilation(disk(intention_map_line_thickness - 1))``.  ``simq_intention_maps``
(csrc/intention_maps.hip) draws the maps of many robots in one launch, bit for bit equal to that sequence, into a ``[P, rows, cols]``
device tensor whose rows ``simq.local_state_images`` reads in place as ``('map', k)`` channels.  The pixels of the waypoints and the
float64 ramp parameters are computed here in the reference's order of operations and handed to the library; what the library draws
from them is described in include/simq.h.

The per-robot spatial intention channel (envs.py:2360-2366) is one target pixel at ``intention_map_scale``, always dilated with the
same disk: ``encoding='circle'`` with the one robot's target as the problem's only entry (an idle robot: no entry, a map of zeros).
The reference orders those channels from the closest robot to the furthest (envs.py:2350-2354); that ordering stays with the caller,
who lists the problems in the order the channels are wanted.
"""
import ctypes
import math

import numpy as np
import torch

from . import _batch
from ._lib import IntentionShapedProblem as ShapedProblem, lib, ptr, stream_ptr
from .local_maps import as_ctypes, distances, pixel_indices_many, position_to_pixel_indices

ENCODINGS = ('circle', 'ramp', 'binary', 'line', 'history')
STORE, RAMP = 0, 1
MAX_RADIUS = 8                   # SIMQ_INTENTION_MAX_RADIUS of include/simq.h


class Segment(ctypes.Structure):
    """simq_intention_segment of include/simq.h."""
    _fields_ = [('start', ctypes.c_double), ('stop', ctypes.c_double), ('step', ctypes.c_double), ('r0', ctypes.c_int32), ('c0', ctypes.c_int32),
                ('r1', ctypes.c_int32), ('c1', ctypes.c_int32), ('mode', ctypes.c_int32), ('drop_last', ctypes.c_int32),
                ('value', ctypes.c_float), ('reserved_', ctypes.c_int32)]


class Problem(ctypes.Structure):
    """simq_intention_problem of include/simq.h."""
    _fields_ = [('seg_begin', ctypes.c_int32), ('seg_count', ctypes.c_int32)]


def _length(a, b):
    """The distance of envs.py:2556-2557 between two waypoints, on the values as they are given (so that Python floats take the
    reference's own float operations)."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    return math.sqrt(dx**2 + dy**2)


def segments(robots, map_shape, encoding, scale=1.0):
    """The segment descriptors of one map as tuples (r0, c0, r1, c1, mode, drop_last, value, start, stop, step).

    robots: for every drawn robot (every robot of the environment but the mapper's own and the idle ones) what the reference reads
    from it -- its target position for 'circle', controller.get_intention_path() for 'ramp' / 'binary' / 'line',
    controller.get_history_path() for 'history' (reversed here, as envs.py:2317 does; 'line' keeps the first and last waypoint here,
    as envs.py:2315 does)."""
    if encoding not in ENCODINGS:
        raise ValueError('encoding %r: choose from %s' % (encoding, list(ENCODINGS)))
    out = []
    for waypoints in robots:
        if encoding == 'circle':
            try:
                i, j = position_to_pixel_indices(waypoints[0], waypoints[1], map_shape)
            except (TypeError, IndexError):
                raise ValueError("'circle' takes one target position (x, y[, z]) per robot, got %r" % (waypoints,)) from None
            out.append((i, j, i, j, STORE, 0, scale, 0.0, 0.0, 0.0))
            continue
        try:
            waypoints = [(w[0], w[1]) for w in waypoints]
        except (TypeError, IndexError):
            raise ValueError('%r takes a list of waypoint positions (x, y[, z]) per robot, got %r' % (encoding, waypoints)) from None
        if not waypoints:
            raise ValueError('a drawn robot has an empty waypoint list (an idle robot is left out of its problem)')
        if encoding == 'line':
            waypoints = [waypoints[0], waypoints[-1]]
        elif encoding == 'history':
            waypoints = waypoints[::-1]
        pixels = [position_to_pixel_indices(w[0], w[1], map_shape) for w in waypoints]
        path_length = 0
        for k in range(1, len(waypoints)):
            source, target = waypoints[k - 1], waypoints[k]
            segment_length = scale * _length(source, target)
            (r0, c0), (r1, c1) = pixels[k - 1], pixels[k]
            drop_last = int(k < len(waypoints) - 1)
            if encoding in ('binary', 'line'):
                out.append((r0, c0, r1, c1, STORE, drop_last, scale, 0.0, 0.0, 0.0))
            else:
                # np.linspace(start, stop, num) of envs.py:2334 with num = len(rr): step = (stop - start) / (num - 1)
                start, stop = 1 - path_length, 1 - (path_length + segment_length)
                div = max(abs(r1 - r0), abs(c1 - c0))
                step = (stop - start) / div if div > 0 else 0.0
                out.append((r0, c0, r1, c1, RAMP, drop_last, 0.0, float(start), float(stop), float(step)))
            path_length += segment_length
    return out


SEGMENT, PROBLEM = np.dtype(Segment), np.dtype(Problem)      # the descriptor tables as numpy structured arrays (local_maps.as_ctypes)
SHAPED_PROBLEM = np.dtype(ShapedProblem)                     # simq_intention_shaped_problem: a problem with its own place, shape and radius


def _starts(counts):
    """Where each of consecutive runs of `counts` entries begins."""
    return np.cumsum(counts) - counts


def ragged(begin, count):
    """The indices begin[k] .. begin[k] + count[k] - 1 of every k, one range behind the other."""
    count = np.asarray(count, np.int64)
    return np.repeat(np.asarray(begin, np.int64) - _starts(count), count) + np.arange(int(count.sum()), dtype=np.int64)


def circle_segments(targets, rows, cols, scale=1.0):
    """The SEGMENT table of `segments([target], shape, 'circle', scale)` for every row of targets (float64 [D, 2]): one entry each;
    rows, cols: the map shape, one int or an int array [D]."""
    table = np.zeros(len(targets), SEGMENT)
    i, j = pixel_indices_many(targets[:, 0], targets[:, 1], (rows, cols))
    table['r0'], table['c0'], table['r1'], table['c1'], table['mode'], table['value'] = i, j, i, j, STORE, scale
    return table


def path_segments(points, lo, hi, rows, cols, encoding, scale=1.0):
    """The SEGMENT tables of `segments([path], shape, encoding, scale)` for D paths at once, one behind the other, and the number of
    entries of each: path d is points[lo[d]:hi[d]] (points float64 [N, 2], at least one waypoint per path), its map rows[d] x cols[d]
    (or one int for all); encoding one of 'ramp', 'binary', 'line', 'history'.  Every segment is computed once, whoever observes it."""
    if encoding not in ENCODINGS[1:]:
        raise ValueError('encoding %r: choose from %s' % (encoding, list(ENCODINGS[1:])))
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    if (hi <= lo).any():
        raise ValueError('a drawn robot has an empty waypoint list (an idle robot is left out of its problem)')
    D = len(lo)
    count = np.ones(D, np.int64) if encoding == 'line' else hi - lo - 1
    path = np.repeat(np.arange(D), count)
    k = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(_starts(count), count) + 1            # 1 .. count, as segments() counts
    if encoding == 'line':
        source, target = lo[path], hi[path] - 1
    elif encoding == 'history':                                     # the path reversed (envs.py:2317)
        source, target = hi[path] - k, hi[path] - 1 - k
    else:
        source, target = lo[path] + k - 1, lo[path] + k
    shape = (rows if np.ndim(rows) == 0 else np.asarray(rows)[path], cols if np.ndim(cols) == 0 else np.asarray(cols)[path])
    table = np.zeros(len(path), SEGMENT)
    ends, S = points[np.concatenate([source, target])], len(path)
    i, j = pixel_indices_many(ends[:, 0], ends[:, 1], shape if np.ndim(rows) == 0 else (np.tile(shape[0], 2), np.tile(shape[1], 2)))
    table['r0'], table['c0'], table['r1'], table['c1'] = i[:S], j[:S], i[S:], j[S:]
    table['drop_last'] = k < count[path]
    if encoding in ('binary', 'line'):
        table['mode'], table['value'] = STORE, scale
        return table, count
    length = scale * distances(ends[S:, 0] - ends[:S, 0], ends[S:, 1] - ends[:S, 1])
    # the running path_length of segments(): a sum from the left that starts at 0, per path -- np.cumsum along the rows of a table
    # that holds every path's lengths from column 0 on (the zeros behind a shorter path change nothing before them)
    run = np.zeros((D, max(int(count.max()), 1) if D else 1))
    run[path, k - 1] = length
    run = np.cumsum(run, axis=1)
    before = np.where(k > 1, run[path, k - 2], 0.0)
    start, stop = 1 - before, 1 - run[path, k - 1]
    div = np.maximum(np.abs(i[S:] - i[:S]), np.abs(j[S:] - j[:S]))
    step = np.zeros(len(path))
    np.divide(stop - start, div, out=step, where=div > 0)
    table['mode'], table['start'], table['stop'], table['step'] = RAMP, start, stop, step
    return table, count


def check_drawing(scale, line_thickness):
    """The two checks _prepare makes of what every map of a call shares."""
    if int(line_thickness) != line_thickness or not 1 <= line_thickness <= MAX_RADIUS + 1:
        raise ValueError('line_thickness = %r (a whole number in 1 .. %d)' % (line_thickness, MAX_RADIUS + 1))
    value = float(scale)
    if not (math.isfinite(value) and value >= 0) or math.copysign(1.0, value) < 0:
        raise ValueError('scale = %r (finite, >= 0 and not -0)' % (scale,))


def intention_maps(paths, map_shape, encoding, scale=1.0, line_thickness=2, out=None):
    """The [P, rows, cols] float32 global intention / history maps of P problems in one launch, on the device.

    paths[p]: the drawn robots of problem p as `segments` takes them; an empty list gives a map of zeros (an environment whose other
    robots are all idle).  map_shape: (rows, cols) of Mapper.create_padded_room_zeros.  encoding: one of 'circle', 'ramp', 'binary',
    'line', 'history' (env.intention_map_encoding, or 'history' for the history map), or P of them.  scale:
    env.intention_map_scale.  line_thickness: env.intention_map_line_thickness; the maps are dilated with disk(line_thickness - 1)
    (1: not at all).  out: a contiguous float32 device tensor [P, rows, cols] to write into, e.g. a slice of a larger map bank; every
    pixel is written.

    A row of the result is a global map for simq.local_state_images: local_state_images(maps, [('map', k), ...], poses).

    Several room shapes or line thicknesses in the one launch (simq_intention_maps_shapes): map_shape may be a list of P (rows, cols)
    pairs and line_thickness a list of P whole numbers.  With a list of shapes the result is a list of P device views [rows_p, cols_p]
    of one flat float32 tensor, packed in problem order (each is a global map for simq.local_state_images as it is), and `out` a
    contiguous flat float32 device tensor of at least the sum of the cells; with one shape and a list of thicknesses the result and
    `out` are the [P, rows, cols] tensor.
    Raises SimqError, launching nothing, for what the library refuses."""
    if _is_list(line_thickness) or _shape_list(map_shape):
        args, out, keep = _prepare_shapes(paths, map_shape, encoding, scale, line_thickness, out)
        lib.call('simq_intention_maps_shapes', *args)
        del keep
        return out
    args, out, keep = _prepare(paths, map_shape, encoding, scale, line_thickness, out)
    lib.call('simq_intention_maps', *args)
    del keep                                     # (the descriptor scratch: alive until the launch is queued)
    return out


def _is_list(x):
    return isinstance(x, (list, tuple, np.ndarray))


def _shape_list(map_shape):
    """map_shape is a list of (rows, cols) pairs and not one pair."""
    return _is_list(map_shape) and len(map_shape) > 0 and _is_list(map_shape[0])


def _shape(map_shape):
    """(rows, cols) of one map_shape argument as two ints."""
    try:
        rows, cols = int(map_shape[0]), int(map_shape[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError('map_shape is (rows, cols), got %r' % (map_shape,)) from None
    if rows < 1 or cols < 1 or len(map_shape) != 2:
        raise ValueError('map_shape is (rows, cols) with rows, cols >= 1, got %r' % (map_shape,))
    return rows, cols


def _prepare_shapes(paths, map_shape, encoding, scale, line_thickness, out):
    """_prepare for problems with their own shapes or thicknesses: the argument tuple of simq_intention_maps_shapes, what
    intention_maps returns (the views of a flat tensor for a list of shapes, the [P, rows, cols] tensor for one shape) and the device
    tensors the call reads."""
    paths = list(paths)
    P = len(paths)
    if P < 1:
        raise ValueError('intention_maps needs at least one problem')
    several = _shape_list(map_shape)
    shapes = [_shape(s) for s in map_shape] if several else [_shape(map_shape)] * P
    if len(shapes) != P:
        raise ValueError('%d map shapes for %d problems' % (len(shapes), P))
    thicknesses = list(line_thickness) if _is_list(line_thickness) else [line_thickness] * P
    if len(thicknesses) != P:
        raise ValueError('%d line thicknesses for %d problems' % (len(thicknesses), P))
    encodings = [encoding] * P if isinstance(encoding, str) else list(encoding)
    if len(encodings) != P:
        raise ValueError('%d encodings for %d problems' % (len(encodings), P))
    for thickness in thicknesses:
        check_drawing(scale, thickness)

    tables, counts = [], np.zeros(P, np.int64)
    for p in range(P):
        rows = segments(paths[p], shapes[p], encodings[p], scale)
        table = np.zeros(len(rows), SEGMENT)
        for k, (r0, c0, r1, c1, mode, drop_last, v, start, stop, step) in enumerate(rows):
            table[k] = (start, stop, step, r0, c0, r1, c1, mode, drop_last, v, 0)
        tables.append(table)
        counts[p] = len(rows)
    c_segs = np.concatenate([t.view(np.uint8) for t in tables]).view(SEGMENT)
    cells = np.asarray([r * c for r, c in shapes], np.int64)
    c_probs = shaped_problems(shapes, _starts(cells), _starts(counts), counts, np.asarray(thicknesses, np.int64) - 1)
    total = int(cells.sum())
    if several:
        if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.dim() == 1 and out.is_contiguous()
                                    and out.numel() >= total):
            raise ValueError('out must be a contiguous flat float32 tensor of at least %d elements for maps of several shapes, got %s' % (
                total, '%s %s' % (out.dtype, tuple(out.shape)) if isinstance(out, torch.Tensor) else type(out).__name__))
    dev = _batch.device('intention maps')       # (after the argument checks: those need no device)
    want = (total,) if several else (P,) + shapes[0]
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=dev)
    elif not _batch.out_fits(out, torch.float32, dev, None if several else want, total):
        raise ValueError('out must be a contiguous float32 tensor of %s on %s' % ('at least %d elements' % total if several else 'shape %s' % (want,), dev))
    args, d_desc = shapes_call(c_segs, c_probs, out, dev)
    return args, (_batch.views(out[:total], shapes) if several else out), (d_desc, c_segs, c_probs)


def shaped_problems(shapes, out_offset, seg_begin, seg_count, radius):
    """The SHAPED_PROBLEM table of len(shapes) problems from arrays of its fields (radius: one int or an array)."""
    table = np.zeros(len(shapes), SHAPED_PROBLEM)
    shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
    table['rows'], table['cols'], table['out_offset'] = shapes[:, 0], shapes[:, 1], out_offset
    table['seg_begin'], table['seg_count'], table['radius'] = seg_begin, seg_count, radius
    return table


def shapes_call(c_segs, c_probs, out, dev):
    """The argument tuple of simq_intention_maps_shapes for a SEGMENT and a SHAPED_PROBLEM table and the tensor the maps go to, and
    the descriptor scratch of the call (to keep until the launch is queued).  The tables are read during the call only."""
    d_desc = torch.empty(max(int(lib.c.simq_intention_shapes_desc_bytes(len(c_segs), len(c_probs))), 8), dtype=torch.uint8, device=dev)
    return (as_ctypes(c_segs, Segment) if len(c_segs) else None, len(c_segs), as_ctypes(c_probs, ShapedProblem), len(c_probs), ptr(d_desc),
            ctypes.c_int64(d_desc.numel()), ptr(out), ctypes.c_int64(out.numel()), stream_ptr(dev)), d_desc


def _prepare(paths, map_shape, encoding, scale, line_thickness, out):
    """The argument tuple of simq_intention_maps for intention_maps' inputs, the output tensor and the device tensors the call reads
    (tools/intention_maps_rate.py times the library call alone with it)."""
    paths = list(paths)
    P = len(paths)
    if P < 1:
        raise ValueError('intention_maps needs at least one problem')
    try:
        rows, cols = int(map_shape[0]), int(map_shape[1])
    except (TypeError, IndexError, ValueError):
        raise ValueError('map_shape is (rows, cols), got %r' % (map_shape,)) from None
    if rows < 1 or cols < 1 or len(map_shape) != 2:
        raise ValueError('map_shape is (rows, cols) with rows, cols >= 1, got %r' % (map_shape,))
    encodings = [encoding] * P if isinstance(encoding, str) else list(encoding)
    if len(encodings) != P:
        raise ValueError('%d encodings for %d problems' % (len(encodings), P))
    if int(line_thickness) != line_thickness or not 1 <= line_thickness <= MAX_RADIUS + 1:
        raise ValueError('line_thickness = %r (a whole number in 1 .. %d)' % (line_thickness, MAX_RADIUS + 1))
    value = float(scale)
    if not (math.isfinite(value) and value >= 0) or math.copysign(1.0, value) < 0:
        raise ValueError('scale = %r (finite, >= 0 and not -0)' % (scale,))

    c_segs_list, ranges = [], []
    for p in range(P):
        begin = len(c_segs_list)
        for r0, c0, r1, c1, mode, drop_last, v, start, stop, step in segments(paths[p], (rows, cols), encodings[p], scale):
            c_segs_list.append(Segment(start, stop, step, r0, c0, r1, c1, mode, drop_last, v, 0))
        ranges.append((begin, len(c_segs_list) - begin))
    n_segs = len(c_segs_list)
    c_segs = (Segment * max(n_segs, 1))(*c_segs_list)
    c_probs = (Problem * P)(*[Problem(b, c) for b, c in ranges])

    dev = _batch.device('intention maps')       # (after the argument checks: those need no device)
    want = (P, rows, cols)
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=dev)
    elif not _batch.out_fits(out, torch.float32, dev, want):
        raise ValueError('out must be a contiguous float32 tensor of shape %s on %s' % (want, dev))
    desc_bytes = lib.c.simq_intention_desc_bytes(n_segs, P)
    d_desc = torch.empty(max(int(desc_bytes), 8), dtype=torch.uint8, device=dev)
    args = (c_segs if n_segs else None, n_segs, c_probs, P, rows, cols, int(line_thickness) - 1, ptr(d_desc), ctypes.c_int64(d_desc.numel()),
            ptr(out), ctypes.c_int64(out.numel()), stream_ptr(dev))
    return args, out, (d_desc,)


def intention_map(robots, map_shape, encoding, scale=1.0, line_thickness=2):
    """Drop-in for Mapper._create_global_intention_or_history_map(encoding) (envs.py:2301-2346) with the drawn robots' paths passed
    in: the float32 [rows, cols] numpy map.  With encoding='circle', one target and the environment's line thickness it is the
    global map of one spatial intention channel (envs.py:2360-2365)."""
    return intention_maps([robots], map_shape, encoding, scale, line_thickness)[0].cpu().numpy()
