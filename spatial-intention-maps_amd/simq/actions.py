"""Robot.store_new_action (envs.py:856-902) for many robots in one call: actions to waypoint positions and headings.

The rule is stated in include/simq.h (simq_action_waypoints) and DESIGN.md section 21.  The device does what is integer and fp32 --
the straight-line test, the snap, the search, the walk, the exact simplification and the pruning of OccupancyMap.shortest_path, one
launch of ``simq_action_waypoints`` (csrc/action_waypoints.hip) on the maps where they lie -- and the host does every float64: the
library has no trigonometry, and the reference's numbers are CPython's ``math``.  The host side is arrays in and arrays out:
elementwise numpy where numpy's operation is the C double operation (+, -, *, /, sqrt, floor; float_power for ``** 2``), and one
comprehension over ``math`` for each libm function and for the float ``%``.
"""
import ctypes
import math

import numpy as np
import torch

from . import _batch, arch
from ._lib import SimqError, lib, ptr, stream_ptr
from .intention_drawing import _starts, ragged
from .local_maps import PIXELS_PER_METER, as_ctypes, distances, pixel_indices_many

WIDTH = arch.STATE_WIDTH                               # Mapper.LOCAL_MAP_PIXEL_WIDTH
TRACED, STRAIGHT, BAD_DESCRIPTOR, CAPACITY = 0, 1, 2, 3
WAY_CAPACITY = 64                                      # pairs per robot in the first read-back (grid_waypoints'); a longer list costs one more round
MAX_BOX_CELLS = 20000                                  # SIMQ_GRID_PATH_MAX_BOX_CELLS of include/simq.h
TWO_PI = 2 * math.pi


class ActionWaypointProblem(ctypes.Structure):
    """simq_action_waypoint_problem of include/simq.h."""
    _fields_ = [(n, ctypes.c_int64) for n in ('cspace_offset', 'thin_offset', 'closest_offset', 'way_offset')] + \
               [(n, ctypes.c_int32) for n in ('way_capacity', 'rows', 'cols', 'src_i', 'src_j', 'tgt_i', 'tgt_j', 'box_i0', 'box_j0', 'box_rows',
                                              'box_cols', 'upstream')]


class ActionWaypointLargeProblem(ctypes.Structure):
    """simq_action_waypoint_large_problem of include/simq.h: ActionWaypointProblem's fields plus work_offset."""
    _fields_ = ActionWaypointProblem._fields_[:4] + [('work_offset', ctypes.c_int64)] + ActionWaypointProblem._fields_[4:]


ACTION_PROBLEM = np.dtype(ActionWaypointProblem)
ACTION_LARGE_PROBLEM = np.dtype(ActionWaypointLargeProblem)


def large_work_bytes(box_rows, box_cols):
    """simq_action_waypoints_large_work_bytes of include/simq.h restated: simq_grid_paths_large's state -- fp32 distances, one-byte
    parents and flags over the window plus its halo, a ring of window cells + 1 32-bit entries, rounded up to 16."""
    cells = (box_rows + 2) * (box_cols + 2)
    return (6 * cells + 4 * (box_rows * box_cols + 1) + 15) // 16 * 16


def split_by_window(boxes):
    """(fit, over): the problems whose window (i0, j0, rows, cols) plus its halo has at most MAX_BOX_CELLS cells --
    simq_action_waypoints takes them, its search state in LDS -- and the others, for simq_action_waypoints_large; both ascending."""
    fit = [p for p, b in enumerate(boxes) if (int(b[2]) + 2) * (int(b[3]) + 2) <= MAX_BOX_CELLS]
    over = [p for p, b in enumerate(boxes) if (int(b[2]) + 2) * (int(b[3]) + 2) > MAX_BOX_CELLS]
    return fit, over


def entry_calls(n_fit, n):
    """The entry points a call over n problems makes when the first n_fit fit the LDS cap: [(name, first, last + 1)], an empty part
    left out."""
    return [c for c in (('simq_action_waypoints', 0, n_fit), ('simq_action_waypoints_large', n_fit, n)) if c[2] > c[1]]


def _check_large_windows(large_windows):
    if not isinstance(large_windows, bool):
        raise ValueError('large_windows must be True or False, got %r' % (large_windows,))
    return large_windows


def launch_order(problems, large_windows):
    """(order, n_fit) of an ACTION_PROBLEM table: the problems in the order they are launched -- with large_windows those over the LDS
    cap behind the others, for simq_action_waypoints_large; without it all as they come, for simq_action_waypoints to take or refuse."""
    if not large_windows:
        return np.arange(len(problems)), len(problems)
    fit, over = split_by_window(np.stack([problems[n] for n in ('box_i0', 'box_j0', 'box_rows', 'box_cols')], axis=1).tolist())
    return np.asarray(fit + over, np.int64), len(fit)


#: replaces the device when set: callable(problems: ACTION_PROBLEM table) -> (status int32 [P], counts int32 [P], endpoints int32
#: [P, 4], waypoint pixels int32 [sum of the counts of the traced problems, 2]); the tests pin the host arithmetic through it without
#: a device (WaypointGraph.search is the precedent)
search = None

_TABLE = []


def action_table():
    """(dist, angle) float64 [96, 96] of every action pixel: dist = sqrt(dx**2 + dy**2) and atan2(-dx, dy) with (dx, dy) =
    pixel_indices_to_position(row, col, (96, 96)) (envs.py:865-867), built once with `math`."""
    if not _TABLE:
        dist, angle = np.empty((WIDTH, WIDTH)), np.empty((WIDTH, WIDTH))
        for row in range(WIDTH):
            dy = (WIDTH / 2 - (row + 0.5)) / PIXELS_PER_METER
            for col in range(WIDTH):
                dx = ((col + 0.5) - WIDTH / 2) / PIXELS_PER_METER
                dist[row, col], angle[row, col] = math.sqrt(dx**2 + dy**2), math.atan2(-dx, dy)
        _TABLE.extend((dist, angle))
    return _TABLE


def restrict_heading_range_many(h):
    """restrict_heading_range (envs.py:2566-2567) of every entry of a float64 array, the `%` Python's."""
    return np.asarray([x % TWO_PI for x in (h + math.pi).tolist()], np.float64) - math.pi


def headings_between(a, b):
    """restrict_heading_range(atan2(b.y - a.y, b.x - a.x)) for the rows of two float64 arrays [n, 2] (envs.py:882-884)."""
    dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    return restrict_heading_range_many(np.asarray([math.atan2(y, x) for y, x in zip(dy.tolist(), dx.tolist())], np.float64))


class NewActions:
    """What store_new_action leaves in P robots, as arrays: action int64 [P, 3], target_end_effector_position float64 [P, 2] (z is 0),
    waypoint_positions float64 [W, 2] -- all robots' waypoints one behind the other, robot p's at offsets[p]:offsets[p + 1] (int64
    [P + 1]); with `offsets` the packed form RobotArrays(intention_path=...) takes --, waypoint_headings float64 [W], status int32 [P]:
    the device status (TRACED / STRAIGHT; STRAIGHT for every robot when nothing was searched)."""

    def __init__(self, action, target_end_effector_position, waypoint_positions, offsets, waypoint_headings, status, positions=None):
        self.action, self.target_end_effector_position = action, target_end_effector_position
        self.waypoint_positions, self.offsets, self.waypoint_headings, self.status = waypoint_positions, offsets, waypoint_headings, status
        self._positions = positions

    def __len__(self):
        return len(self.action)

    def as_lists(self):
        """Per robot the reference's four attributes (action, target_end_effector_position, waypoint_positions, waypoint_headings): a
        tuple of three ints, a 3-tuple ending in the int 0, a list of 3-tuples whose first element is the position as given (the
        row of the positions array as a tuple when none was given as a sequence), a list of floats."""
        actions, targets = self.action.tolist(), self.target_end_effector_position.tolist()
        ways, headings, off = self.waypoint_positions.tolist(), self.waypoint_headings.tolist(), self.offsets.tolist()
        out = []
        for p in range(len(actions)):
            path = [(x, y, 0) for x, y in ways[off[p]:off[p + 1]]]
            if self._positions is not None:
                path[0] = self._positions[p]
            out.append((tuple(actions[p]), (targets[p][0], targets[p][1], 0), path, headings[off[p]:off[p + 1]]))
        return out


def constants_of(robot_types):
    """(NUM_OUTPUT_CHANNELS int64 [P], END_EFFECTOR_LOCATION + CUBE_WIDTH / 2 float64 [P]) of a list of robot types."""
    return (np.asarray([arch.get_num_output_channels(t) for t in robot_types], np.int64),
            np.asarray([arch.get_end_effector_location(t) + arch.CUBE_WIDTH / 2 for t in robot_types], np.float64))


def _targets(actions, positions, headings, channels):
    """Steps 1 and 2 of the rule: (action int64 [P, 3], target float64 [P, 2]).  channels: every robot's NUM_OUTPUT_CHANNELS."""
    bad = np.flatnonzero((actions < 0) | (actions >= channels * (WIDTH * WIDTH)))
    if bad.size:
        raise ValueError('action %d of robot %d is outside [0, %d * %d * %d)' % (actions[bad[0]], bad[0], channels[bad[0]], WIDTH, WIDTH))
    action = np.stack(np.unravel_index(actions, (2, WIDTH, WIDTH)), axis=1).astype(np.int64)       # (the channel count changes no index)
    dist, angle = action_table()
    dist, theta = dist[action[:, 1], action[:, 2]], headings + angle[action[:, 1], action[:, 2]]
    cos, sin = (np.asarray([f(t) for t in theta.tolist()], np.float64) for f in (math.cos, math.sin))
    return action, np.stack([positions[:, 0] + dist * cos, positions[:, 1] + dist * sin], axis=1)


def _finish(action, positions, headings, targets, reach, status, counts, pixels, rows, cols, given):
    """Steps 3 (from the waypoint pixels on) to 6.  reach: every robot's END_EFFECTOR_LOCATION + CUBE_WIDTH / 2; counts: the waypoints
    the device found per robot (0 when its line is clear or nothing was searched); pixels: int [sum(counts), 2] one robot behind the
    other; rows, cols: every robot's map shape."""
    traced = counts >= 2                                         # fewer than two waypoints: the two positions alone (envs.py:2498-2499)
    n = np.where(traced, counts, 2).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    first, last = offsets[:-1], offsets[1:] - 1
    way = np.empty((int(offsets[-1]), 2), np.float64)
    if traced.any():
        src = ragged(_starts(counts.astype(np.int64))[traced], counts[traced])
        dst = ragged(first[traced], counts[traced])
        of = np.repeat(np.flatnonzero(traced), counts[traced])
        way[dst, 0] = ((pixels[src, 1] + 0.5) - cols[of] / 2) / PIXELS_PER_METER          # Mapper.pixel_indices_to_position
        way[dst, 1] = (rows[of] / 2 - (pixels[src, 0] + 0.5)) / PIXELS_PER_METER
    way[first], way[last] = positions, targets
    heading = np.empty(len(way), np.float64)
    later = np.ones(len(way), bool)
    later[first] = False
    later = np.flatnonzero(later)
    heading[first] = headings
    heading[later] = headings_between(way[later - 1], way[later])
    signed = distances(way[last, 0] - way[last - 1, 0], way[last, 1] - way[last - 1, 1]) - reach
    cos, sin = (np.asarray([f(h) for h in heading[last].tolist()], np.float64) for f in (math.cos, math.sin))
    way[last] = np.stack([way[last - 1, 0] + signed * cos, way[last - 1, 1] + signed * sin], axis=1)
    back = np.flatnonzero((n > 2) & (signed < 0))                # no backing up to the last waypoint (envs.py:898-902)
    if back.size:
        way[last[back] - 1] = way[last[back]]
        heading[last[back] - 1] = headings_between(way[last[back] - 2], way[last[back] - 1])
    return NewActions(action, targets, way, offsets, heading, status.astype(np.int32), given)


def _as_inputs(positions, headings, actions, robot_types):
    """The per-robot inputs as arrays, and the positions as they were given when they came as a sequence of tuples."""
    given = None
    if not isinstance(positions, np.ndarray):
        given = list(positions)
        positions = np.asarray([(p[0], p[1]) for p in given], np.float64).reshape(-1, 2)
    if positions.dtype != np.float64 or positions.ndim != 2 or positions.shape[1] not in (2, 3):
        raise ValueError('positions must be float64 [P, 2] (or P tuples (x, y[, z])), got %s %s' % (positions.dtype, positions.shape))
    positions = positions[:, :2]
    P = len(positions)
    headings = np.asarray(headings)
    actions = np.asarray(actions)
    robot_types = [robot_types] * P if isinstance(robot_types, str) else [str(t) for t in robot_types]
    if P < 1 or headings.shape != (P,) or headings.dtype != np.float64:
        raise ValueError('headings must be float64 [%d], one per position (at least one), got %s %s' % (P, headings.dtype, headings.shape))
    if actions.shape != (P,) or actions.dtype.kind not in 'iu':
        raise ValueError('actions must be %d integers, one per position, got %s %s' % (P, actions.dtype, actions.shape))
    if len(robot_types) != P or any(t not in arch.ROBOT_BASE_LENGTH for t in robot_types):
        raise ValueError('robot_types must name one of %s for each of the %d robots, got %s' % (sorted(arch.ROBOT_BASE_LENGTH), P, robot_types[:8]))
    return positions, headings, actions.astype(np.int64), robot_types, given


def free_box(grid):
    """(i0, j0, rows, cols) of the bounding box of the nonzero cells of a host grid, (0, 0, 0, 0) when there is none."""
    ii, jj = np.nonzero(grid)
    if ii.size == 0:
        return 0, 0, 0, 0
    return int(ii.min()), int(jj.min()), int(ii.max() - ii.min() + 1), int(jj.max() - jj.min() + 1)


def run_problems(problems, bases, upstream=None, capacity=WAY_CAPACITY, what='store_new_actions', large_windows=False, work=None):
    """The device side of a call: one simq_action_waypoints over the ACTION_PROBLEM table `problems` (way_offset and way_capacity are
    set here), one read-back of status words, counts, end pixels, waypoints and the upstream words, and one more round for the
    problems whose waypoints did not fit `capacity` pairs.  bases: (cspace, thin or None, closest or None) flat device tensors.
    large_windows: the problems whose window is over the LDS cap go to simq_action_waypoints_large, queued behind the launch of the
    others and before the one read-back; both write their own problems' ranges of the same buffers, and the second round works over
    both parts in the same way.  work: (uint8 device tensor, int64 byte offset of each problem's search state in it) for the large
    part; omitted, a workspace is allocated per launch.
    Returns (status, counts, endpoints [P, 4], pixels [sum(counts), 2], words) as host arrays: counts is 0 for every problem that was
    not traced, status 3 does not come back, and words holds every problem's upstream word (0 without one) -- a passed-on word is told
    from the entry's own codes by it (include/simq.h)."""
    if search is not None:
        return tuple(search(problems)) + (np.zeros(len(problems), np.int32),)
    cspace, thin, closest = bases
    dev = cspace.device

    def launch(probs, cap, up, work):
        P = len(probs)
        probs['way_capacity'] = cap
        order, n_fit = launch_order(probs, large_windows)            # (the launches in this order; the results back in the problems')
        probs['way_offset'][order] = _starts(probs['way_capacity'][order].astype(np.int64))
        pairs = int(probs['way_capacity'].sum())
        n_up = 0 if up is None else up.numel()
        base = 6 * P + n_up
        base += base % 2                                             # the waypoints start on an 8-byte boundary
        small = torch.empty(base + 2 * pairs, dtype=torch.int32, device=dev)          # status | counts | end pixels | upstream | waypoints
        for name, a, b in entry_calls(n_fit, P):
            extra = ()
            table, struct = np.ascontiguousarray(probs[order[a:b]]), ActionWaypointProblem
            if name == 'simq_action_waypoints_large':
                small_table, table, struct = table, np.zeros(b - a, ACTION_LARGE_PROBLEM), ActionWaypointLargeProblem
                for field in ACTION_PROBLEM.names:
                    table[field] = small_table[field]
                if work is None:
                    need = [large_work_bytes(int(r), int(c)) for r, c in zip(table['box_rows'], table['box_cols'])]
                    table['work_offset'] = _starts(np.asarray(need, np.int64))
                    space = torch.empty(int(sum(need)), dtype=torch.uint8, device=dev)
                else:
                    space, table['work_offset'] = work[0], np.asarray(work[1], np.int64)[order[a:b]]
                extra = (ptr(space), ctypes.c_int64(space.numel()))
            d_probs = torch.empty(table.nbytes, dtype=torch.uint8, device=dev)
            lib.call(name, ptr(cspace), ctypes.c_int64(cspace.numel()), ptr(thin), ctypes.c_int64(0 if thin is None else thin.numel()),
                     ptr(closest), ctypes.c_int64(0 if closest is None else closest.numel()), as_ctypes(table, struct), b - a,
                     ptr(d_probs), ptr(small[base:]), ctypes.c_int64(pairs), ptr(small[P + a:P + b]), ptr(small[2 * P + 4 * a:2 * P + 4 * b]),
                     ptr(up), n_up, ptr(small[a:b]), *extra, stream_ptr(dev))
        if n_up:
            small[6 * P:6 * P + n_up].copy_(up)
        host = small.cpu().numpy()                                    # the one read-back of the round
        back = np.argsort(order)
        return (host[:P][back], host[P:2 * P][back], host[2 * P:6 * P].reshape(P, 4)[back], host[base:].reshape(-1, 2),
                host[6 * P:6 * P + n_up])

    probs = np.ascontiguousarray(problems)
    status, counts, ends, ways, up = launch(probs, capacity, upstream, work)
    words = np.where(probs['upstream'] >= 0, up[np.maximum(probs['upstream'], 0)], 0).astype(np.int32) if len(up) else np.zeros(len(probs), np.int32)
    counts = np.where(((status == TRACED) | (status == CAPACITY)) & (words == 0), counts, 0)          # (nothing is counted for any other status)
    at = _starts(counts.astype(np.int64))
    pixels = np.empty((int(counts.sum()), 2), np.int32)
    whole = np.where(status == TRACED, counts, 0)
    pixels[ragged(at, whole)] = ways[ragged(probs['way_offset'], whole)]
    short = np.flatnonzero((status == CAPACITY) & (words == 0))
    if short.size:                                               # buffers that hold every waypoint, once; the pixels the search used
        again = probs[short].copy()
        again['src_i'], again['src_j'], again['tgt_i'], again['tgt_j'] = ends[short].T
        again['thin_offset'] = again['closest_offset'] = again['upstream'] = -1
        status2, counts2, _, ways2, _ = launch(again, counts[short], None, None if work is None else (work[0], np.asarray(work[1])[short]))
        if (status2 != TRACED).any() or (counts2 != counts[short]).any():
            raise SimqError('%s: the second round of simq_action_waypoints ended with status %s and counts %s for %s'
                            % (what, status2[:8].tolist(), counts2[:8].tolist(), counts[short][:8].tolist()))
        status[short] = TRACED
        pixels[ragged(at[short], counts[short])] = ways2[ragged(again['way_offset'], counts[short])]
    return status, counts, ends, pixels, words


def store_new_actions(cspace, cspace_thin, closest, positions, headings, actions, robot_types, map_index=None,
                      use_shortest_path_movement=True, upstream=None, window=None, large_windows=False):
    """Robot.store_new_action for P robots on loose tensors: the maps simq.occupancy_maps returned (cspace, cspace_thin: M uint8 maps
    each as one [M, rows, cols] tensor or a list; closest: M int32 [2, rows, cols]), positions float64 [P, 2] (or P tuples), headings
    float64 [P], actions P integers, robot_types P names (or one for all); map_index: the map of each robot (robot p uses map p when
    omitted).  upstream: an int32 device tensor with one word per map, e.g. the status words of simq.occupancy_maps: a robot whose
    map's word is not 0 is not searched and is reported.  window: (i0, j0, rows, cols) per map, or one for all, that holds every free
    cell of the configuration space; omitted, host maps are measured on the host and device maps once each on the device (the
    reduction and read-back BatchedMapper.store_new_actions does without).  large_windows: a window of more than MAX_BOX_CELLS cells
    with its halo is refused (SimqError, nothing launched) unless this is True; then those robots go to simq_action_waypoints_large,
    whose search state lies in a workspace in device memory allocated here, the others to simq_action_waypoints as before, with the
    one read-back behind both.  Returns NewActions."""
    _check_large_windows(large_windows)
    positions, headings, actions, robot_types, given = _as_inputs(positions, headings, actions, robot_types)
    P = len(positions)
    channels, reach = constants_of(robot_types)
    action, targets = _targets(actions, positions, headings, channels)
    if not use_shortest_path_movement:
        z = np.zeros(P, np.int64)
        return _finish(action, positions, headings, targets, reach, np.full(P, STRAIGHT), z, np.zeros((0, 2), np.int64), z, z, given)
    from .waypoints import _boxes, _check_closest
    maps, _ = _batch.as_maps(cspace, 'cspace')
    thins, _ = _batch.as_maps(cspace_thin, 'cspace_thin')
    closests, _ = _batch.as_maps(closest, 'closest', _check_closest)
    M = len(maps)
    if len(thins) != M or len(closests) != M:
        raise ValueError('%d configuration spaces, %d thin maps and %d closest blocks (one each per map)' % (M, len(thins), len(closests)))
    map_index = _batch.problem_index(map_index, M, P, '%d maps but %d robots (map_index shares maps between robots)' % (M, P),
                                     'map_index must name one of the %d maps for each of the %d robots' % (M, P))
    used = sorted(set(map_index))
    for k in used:
        if tuple(thins[k].shape) != tuple(maps[k].shape) or tuple(closests[k].shape) != (2,) + tuple(maps[k].shape):
            raise ValueError('map %d: cspace %s, cspace_thin %s, closest %s' % (k, tuple(maps[k].shape), tuple(thins[k].shape), tuple(closests[k].shape)))
    if window is not None:
        window = [tuple(int(x) for x in window)] * M if np.ndim(window) == 1 else [tuple(int(x) for x in w) for w in window]
        if len(window) != M or any(len(w) != 4 for w in window):
            raise ValueError('window is (i0, j0, rows, cols), one for all maps or one per map (%d)' % M)
    if upstream is not None and not (isinstance(upstream, torch.Tensor) and upstream.dtype == torch.int32 and tuple(upstream.shape) == (M,)
                                     and upstream.is_contiguous()):
        raise ValueError('upstream must be a contiguous int32 device tensor with one word per map (%d)' % M)
    rows = np.asarray([maps[k].shape[0] for k in map_index], np.int32)
    cols = np.asarray([maps[k].shape[1] for k in map_index], np.int32)
    src = pixel_indices_many(positions[:, 0], positions[:, 1], (rows, cols))
    tgt = pixel_indices_many(targets[:, 0], targets[:, 1], (rows, cols))
    probs = np.zeros(P, ACTION_PROBLEM)
    probs['rows'], probs['cols'], probs['src_i'], probs['src_j'], probs['tgt_i'], probs['tgt_j'] = rows, cols, src[0], src[1], tgt[0], tgt[1]
    bases = None
    if search is None:
        dev = _batch.device('new actions')
        if upstream is not None and upstream.device != dev:
            raise ValueError('upstream must be a contiguous int32 device tensor with one word per map (%d) on %s' % (M, dev))
        packed, offsets = _batch.pack([maps[k] for k in used], torch.uint8, dev, align=16)
        packed_thin, _ = _batch.pack([thins[k] for k in used], torch.uint8, dev, align=16)
        packed_closest, closest_offsets = _batch.pack([closests[k] for k in used], torch.int32, dev, align=16)
        at, closest_at = dict(zip(used, offsets)), dict(zip(used, closest_offsets))
        probs['cspace_offset'] = probs['thin_offset'] = [at[k] for k in map_index]
        probs['closest_offset'] = [closest_at[k] for k in map_index]
        bases = (packed, packed_thin, packed_closest)
        if window is None:
            boxes = _boxes(maps, used, dev)
            window = [boxes.get(k, (0, 0, 0, 0)) for k in range(M)]
    elif window is None:
        window = [free_box(maps[k]) if k in used else (0, 0, 0, 0) for k in range(M)]
    box = np.asarray([window[k] for k in map_index], np.int32).reshape(P, 4)
    probs['box_i0'], probs['box_j0'], probs['box_rows'], probs['box_cols'] = box.T
    over = np.flatnonzero((box[:, 2].astype(np.int64) + 2) * (box[:, 3] + 2) > MAX_BOX_CELLS)
    if over.size and not large_windows:
        raise SimqError('store_new_actions: the window of map %d is %d x %d cells, with its halo over SIMQ_GRID_PATH_MAX_BOX_CELLS = %d'
                        % (map_index[over[0]], box[over[0], 2], box[over[0], 3], MAX_BOX_CELLS))
    probs['upstream'] = map_index if upstream is not None else -1
    status, counts, _, pixels, words = run_problems(probs, bases, upstream, **({'large_windows': True} if large_windows else {}))
    bad = np.flatnonzero((words != 0) | ((status != TRACED) & (status != STRAIGHT)))
    codes = status[bad]
    if bad.size:
        raise SimqError('store_new_actions: %d robot(s) failed (status %s at robots %s; 2: a bad pixel, snapped pixel or window, 4: a loop '
                        'bound, other: the upstream word of the map)' % (bad.size, codes[:8].tolist(), bad[:8].tolist()))
    return _finish(action, positions, headings, targets, reach, status, counts, pixels, rows, cols, given)
