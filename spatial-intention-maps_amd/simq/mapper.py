"""The Mapper of every robot of many environments as one object on the GPU: ``Mapper.update`` and ``Mapper.get_state`` in batches.

The reference gives every robot its own ``Mapper`` (envs.py:2009-2406) and every Mapper its ``OccupancyMap`` (envs.py:2408-2554); after
each environment step it calls ``update`` and ``get_state`` on them one by one, on the host.  ``BatchedMapper`` stands for all those
pairs of E environments: a *mapper* m is one (environment, robot) pair, the maps of all M mappers are rows of device tensors this
object owns, and the two calls run the batched operators of this package as one chain on them:

    update       simq_observation_update  ->  simq_occupancy_maps                                     (envs.py:2053-2065, 2444-2459)
    get_states   simq_grid_distance_images_snapped  ->  simq_intention_maps  ->  simq_local_state_images     (envs.py:2067-2112)
    defer ...    nothing: the frames of any number of update calls wait in pinned memory, per mapper in capture order
    flush        simq_observation_update_sequences  ->  simq_occupancy_maps      (what those update calls would have left)

Each stage is one launch however many mappers are named, reads the tensors of the stage before it where they lie, and leaves its
status words on the device; the call reads them back once, at its end.  What lets the read-back wait is the upstream status of
the snapped distance images (include/simq.h): a mapper whose configuration space has no free cell -- its closest cells are undefined
-- is not searched.  ``store_new_actions`` is Robot.store_new_action for the deciding robots: one simq_action_waypoints launch on the same
tensors, the float64 arithmetic on the host.  Douglas-Peucker by scikit-image stays on the host (section 13).
simq_occupancy_maps and simq_action_waypoints keep their state in LDS, which bounds a room (a padded map of 256 cells a side, a
room-mask box of 20 000 cells with its halo); with large_rooms=True the mappers over a bound go to simq_occupancy_maps_large and
simq_action_waypoints_large, the same kernels with that state in workspaces of this object's in device memory (section 24).
"""
import collections
import collections.abc
import ctypes
import math

import numpy as np
import torch

from . import _batch, arch, grid_paths, intention_drawing, local_maps, observation, occupancy
from ._lib import SimqError, lib, ptr, stream_ptr

FLAGS = ('use_robot_map', 'use_distance_to_receptacle_map', 'use_shortest_path_to_receptacle_map', 'use_shortest_path_map', 'use_history_map',
         'use_intention_map', 'use_intention_channels')
CHANNEL_ENCODINGS = ('spatial', 'nonspatial')
WITH_CUBE = 'lifting_robot_with_cube'                   # the key of envs.py:2037
NOT_UPDATED = 4                                        # occupancy status of a mapper that had no update since construction / reset

# What Mapper.get_state reads of one robot (envs.py:2199-2203, 2250-2270, 2303-2317, 2350-2373): get_position(), get_heading(), the
# class, lift_state (LiftingRobot), is_idle(), target_end_effector_position, controller.get_intention_path() / get_history_path().
# An idle robot needs no target and no paths; the paths are read only by the encodings that draw them.
RobotState = collections.namedtuple('RobotState', ('position', 'heading', 'robot_type', 'lift_state', 'idle', 'target', 'intention_path',
                                                   'history_path'), defaults=(None, False, None, None, None))


def _array(value, what, dtype, shape):
    """`value` as it is when it is an ndarray of `dtype` and `shape` (None: any length); nothing is converted."""
    if not isinstance(value, np.ndarray) or value.dtype != dtype or value.ndim != len(shape) or \
            any(s is not None and n != s for n, s in zip(value.shape, shape)):
        raise ValueError('RobotArrays.%s must be a %s array of shape [%s], got %s' % (
            what, np.dtype(dtype).name, ', '.join('M' if s is None else str(s) for s in shape),
            '%s %s' % (value.dtype, list(value.shape)) if isinstance(value, np.ndarray) else type(value).__name__))
    return value


class RobotArrays:
    """What RobotState holds of every robot of a BatchedMapper, as arrays indexed by mapper m = env_begin[e] + robot:

    position float64 [M, 2], heading float64 [M], lifting bool [M] (lift_state == 'lifting'; read for lifting robots only), idle bool [M],
    target float64 [M, 2] or None, intention_path / history_path: a pair (points float64 [N, 2], offsets int64 [M + 1]) -- the
    waypoints of mapper m are points[offsets[m]:offsets[m + 1]] -- or None.  lifting and idle may be omitted (nobody lifts, nobody is idle).

    The rows of mappers a call does not read may hold anything; a robot that is not idle and is drawn needs a target without NaN and
    a path of at least one waypoint where the list form needs them.  An array of another type or shape is refused, not converted:
    the list form computes on the values as they are given, and a float32 position would take float32 arithmetic there."""

    def __init__(self, position, heading, lifting=None, idle=None, target=None, intention_path=None, history_path=None):
        self.position = _array(position, 'position', np.float64, (None, 2))
        M = self.num_mappers = len(position)
        self.heading = _array(heading, 'heading', np.float64, (M,))
        self.lifting = np.zeros(M, bool) if lifting is None else _array(lifting, 'lifting', np.bool_, (M,))
        self.idle = np.zeros(M, bool) if idle is None else _array(idle, 'idle', np.bool_, (M,))
        self.target = None if target is None else _array(target, 'target', np.float64, (M, 2))
        self.intention_path = self._path(intention_path, 'intention_path')
        self.history_path = self._path(history_path, 'history_path')

    def _path(self, path, what):
        if path is None:
            return None
        try:
            points, offsets = path
        except (TypeError, ValueError):
            raise ValueError('RobotArrays.%s is a pair (points, offsets) or None' % what) from None
        points = _array(points, what + ' points', np.float64, (None, 2))
        offsets = _array(offsets, what + ' offsets', np.int64, (self.num_mappers + 1,))
        if offsets[0] != 0 or offsets[-1] != len(points) or (np.diff(offsets) < 0).any():
            raise ValueError('RobotArrays.%s offsets must rise from 0 to the number of points (%d) without falling, got %s%s'
                             % (what, len(points), offsets[:8].tolist(), ' ...' if len(offsets) > 8 else ''))
        return points, offsets

    @classmethod
    def from_states(cls, mapper, robots):
        """The list form of `mapper.get_states` as arrays: robots holds per environment the RobotState of each robot, or None for an
        environment no call will read (its rows are NaN).  Coordinates and headings are taken as Python floats or np.float64 only.  A
        robot without a target gets a row of NaN, a robot without a path an empty one; a field no robot has is None."""
        M = mapper.num_mappers
        states = mapper._robots(robots, [e for e in range(min(len(robots), mapper.num_envs)) if robots[e] is not None])

        def number(v, what):
            if type(v) not in (float, np.float64):
                raise ValueError('RobotArrays.from_states takes Python floats and np.float64, got %s as %s' % (type(v).__name__, what))
            return v
        position, heading = np.full((M, 2), np.nan), np.full(M, np.nan)
        lifting, idle, target = np.zeros(M, bool), np.zeros(M, bool), np.full((M, 2), np.nan)
        paths = {'intention_path': [[] for _ in range(M)], 'history_path': [[] for _ in range(M)]}
        given = set()
        for e, env in states.items():
            for k, r in enumerate(env):
                m = mapper.env_begin[e] + k
                position[m] = number(r.position[0], 'position'), number(r.position[1], 'position')
                heading[m] = number(r.heading, 'heading')
                lifting[m], idle[m] = r.lift_state == 'lifting', bool(r.idle)
                if r.target is not None:
                    target[m] = number(r.target[0], 'target'), number(r.target[1], 'target')
                    given.add('target')
                for name, rows in paths.items():
                    if getattr(r, name) is not None:
                        rows[m] = [(number(w[0], name), number(w[1], name)) for w in getattr(r, name)]
                        given.add(name)

        def packed(rows):
            offsets = np.concatenate([[0], np.cumsum([len(row) for row in rows])]).astype(np.int64)
            return np.array([w for row in rows for w in row], np.float64).reshape(-1, 2), offsets
        return cls(position, heading, lifting, idle, target if 'target' in given else None,
                   *[packed(paths[name]) if name in given else None for name in ('intention_path', 'history_path')])


class _StageMaps(collections.abc.Mapping):
    """BatchedMapper.stage_maps after an array-form call: the same keys and tensors as the dict of the list form, each view formed
    when it is asked for.  where: {key: (buffer name, index)}; buffers: {name: tensor [n, rows, cols], or (flat tensor, offsets, shapes)}."""

    def __init__(self, where, buffers):
        self._where, self._buffers = where, buffers

    def __getitem__(self, key):
        name, k = self._where[key]
        held = self._buffers[name]
        if isinstance(held, tuple):
            flat, offsets, shapes = held
            return flat[offsets[k]:offsets[k] + shapes[k][0] * shapes[k][1]].view(shapes[k])
        return held[k]

    def __iter__(self):
        return iter(self._where)

    def __len__(self):
        return len(self._where)


def closest_order(positions, me, own):
    """The other robots of P environments of R robots from the closest to the furthest, as envs.py:2350-2358 orders them: int [P, R - 1]
    for positions float64 [P, R, 2], the observers' positions me [P, 2] and their indices own [P].  np.argsort sorts each row as it
    sorts the list of the list form, so robots at equal distances fall as they do there."""
    order = np.argsort(local_maps.distances(positions[:, :, 0] - me[:, None, 0], positions[:, :, 1] - me[:, None, 1]))
    return order[order != np.asarray(own)[:, None]].reshape(len(order), -1)


class _Plan:
    """What get_states' array form needs of one `mappers` tuple and of the object, but of no call: index arrays, and the descriptor
    tables with every field filled that no robot's state changes (a call copies a table and fills the rest).  The order of robots,
    maps, problems and channels is the one the list form arrives at through local_maps._prepare and intention_drawing._prepare."""

    def __init__(self, bm, ms):
        self.stage_keys = {}                                         # BatchedMapper.stage_maps' key: (buffer, index in it)
        self._index(bm, ms)
        self._described_robots(bm)
        slots = self._map_slots(bm)
        self._stage1(bm, slots)
        self._stage2(bm, slots)
        self._stage3(bm, slots)
        self._fixed = None

    def _index(self, bm, ms):
        """Of every named mapper p its environment, its robot, its room shape and where its maps lie; the pairs (p, another robot of
        p's environment), p by p in env.robots' order: whom p's maps draw."""
        starts, f = intention_drawing._starts, bm.flags
        self.ms = np.asarray(ms, np.int64)
        P = self.P = len(ms)
        self.env_begin = env_begin = np.asarray(bm.env_begin, np.int64)
        self.env = env = np.asarray(bm.env_of, np.int64)[self.ms]
        self.robot = self.ms - env_begin[env]
        self.rows_of, self.cols_of = (np.asarray([s[k] for s in bm.shapes], np.int32) for k in (0, 1))
        self.rows, self.cols = self.rows_of[self.ms], self.cols_of[self.ms]
        cells = self.rows_of.astype(np.int64) * self.cols_of
        self._at = np.concatenate([starts(cells), [cells.sum()]])     # cell offset of every mapper's maps (BatchedMapper._at)
        others = env_begin[env + 1] - env_begin[env] - 1
        self.pair_p = np.repeat(np.arange(P), others)
        rank = np.arange(int(others.sum())) - np.repeat(starts(others), others)
        self.others = env_begin[env][self.pair_p] + rank + (rank >= self.robot[self.pair_p])
        self.R = self.env_rows = None
        if f['use_intention_channels']:
            self.R = len(bm.robot_types[0])
            self.env_rows = env_begin[env][:, None] + np.arange(self.R)
        self.spatial = f['use_intention_channels'] and bm.intention_channel_encoding == 'spatial'

    def _described_robots(self, bm):
        """The robots as stage 3 has them described -- every environment once, in the order in which `ms` comes to it -- and the
        problems of stage 3 with each one's range of them."""
        env, env_begin = self.env, self.env_begin
        first = list(dict.fromkeys(env.tolist()))
        begin = dict(zip(first, intention_drawing._starts(np.asarray([len(bm.robot_types[e]) for e in first], np.int64)).tolist()))
        self.robots = np.concatenate([np.arange(env_begin[e], env_begin[e + 1]) for e in first])
        self.robot_rows, self.robot_cols = self.rows_of[self.robots], self.cols_of[self.robots]
        robot_begin = np.asarray([begin[e] for e in env.tolist()], np.int64)
        self.own_row = robot_begin + self.robot
        types = [t for e in first for t in bm.robot_types[e]]
        self.stamps = np.zeros(len(self.robots), local_maps.LOCAL_ROBOT)
        self.stamps['seg_mask'] = [bm.mask_index[t] for t in types]
        self.stamps['seg_value'] = [bm.seg_values['robot_group_%d' % (g + 1)] for e in first for g in bm.group_indices[e]]
        self.lifters = np.asarray([t == 'lifting_robot' for t in types])
        self.cube_mask = bm.mask_index.get(WITH_CUBE, 0)
        self.problems = np.zeros(self.P, local_maps.LOCAL_PROBLEM)
        self.problems['rows'], self.problems['cols'], self.problems['robot_begin'] = self.rows, self.cols, robot_begin
        self.problems['robot_count'] = env_begin[env + 1] - env_begin[env]

    def _map_slots(self, bm):
        """The maps of stage 3 in the order of their first use: p by p its overhead map, the receptacle map where p is the first to use
        it, its distance images, its drawn maps.  Returns where in that table each kind lies: {'overhead', 'receptacle', 'history',
        'intention': [P], 'images': nd arrays [P], 'channels': [P, nq]}, None for a kind the configuration does not have."""
        f, P = bm.flags, self.P
        nd = int(f['use_shortest_path_to_receptacle_map']) + int(f['use_shortest_path_map'])
        nq = self.R - 1 if self.spatial else 0
        new = np.zeros(P, np.int64)
        first_user = np.zeros(P, np.int64)
        if f['use_distance_to_receptacle_map']:
            seen = {}
            for p, e in enumerate(self.env.tolist()):
                first_user[p] = seen.setdefault((bm.env_shapes[e], bm.receptacle_positions[e]), p)
            new = (first_user == np.arange(P)).astype(np.int64)
        per = 1 + nd + int(f['use_history_map']) + int(f['use_intention_map']) + nq
        base = intention_drawing._starts(per + new)
        after = base + 1 + new
        drawn = after + nd
        slots = {'overhead': base, 'receptacle': base[first_user] + 1 if f['use_distance_to_receptacle_map'] else None,
                 'images': [after + d for d in range(nd)], 'history': drawn if f['use_history_map'] else None,
                 'intention': drawn + int(f['use_history_map']) if f['use_intention_map'] else None,
                 'channels': (drawn + int(f['use_history_map']) + int(f['use_intention_map']))[:, None] + np.arange(nq)}
        self.overhead_maps, self.receptacle_maps = base, base[first_user] + 1
        self.n_maps = int((per + new).sum())
        self.map_rows, self.map_cols = np.zeros(self.n_maps, np.int32), np.zeros(self.n_maps, np.int32)
        for where in [slots[k] for k in ('overhead', 'receptacle', 'history', 'intention') if slots[k] is not None] + slots['images'] + \
                [slots['channels'][:, q] for q in range(nq)]:
            self.map_rows[where], self.map_cols[where] = self.rows, self.cols
        return slots

    def _stage1(self, bm, slots):
        """Stage 1: the problems, receptacle-sourced then robot-sourced, each over `ms`, but for the robot pixels."""
        f, P, at, rows, cols = bm.flags, self.P, self._at, self.rows, self.cols
        nd = len(slots['images'])
        self.grid = None
        if not nd:
            return
        lo, hi = int(self.ms.min()), int(self.ms.max())
        self.grid_lo, self.grid_cells = int(at[lo]), int(at[hi + 1] - at[lo])
        g = self.grid = np.zeros(nd * P, grid_paths.SNAPPED_PROBLEM)
        g['grid_offset'] = np.tile(at[self.ms] - at[lo], nd)
        g['closest_offset'] = 2 * g['grid_offset']
        g['rows'], g['cols'], g['upstream'] = np.tile(rows, nd), np.tile(cols, nd), np.tile(self.ms, nd)
        self.image_at = intention_drawing._starts(g['rows'].astype(np.int64) * g['cols'])
        g['out_offset'] = self.image_at
        self.grid_want = (int((g['rows'].astype(np.int64) * g['cols']).sum()),)
        if f['use_shortest_path_to_receptacle_map']:
            at_receptacle = np.asarray([bm.receptacle_positions[e][:2] for e in self.env.tolist()], np.float64)
            g['src_i'][:P], g['src_j'][:P] = local_maps.pixel_indices_many(at_receptacle[:, 0], at_receptacle[:, 1], (rows, cols))
        self.image_maps = np.concatenate(slots['images'])
        self.image_shapes = [(int(r), int(c)) for r, c in zip(g['rows'], g['cols'])]
        self.stage_keys.update({('image', d, p): ('image', d * P + p) for d in range(nd) for p in range(P)})

    def _stage2(self, bm, slots):
        """Stage 2: per room shape the problems -- history maps, intention maps, the maps behind the spatial channels -- over the p of
        that shape; `pairs`: their rows of `others`; `problem`: for every (problem, drawn robot) its problem; `maps`: where their maps go."""
        nq = slots['channels'].shape[1]
        self.jobs = []
        if slots['history'] is None and slots['intention'] is None and not self.spatial:
            return
        shapes = sorted(set(bm.shapes[m] for m in self.ms.tolist()))
        if bm.one_drawing_launch and len(shapes) > 1:
            # one job over every p: the buffer 'drawn' is flat, each problem with its shape and its offset (simq_intention_maps_shapes)
            shapes = [None]
        for shape in shapes:
            sel = np.arange(self.P) if shape is None else np.flatnonzero((self.rows == shape[0]) & (self.cols == shape[1]))
            pairs = np.flatnonzero(np.isin(self.pair_p, sel))
            of_pair = np.searchsorted(sel, self.pair_p[pairs])
            buffer = 'drawn' if shape is None else shape
            problem, maps, owner, n = [], [], [], 0
            for name in ('history', 'intention'):
                if slots[name] is not None:
                    problem.append(n + of_pair)
                    maps.append(slots[name][sel])
                    owner.append(sel)
                    self.stage_keys.update({(name, int(p)): (buffer, n + k) for k, p in enumerate(sel)})
                    n += len(sel)
            if self.spatial:
                problem.append(n + np.arange(len(sel) * nq))
                maps.append(slots['channels'][sel].reshape(-1))
                owner.append(np.repeat(sel, nq))
                self.stage_keys.update({('channel', int(p), q): (buffer, n + k * nq + q) for k, p in enumerate(sel) for q in range(nq)})
                n += len(sel) * nq
            job = {'p': sel, 'pairs': pairs, 'problem': np.concatenate(problem), 'n': n, 'maps': np.concatenate(maps)}
            if shape is None:                                        # every problem's shape, and where its map begins in the flat tensor
                owner = np.concatenate(owner)
                job['shapes'] = np.stack([self.rows[owner], self.cols[owner]], axis=1).astype(np.int64)
                cells = job['shapes'][:, 0] * job['shapes'][:, 1]
                job['at'], job['cells'] = intention_drawing._starts(cells), int(cells.sum())
                job['shape_list'] = [(int(r), int(c)) for r, c in job['shapes']]
            self.jobs.append((shape, job))

    def _stage3(self, bm, slots):
        """Stage 3: the channels in get_state's order, with every field but the constants of the nonspatial encoding."""
        f, C = bm.flags, bm.num_channels
        columns = [('overhead', slots['overhead'])]
        if f['use_robot_map']:
            columns.append(('robots', 0))
        if slots['receptacle'] is not None:
            columns.append(('distance', slots['receptacle']))
        columns += [('distance', where) for where in slots['images']]
        columns += [('map', slots[name]) for name in ('history', 'intention') if slots[name] is not None]
        if self.spatial:
            columns += [('map', slots['channels'][:, q]) for q in range(slots['channels'].shape[1])]
        elif f['use_intention_channels']:
            columns += [('constant', 0)] * (2 * (self.R - 1))
        assert len(columns) == C, (len(columns), bm.channels)
        table = np.zeros((self.P, C), local_maps.LOCAL_CHANNEL)
        for c, (kind, where) in enumerate(columns):
            table['kind'][:, c], table['map'][:, c] = local_maps.KINDS[kind], where
        self.constant_at = np.flatnonzero(table['kind'].reshape(-1) == local_maps.KINDS['constant'])
        self.channels = table.reshape(-1)

    def on_device(self, bm):
        """The part that holds addresses of the object's tensors: the table of stage 3's maps with every map that outlives a call,
        and where the grids and closest blocks of stage 1 begin."""
        if self._fixed is None:
            maps = np.zeros(self.n_maps, local_maps.LOCAL_MAP)
            maps['rows'], maps['cols'] = self.map_rows, self.map_cols
            maps['d_data'][self.overhead_maps] = bm._overhead.data_ptr() + 4 * self._at[self.ms]
            if bm.distance_to_receptacle_maps is not None:
                maps['d_data'][self.receptacle_maps] = [bm.distance_to_receptacle_maps[e].data_ptr() for e in self.env.tolist()]
            self._fixed = {'maps': maps}
            if self.grid is not None:
                self._fixed.update(grids=bm._cspace.data_ptr() + self.grid_lo, closest=bm._closest.data_ptr() + 8 * self.grid_lo)
        return self._fixed


class _Deferred:
    """One deferred camera frame: px, py, depth and ids as `words` 4-byte words at word `at` of staging block `block`, and its
    descriptor with every field final but the four frame offsets, which count from the frame's first word."""
    __slots__ = ('block', 'at', 'words', 'problem')

    def __init__(self, block, at, words, problem):
        self.block, self.at, self.words, self.problem = block, at, words, problem


class _Staging:
    """The host memory deferred frames wait in: int32 blocks, pinned where there is a device to pin them for, handed out front to back.
    It grows by blocks (each as large as all before it, at least BLOCK_WORDS and the frame that asked) and is never freed: `compact`
    moves what still waits to the front and the rest is reused."""
    BLOCK_WORDS = 1 << 22

    def __init__(self):
        self.tensors, self.arrays, self.used, self.cursor = [], [], [], 0

    def take(self, words):
        """(block, word offset) of `words` free words; the cursor never goes back to an earlier block."""
        while self.cursor < len(self.tensors):
            b = self.cursor
            if self.used[b] + words <= self.arrays[b].size:
                at = self.used[b]
                self.used[b] += words
                return b, at
            self.cursor += 1
        size = max(words, self.BLOCK_WORDS, sum(a.size for a in self.arrays))
        t = torch.empty(size, dtype=torch.int32, pin_memory=torch.cuda.is_available())
        self.tensors.append(t)
        self.arrays.append(t.numpy())
        self.used.append(words)
        return len(self.tensors) - 1, 0

    def compact(self, waiting):
        """Moves the frames `waiting` (_Deferred) to the front, in the order they lie in.  A frame never moves to a later place than
        it has -- the frames before it take no more room than they did -- so no move overwrites a frame that has yet to move.  Only
        for a time when no upload from the blocks is in flight."""
        waiting = sorted(waiting, key=lambda f: (f.block, f.at))
        self.used, self.cursor = [0] * len(self.tensors), 0
        for f in waiting:
            b, at = self.take(f.words)
            if (b, at) != (f.block, f.at):
                self.arrays[b][at:at + f.words] = self.arrays[f.block][f.at:f.at + f.words]
                f.block, f.at = b, at


def round_up_to_even(x):
    """envs.py:2404-2406."""
    return 2 * math.ceil(x / 2)


def padded_room_shape(room_width, room_length):
    """The shape of Mapper.create_padded_room_zeros (envs.py:2382-2388)."""
    return (round_up_to_even(room_width * arch.LOCAL_MAP_PIXELS_PER_METER + math.sqrt(2) * arch.STATE_WIDTH),
            round_up_to_even(room_length * arch.LOCAL_MAP_PIXELS_PER_METER + math.sqrt(2) * arch.STATE_WIDTH))


def room_mask(room_width, room_length):
    """OccupancyMap._create_room_mask (envs.py:2467-2475)."""
    mask = np.zeros(padded_room_shape(room_width, room_length), np.uint8)
    room_length_pixels = round_up_to_even((room_length - 2 * arch.ROBOT_HALF_WIDTH) * arch.LOCAL_MAP_PIXELS_PER_METER)
    room_width_pixels = round_up_to_even((room_width - 2 * arch.ROBOT_HALF_WIDTH) * arch.LOCAL_MAP_PIXELS_PER_METER)
    start_i = int(mask.shape[0] / 2 - room_width_pixels / 2)
    start_j = int(mask.shape[1] / 2 - room_length_pixels / 2)
    mask[start_i:start_i + room_width_pixels, start_j:start_j + room_length_pixels] = 1
    return mask


def distance_to_receptacle_map(shape, receptacle_position, scale):
    """Mapper._create_global_distance_to_receptacle_map (envs.py:2277-2285), pixel by pixel in Python floats as there: the position of
    envs.py:2398-2402, the distance of envs.py:2556-2557, stored as float32, then scaled in place."""
    rows, cols = shape
    ppm = arch.LOCAL_MAP_PIXELS_PER_METER
    global_map = np.zeros(shape, np.float32)
    for i in range(rows):
        pos_y = (rows / 2 - (i + 0.5)) / ppm
        for j in range(cols):
            pos_x = ((j + 0.5) - cols / 2) / ppm
            global_map[i, j] = _distance((pos_x, pos_y), receptacle_position)
    global_map *= scale
    return global_map


def channel_names(flags, intention_channel_encoding='spatial', n_robots=1):
    """The channels of Mapper.get_state in its order (envs.py:2067-2112) for a dict of use_* flags; the intention channels of the
    other robots come closest first (envs.py:2350-2354): one per robot ('spatial') or two ('nonspatial')."""
    names = ['overhead']
    names += [n for f, n in zip(FLAGS[:6], ('robots', 'distance_to_receptacle', 'shortest_path_to_receptacle', 'shortest_path', 'history',
                                            'intention')) if flags.get(f)]
    if flags.get('use_intention_channels'):
        per = 1 if intention_channel_encoding == 'spatial' else 2
        names += ['intention_channel_%d' % k for k in range(per * (n_robots - 1))]
    return names


def _distance(p1, p2):
    return math.sqrt((p2[0] - p1[0])**2 + (p2[1] - p1[1])**2)                              # envs.py:2556-2557


def _per_env(value, E, what, scalar):
    """`value` for each of E environments: one value for all (scalar(value) is true) or a sequence of E."""
    if scalar(value):
        return [value] * E
    values = list(value)
    if len(values) != E:
        raise ValueError('%s is one value or one per environment: %d values for %d environments' % (what, len(values), E))
    return values


def _is_number(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


class BatchedMapper:
    """The Mapper + OccupancyMap pairs of every robot of E environments.

    room_width, room_length: env.room_width, env.room_length -- one value, or one per environment.  robot_types: per environment the
    robots' types in env.robots' order ('pushing_robot', 'lifting_robot', 'throwing_robot', 'rescue_robot'); group_indices: per
    environment each robot's group_index (omitted: 0).  robot_masks: {robot type: float32 [96, 96] mask} plus
    'lifting_robot_with_cube' when a lifting robot is present -- Mapper.robot_masks (envs.py:2031-2037), from
    Mapper._create_robot_mask.  receptacle_position: env.receptacle_position, one (x, y[, z]) or one per environment.  The use_*
    switches (FLAGS) and the remaining keywords are the environment's attributes of the same names; seg_values: Camera.SEG_VALUES.

    Mapper m = (environment e, robot r) has the index `mapper_index(e, r)`: environments in order, robots in env.robots' order.  The
    persistent maps live in one device buffer per kind and are exposed as `overhead` fp32 [M, rows, cols]
    (global_overhead_map_without_robots), `occupancy`, `configuration_space`, `cspace_thin` uint8 [M, rows, cols] and
    `closest_cspace_indices` int32 [M, 2, rows, cols] when every environment has the same room, otherwise as lists of M views
    ([rows_m, cols_m], [2, rows_m, cols_m]) into those buffers.  `occupancy_status` int32 [M] holds the status word of each mapper's
    last configuration space (NOT_UPDATED before the first); `distance_to_receptacle_maps` (use_distance_to_receptacle_map) one
    fp32 [rows, cols] device map per environment (environments of one room and receptacle share it).  `pending` int64 [M] counts the
    frames `defer` holds of each mapper until `flush` applies them.

    large_rooms: without it a room whose padded map has a side over 256 cells is refused by update and flush, and one whose
    room-mask box has more than 20 000 cells with its halo by store_new_actions, both by the library.  With it the constructor decides
    per mapper, from the shapes and the room masks' boxes, which entry point each stage uses (`occupancy_entry`, `action_entry`: one
    name per mapper) and allocates the two workspaces once; update / flush and store_new_actions then make at most two launches per
    stage, the mappers under the caps first, and a set of mappers on both sides of a cap works as one.

    one_drawing_launch: without it get_states draws the history and intention maps with one simq_intention_maps launch per room shape
    among the named mappers.  With it a call whose mappers have more than one room shape draws them all in one
    simq_intention_maps_shapes launch, into one flat tensor, with one descriptor upload; a call whose mappers
    share a shape makes the call it makes without it.  The states are the same either way."""

    def __init__(self, room_width, room_length, robot_types, robot_masks, group_indices=None, receptacle_position=None, *,
                 use_robot_map=True, use_distance_to_receptacle_map=False, use_shortest_path_to_receptacle_map=False,
                 use_shortest_path_map=False, use_history_map=False, use_intention_map=False, use_intention_channels=False,
                 intention_map_encoding='ramp', intention_map_scale=1.0, intention_map_line_thickness=2, intention_channel_encoding='spatial',
                 intention_channel_nonspatial_scale=0.1, distance_to_receptacle_map_scale=0.25, shortest_path_map_scale=0.25, seg_values=None, large_rooms=False,
                 one_drawing_launch=False):
        given = locals()
        if not isinstance(large_rooms, bool):
            raise ValueError('large_rooms must be True or False, got %r' % (large_rooms,))
        self.large_rooms = large_rooms
        if not isinstance(one_drawing_launch, bool):
            raise ValueError('one_drawing_launch must be True or False, got %r' % (one_drawing_launch,))
        self.one_drawing_launch = one_drawing_launch
        self.flags = {f: bool(given[f]) for f in FLAGS}
        try:
            self.robot_types = [[str(t) for t in env] for env in robot_types]
        except TypeError:
            raise ValueError('robot_types holds, per environment, the list of its robots\' types') from None
        if not self.robot_types or any(not env for env in self.robot_types):
            raise ValueError('BatchedMapper needs at least one environment and one robot in each')
        E = self.num_envs = len(self.robot_types)
        for env in self.robot_types:
            for t in env:
                if t not in arch.ROBOT_BASE_LENGTH:
                    raise ValueError('robot type %r: choose from %s' % (t, sorted(arch.ROBOT_BASE_LENGTH)))
        if group_indices is None:
            group_indices = [[0] * len(env) for env in self.robot_types]
        self.group_indices = [[int(g) for g in env] for env in group_indices]
        if [len(env) for env in self.group_indices] != [len(env) for env in self.robot_types]:
            raise ValueError('group_indices must hold one group index for each robot of robot_types: %s robots, %s group indices'
                             % ([len(env) for env in self.robot_types], [len(env) for env in self.group_indices]))
        self.seg_values = dict(arch.SEG_VALUES if seg_values is None else seg_values)
        for env in self.group_indices:
            for g in env:
                if 'robot_group_%d' % (g + 1) not in self.seg_values:
                    raise ValueError('group index %d has no segmentation value robot_group_%d' % (g, g + 1))
        if intention_map_encoding not in intention_drawing.ENCODINGS[:4]:
            raise ValueError('intention_map_encoding %r: choose from %s' % (intention_map_encoding, list(intention_drawing.ENCODINGS[:4])))
        if intention_channel_encoding not in CHANNEL_ENCODINGS:
            raise ValueError('intention_channel_encoding %r: choose from %s' % (intention_channel_encoding, list(CHANNEL_ENCODINGS)))
        self.intention_map_encoding, self.intention_channel_encoding = intention_map_encoding, intention_channel_encoding
        self.intention_map_scale, self.intention_map_line_thickness = intention_map_scale, int(intention_map_line_thickness)
        self.intention_channel_nonspatial_scale = intention_channel_nonspatial_scale
        self.distance_to_receptacle_map_scale, self.shortest_path_map_scale = distance_to_receptacle_map_scale, shortest_path_map_scale
        self.room_widths = [float(w) for w in _per_env(room_width, E, 'room_width', _is_number)]
        self.room_lengths = [float(w) for w in _per_env(room_length, E, 'room_length', _is_number)]
        if self.flags['use_distance_to_receptacle_map'] or self.flags['use_shortest_path_to_receptacle_map']:
            if receptacle_position is None:                                                # envs.py:2050-2051
                raise ValueError('use_distance_to_receptacle_map and use_shortest_path_to_receptacle_map need receptacle_position')
            if any(t == 'rescue_robot' for env in self.robot_types for t in env):         # envs.py:2047-2049
                raise ValueError('an environment with a rescue robot has no receptacle maps')
        self.receptacle_positions = [None] * E
        if receptacle_position is not None:
            self.receptacle_positions = [tuple(float(x) for x in p) for p in
                                         _per_env(receptacle_position, E, 'receptacle_position', lambda v: _is_number(v[0]))]
        if self.flags['use_intention_channels'] and len(set(len(env) for env in self.robot_types)) != 1:
            raise ValueError('use_intention_channels gives one channel set per other robot: every environment needs the same number of '
                             'robots, got %s' % [len(env) for env in self.robot_types])

        # the bank of masks: each type present, then the lifting robot carrying a cube (envs.py:2031-2037)
        names = sorted(set(t for env in self.robot_types for t in env))
        if 'lifting_robot' in names:
            names.append(WITH_CUBE)
        bank = []
        for name in names:
            m = robot_masks.get(name) if isinstance(robot_masks, dict) else None
            if not isinstance(m, np.ndarray) or m.dtype != np.float32 or m.shape != (arch.STATE_WIDTH, arch.STATE_WIDTH):
                raise ValueError('robot_masks[%r] must be a float32 [96, 96] array (Mapper._create_robot_mask)' % name)
            bank.append(m)
        self.mask_index = {name: k for k, name in enumerate(names)}
        self.env_begin = np.concatenate([[0], np.cumsum([len(env) for env in self.robot_types])]).tolist()
        M = self.num_mappers = self.env_begin[-1]
        self.env_of = [e for e, env in enumerate(self.robot_types) for _ in env]
        self.env_shapes = [padded_room_shape(w, l) for w, l in zip(self.room_widths, self.room_lengths)]
        self.shapes = [self.env_shapes[e] for e in self.env_of]
        self.radius = [math.floor(arch.get_robot_radius(t) * arch.LOCAL_MAP_PIXELS_PER_METER) for env in self.robot_types for t in env]   # envs.py:2420
        self.thin_radius = math.ceil(arch.ROBOT_HALF_WIDTH * arch.LOCAL_MAP_PIXELS_PER_METER)                                            # envs.py:2428
        self.channels = channel_names(self.flags, intention_channel_encoding, len(self.robot_types[0]))
        self.num_channels = len(self.channels)
        self.mask_bank = np.stack(bank)
        self._plans = {}                                   # what get_states' array form needs of a `mappers` tuple, made once
        self._windows = {}                                 # store_new_actions' per-mapper constants, the room masks' boxes among them
        cells = [r * c for r, c in self.shapes]
        self._at = np.concatenate([[0], np.cumsum(cells)]).tolist()                       # cell offset of mapper m's maps; [M]: all cells
        self._pending = [[] for _ in range(M)]             # the deferred frames of every mapper in capture order (_Deferred)
        self._staging = _Staging()
        self._route()

        # the device tensors come after the argument checks, which need no device; without one the object still checks the arguments
        # of its calls, and then says so
        self.device, self.stage_maps = None, {}
        if torch.cuda.is_available():
            self._allocate()

    def _route(self):
        """Which entry point each mapper's occupancy maps and action waypoints go through, and where its state lies in the two
        workspaces: host constants of the shapes and the room masks' boxes.  Without large_rooms every mapper takes the LDS entries,
        which refuse what they do not hold."""
        M = self.num_mappers
        self.occupancy_entry, self.action_entry = ['simq_occupancy_maps'] * M, ['simq_action_waypoints'] * M
        self._occupancy_work_at, self._action_work_at = np.zeros(M + 1, np.int64), np.zeros(M + 1, np.int64)
        if not self.large_rooms:
            return
        from .actions import split_by_window
        for m in occupancy.split_by_shape(self.shapes)[1]:
            self.occupancy_entry[m] = 'simq_occupancy_maps_large'
        boxes = self._action_constants()['box']
        for m in split_by_window(boxes.tolist())[1]:
            self.action_entry[m] = 'simq_action_waypoints_large'
        def need(fn, a, b):                                                               # (the exported host functions: no device)
            return int(fn(int(a), int(b)))
        self._occupancy_work_at[1:] = np.cumsum([need(lib.c.simq_occupancy_maps_large_work_bytes, *self.shapes[m])
                                                 if self.occupancy_entry[m].endswith('large') else 0 for m in range(M)])
        self._action_work_at[1:] = np.cumsum([need(lib.c.simq_action_waypoints_large_work_bytes, boxes[m][2], boxes[m][3])
                                              if self.action_entry[m].endswith('large') else 0 for m in range(M)])
        if (np.diff(self._occupancy_work_at) < 0).any() or (np.diff(self._action_work_at) < 0).any():
            raise ValueError('large_rooms: a room of %s padded cells is over what simq_occupancy_maps_large and simq_action_waypoints_large '
                             'take (sides up to %d, fewer than 2^22 cells)' % (sorted(set(self.shapes))[-1], occupancy.LARGE_MAX_DIM))

    def _allocate(self):
        dev = self.device = _batch.device('batched mappers')
        E, M = self.num_envs, self.num_mappers
        total = self._at[M]
        # occupancy maps and room masks are one uint8 buffer: simq_occupancy_maps reads both from one base, where they lie
        rooms = {}
        for e in range(E):
            key = (self.room_widths[e], self.room_lengths[e])
            if key not in rooms:
                rooms[key] = (total + sum(m.size for _, m in rooms.values()), room_mask(*key))
        self._mask_at = [rooms[(self.room_widths[e], self.room_lengths[e])][0] for e in self.env_of]
        self._bytes = torch.zeros(total + sum(m.size for _, m in rooms.values()), dtype=torch.uint8, device=dev)
        for at, m in rooms.values():
            self._bytes[at:at + m.size].copy_(torch.from_numpy(m.reshape(-1)))
        self._overhead = torch.zeros(total, dtype=torch.float32, device=dev)
        self._cspace = torch.zeros(total, dtype=torch.uint8, device=dev)
        self._thin = torch.zeros(total, dtype=torch.uint8, device=dev)
        self._closest = torch.zeros(2 * total, dtype=torch.int32, device=dev)
        self.occupancy_status = torch.full((M,), NOT_UPDATED, dtype=torch.int32, device=dev)
        # the workspaces of the large entries (large_rooms): every such mapper's state at its own offset, so any set of mappers may be
        # named in one call; the kernels initialise what they read
        self._occupancy_work = torch.empty(int(self._occupancy_work_at[-1]), dtype=torch.uint8, device=dev) if self._occupancy_work_at[-1] else None
        self._action_work = torch.empty(int(self._action_work_at[-1]), dtype=torch.uint8, device=dev) if self._action_work_at[-1] else None
        self.masks = torch.from_numpy(self.mask_bank).to(dev)
        self.uniform = len(set(self.shapes)) == 1

        def rows_of(flat, per=()):
            if self.uniform:
                return flat[:(2 if per else 1) * total].view((M,) + per + self.shapes[0])
            return [self._view(flat, m, per) for m in range(M)]
        self.occupancy = rows_of(self._bytes)
        self.room_masks = [self._bytes[at:at + r * c].view(r, c) for at, (r, c) in zip(self._mask_at, self.shapes)]
        self.overhead = rows_of(self._overhead)
        self.configuration_space, self.cspace_thin = rows_of(self._cspace), rows_of(self._thin)
        self.closest_cspace_indices = rows_of(self._closest, (2,))
        self.distance_to_receptacle_maps = None
        if self.flags['use_distance_to_receptacle_map']:
            made = {}
            for e in range(E):
                key = (self.env_shapes[e], self.receptacle_positions[e])
                if key not in made:
                    made[key] = torch.from_numpy(distance_to_receptacle_map(key[0], key[1], self.distance_to_receptacle_map_scale)).to(dev)
            self.distance_to_receptacle_maps = [made[(self.env_shapes[e], self.receptacle_positions[e])] for e in range(E)]

    # ---- indices ---------------------------------------------------------------------------------------------------------------
    def mapper_index(self, env, robot):
        if not (0 <= env < self.num_envs and 0 <= robot < len(self.robot_types[env])):
            raise ValueError('no robot %d in environment %d' % (robot, env))
        return self.env_begin[env] + robot

    def _mappers(self, mappers):
        if mappers is None:
            return list(range(self.num_mappers))
        ms = [int(m) for m in mappers]
        if not ms or any(m < 0 or m >= self.num_mappers for m in ms) or len(set(ms)) != len(ms):
            raise ValueError('mappers must name distinct mappers in 0 .. %d, got %s' % (self.num_mappers - 1, ms))
        return ms

    def _named(self, bad, ms):
        return ', '.join('%d (environment %d, robot %d)' % (ms[p], self.env_of[ms[p]], ms[p] - self.env_begin[self.env_of[ms[p]]]) for p in bad[:8])

    # ---- Mapper.__init__ at an episode start -------------------------------------------------------------------------------------
    def reset(self, envs=None):
        """Zero the maps of every mapper of the named environments (all when omitted), as the new Mapper objects of an episode start
        (envs.py:2025, 2416); every other environment's maps are not touched."""
        envs = list(range(self.num_envs)) if envs is None else [int(e) for e in envs]
        for e in envs:
            if not 0 <= e < self.num_envs:
                raise ValueError('no environment %d (0 .. %d)' % (e, self.num_envs - 1))
        dropped = False
        for e in envs:                                     # deferred frames belong to the Mapper objects the episode start replaces
            for m in range(self.env_begin[e], self.env_begin[e + 1]):
                dropped = dropped or bool(self._pending[m])
                self._pending[m] = []
        if dropped:
            self._staging.compact([f for waiting in self._pending for f in waiting])
        if self.device is None:
            self._allocate()
        for e in envs:
            a, b = self.env_begin[e], self.env_begin[e + 1]
            lo, hi = self._at[a], self._at[b]
            for flat in (self._overhead, self._bytes, self._cspace, self._thin):
                flat[lo:hi].zero_()
            self._closest[2 * lo:2 * hi].zero_()
            self.occupancy_status[a:b].fill_(NOT_UPDATED)

    # ---- Mapper.update + OccupancyMap.update ---------------------------------------------------------------------------------
    def update(self, depth, ids, geometries, id_ranges, mappers=None):
        """Mapper.update (envs.py:2053-2065) with OccupancyMap.update (envs.py:2444-2459) for the named mappers (all when omitted):
        frame p of `depth` / `ids` is the camera frame of mapper mappers[p]; the four arguments are simq.observation_update's.  The
        observation scatter writes `overhead` and `occupancy` in place, the second launch `configuration_space`, `cspace_thin` and
        `closest_cspace_indices`; the status words of both are read back once.  Raises SimqError naming the mappers whose frame held
        a point that is not finite (their maps are unchanged) or whose configuration space has no free cell (status 1 of
        simq_occupancy_maps: their closest cells are undefined, and get_states reports them until an update succeeds); every
        other mapper of the call is updated."""
        ms = self._mappers(mappers)
        self._nothing_pending(ms, 'update')
        if self.device is None:
            self._allocate()
        P = len(ms)
        st_obs = observation._enqueue(depth, ids, geometries, id_ranges, [self._view(self._overhead, m) for m in ms],
                                      [self._view(self._bytes, m) for m in ms])
        st_occ = self._enqueue_occupancy(ms)
        bad, codes = _batch.bad_problems(torch.cat([st_obs, st_occ]))                       # the one read-back of the call
        if bad.size:
            said = []
            for lo, name, what in ((0, 'simq_observation_update', 'hold a point that is not finite, their maps are unchanged'),
                                   (P, 'simq_occupancy_maps', 'have a configuration space without a free cell, their closest cells are undefined')):
                mine = [(int(p) - lo, int(c)) for p, c in zip(bad, codes) if lo <= p < lo + P]
                first, other = [p for p, c in mine if c == 1], [(p, c) for p, c in mine if c != 1]
                if first:
                    said.append('%s: mapper(s) %s %s' % (name, self._named(first, ms), what))
                if other:
                    said.append('%s: status %s at mapper(s) %s' % (name, [c for _, c in other][:8], self._named([p for p, _ in other], ms)))
            raise SimqError('BatchedMapper.update: ' + '; '.join(said))

    def _enqueue_occupancy(self, ms):
        """simq_occupancy_maps over the mappers `ms` -- with large_rooms simq_occupancy_maps over those within its cap, then
        simq_occupancy_maps_large over the others: queues the launches, stores their status words in `occupancy_status` and returns
        them as a device tensor [len(ms)] in the order of `ms`."""
        P, dev, M = len(ms), self.device, self.num_mappers
        fit = [p for p, m in enumerate(ms) if not self.occupancy_entry[m].endswith('large')]
        order = fit + [p for p, m in enumerate(ms) if self.occupancy_entry[m].endswith('large')]
        sent = [ms[p] for p in order]
        fields = [(self._at[m], self._mask_at[m], self._at[m], self.shapes[m][0], self.shapes[m][1], self.radius[m], self.thin_radius)
                  for m in sent]
        whole = sent == list(range(M))
        st_occ = self.occupancy_status if whole else torch.empty(P, dtype=torch.int32, device=dev)
        occupancy.call_entries(fields, len(fit), self._bytes, (self._cspace, self._thin, self._closest), st_occ, dev,
                               self._occupancy_work, [int(self._occupancy_work_at[m]) for m in sent[len(fit):]])
        if not whole:
            self.occupancy_status[torch.as_tensor(sent, dtype=torch.int64).to(dev)] = st_occ
        if order != list(range(P)):
            st_occ = st_occ[torch.as_tensor(np.argsort(order), dtype=torch.int64).to(dev)]
        return st_occ

    # ---- deferred frames: several Mapper.update calls of a mapper applied by one launch ------------------------------------------
    @property
    def pending(self):
        """The number of deferred frames of every mapper that no flush has applied yet: int64 [M]."""
        return np.asarray([len(held) for held in self._pending], np.int64)

    def _nothing_pending(self, ms, what):
        held = [p for p, m in enumerate(ms) if self._pending[m]]
        if held:
            raise SimqError('BatchedMapper.%s: mapper(s) %s have deferred frames that are not in their maps yet (%s pending); call flush() first'
                            % (what, self._named(held, ms), [len(self._pending[ms[p]]) for p in held[:8]]))

    def defer(self, depth, ids, geometries, id_ranges, mappers=None):
        """`update` put off: the arguments of `update`, checked as there, and every frame copied into host memory of this object
        (pinned where there is a device; it grows in blocks and is reused after a flush), so that the caller may overwrite its arrays.
        Nothing is launched and no device is needed.  A mapper may be named in any number of defer calls: its frames keep the order of
        the calls, and `flush` applies them all in one launch.  Until then the mapper's maps are behind: update, get_states,
        shortest_paths and distances_to_receptacle refuse it."""
        ms = self._mappers(mappers)
        depth, ids, geometries, id_ranges, P = observation._checked_frames(depth, ids, geometries, id_ranges, 'BatchedMapper.defer')
        if P != len(ms):
            raise ValueError('%d frames for %d mappers' % (P, len(ms)))
        observation._layout(depth, ids, geometries)                                       # (the checks of every frame's shape against its geometry)
        for p, m in enumerate(ms):
            g = geometries[p]
            h, w = depth[p].shape
            parts = [np.ascontiguousarray(g.pixel_x, np.float32), np.ascontiguousarray(g.pixel_y, np.float32)] + \
                [a.cpu().numpy() if isinstance(a, torch.Tensor) else a for a in (depth[p], ids[p])]
            words = w + h + 2 * h * w
            block, at = self._staging.take(words)
            room, k = self._staging.arrays[block], at
            for a in parts:
                room[k:k + a.size] = a.reshape(-1).view(np.int32)
                k += a.size
            problem = observation.ObservationProblem()
            observation._describe(problem, g, id_ranges[p], (w + h, w + h + h * w), (0, w), (h, w), self._at[m], self._at[m], self.shapes[m])
            self._pending[m].append(_Deferred(block, at, words, problem))

    def flush(self, mappers=None):
        """Applies the deferred frames of the named mappers (of every mapper that has some when omitted) in capture order, as the
        `update` calls they stand for would have: one upload per staging block that holds some of them, one
        simq_observation_update_sequences launch (more only where a mapper has more than 1 023 frames), one simq_occupancy_maps
        launch over those mappers, one read-back of all status words.  A mapper without deferred frames is left alone.  Raises
        SimqError as `update` does, naming mappers and their frames (counted from 0 in capture order): a frame with a point that is
        not finite is skipped, every other frame and mapper is applied; `occupancy_status` is kept as `update` keeps it."""
        ms = [m for m in (range(self.num_mappers) if mappers is None else self._mappers(mappers)) if self._pending[m]]
        if not ms:
            return
        if self.device is None:
            self._allocate()
        dev, staging = self.device, self._staging
        held = [(p, k, f) for p, m in enumerate(ms) for k, f in enumerate(self._pending[m])]
        spans = {}
        for _, _, f in held:
            lo, hi = spans.get(f.block, (f.at, f.at + f.words))
            spans[f.block] = (min(lo, f.at), max(hi, f.at + f.words))
        shift, words = {}, 0
        for b in sorted(spans):
            shift[b] = words - spans[b][0]
            words += spans[b][1] - spans[b][0]
        frames = torch.empty(words, dtype=torch.int32, device=dev)
        for b, (lo, hi) in sorted(spans.items()):
            frames[shift[b] + lo:shift[b] + hi].copy_(staging.tensors[b][lo:hi], non_blocking=True)
        total = self._at[self.num_mappers]
        bases = (self._overhead.data_ptr(), total, self._bytes.data_ptr(), total)
        st_obs = torch.empty(len(held), dtype=torch.int32, device=dev)
        where, at = np.empty(len(held), np.int64), 0
        for mine, begin in observation.sequence_launches([p for p, _, _ in held]):
            probs = (observation.ObservationProblem * len(mine))()
            for i, n in enumerate(mine.tolist()):
                f = held[n][2]
                probs[i] = f.problem
                q, by = probs[i], shift[f.block] + f.at
                q.depth_offset, q.ids_offset, q.px_offset, q.py_offset = q.depth_offset + by, q.ids_offset + by, q.px_offset + by, q.py_offset + by
            observation.call_sequences(frames, words, probs, begin, bases, st_obs[at:at + len(mine)], dev)
            where[mine] = at + np.arange(len(mine))
            at += len(mine)
        st_occ = self._enqueue_occupancy(ms)
        codes = torch.cat([st_obs, st_occ]).cpu().numpy()                                  # the one read-back of the call
        for m in ms:
            self._pending[m] = []
        staging.compact([f for waiting in self._pending for f in waiting])                 # (the read-back has waited for the uploads)
        obs, occ = codes[:len(held)][where], codes[len(held):]
        if obs.any() or occ.any():
            said = []
            skipped = [n for n in np.flatnonzero(obs == 1).tolist()]
            if skipped:
                said.append('simq_observation_update_sequences: %s hold a point that is not finite, those frames are skipped' % ', '.join(
                    'mapper %s frame %d' % (self._named([held[n][0]], ms), held[n][1]) for n in skipped[:8]))
            other = [n for n in np.flatnonzero(obs > 1).tolist()]
            if other:
                said.append('simq_observation_update_sequences: status %s at %s' % (obs[other][:8].tolist(), ', '.join(
                    'mapper %s frame %d' % (self._named([held[n][0]], ms), held[n][1]) for n in other[:8])))
            first, rest = np.flatnonzero(occ == 1).tolist(), np.flatnonzero(occ > 1).tolist()
            if first:
                said.append('simq_occupancy_maps: mapper(s) %s have a configuration space without a free cell, their closest cells are undefined'
                            % self._named(first, ms))
            if rest:
                said.append('simq_occupancy_maps: status %s at mapper(s) %s' % (occ[rest][:8].tolist(), self._named(rest, ms)))
            raise SimqError('BatchedMapper.flush: ' + '; '.join(said))

    def _view(self, flat, m, per=()):
        k = 2 if per else 1
        return flat[k * self._at[m]:k * self._at[m + 1]].view(per + self.shapes[m])

    # ---- Mapper.get_state ------------------------------------------------------------------------------------------------------
    def _robots(self, robots, envs):
        try:
            n = len(robots)
        except TypeError:
            raise ValueError('robots holds one list of RobotState per environment') from None
        if n != self.num_envs:
            raise ValueError('robots holds one list of RobotState per environment: %d lists for %d environments' % (n, self.num_envs))
        out = {}
        for e in envs:
            states = [r if isinstance(r, RobotState) else RobotState(*r) for r in robots[e]]
            if len(states) != len(self.robot_types[e]):
                raise ValueError('environment %d has %d robots, got %d robot states' % (e, len(self.robot_types[e]), len(states)))
            for k, (r, t) in enumerate(zip(states, self.robot_types[e])):
                if r.robot_type is not None and r.robot_type != t:
                    raise ValueError('environment %d, robot %d is a %s, got the state of a %s' % (e, k, t, r.robot_type))
            out[e] = states
        return out

    def _stamps(self, e, states):
        """The robots of environment e as the robot map and the overhead map draw them (envs.py:2250-2275)."""
        stamps = []
        for r, t, g in zip(states, self.robot_types[e], self.group_indices[e]):
            own = self.mask_index[t]
            lifting = t == 'lifting_robot' and r.lift_state == 'lifting'
            stamps.append(local_maps.RobotStamp(r.position, r.heading, self.mask_index[WITH_CUBE] if lifting else own,
                                                self.seg_values['robot_group_%d' % (g + 1)],
                                                0.5 if t == 'lifting_robot' and not lifting else 1.0, own))
        return stamps

    def _drawn(self, states, own, encoding):
        """What Mapper._create_global_intention_or_history_map draws for robot `own` of an environment (envs.py:2303-2317)."""
        out = []
        for k, r in enumerate(states):
            if k == own or r.idle:
                continue
            path = r.target if encoding == 'circle' else r.history_path if encoding == 'history' else r.intention_path
            if path is None:
                raise ValueError('a robot that is not idle needs its %s for the %r encoding' % (
                    'target' if encoding == 'circle' else 'history_path' if encoding == 'history' else 'intention_path', encoding))
            out.append(path)
        return out

    def get_states(self, robots, mappers=None, out=None, into=None, pools=None):
        """Mapper.get_state() (envs.py:2067-2112) for the named mappers (all when omitted): a float32 [P, 96, 96, C] device tensor,
        state p that of mapper mappers[p], the channels in `self.channels`' order.  robots: per environment the RobotState of each
        robot, in env.robots' order (only the environments of the named mappers are read), or one RobotArrays with the same robots as
        arrays: the same calls and states, the descriptors built without Python per state.  out: a contiguous float32 device
        tensor [P, 96, 96, C] to write into -- a batch buffer, a slice of a replay ring's `states`; every element is written.
        into: instead of `out`, P handles of one AliasedDeviceReplayBuffer (ring.reserve(P)) for states of C channels: state p is
        written where it will be sampled from, the pool slot of into[p], and the handles are returned -- for TransitionTracker,
        the policies' step_many and ring.push, which all take them where they take an ndarray.  A pool of bf16 states
        (AliasedDeviceReplayBuffer(..., dtype='bf16')) receives each state rounded once to nearest even (simq_local_state_images_slots_bf16).
        pools: with `into`, the rings of all robot groups among the named mappers -- 1 to 16 distinct AliasedDeviceReplayBuffers of C
        channels on the mapper's device, of any mix of dtype.  into[p] is then a handle of the ring of mapper p's group, in any
        interleaving, and the states of all groups are written by the one state launch (simq_local_state_images_pools, also for one
        listed ring): one chain and one status read-back per call however many groups there are.

        The distance images and the states are one launch each; the drawn maps one launch per room shape among the named mappers
        (simq_intention_maps draws maps of one shape) or, for an object made with one_drawing_launch=True, one launch whatever the
        shapes (simq_intention_maps_shapes).  Raises ValueError for a wrong robot count or `out`; SimqError, after the
        whole chain has run, naming the mappers whose distance images could not be computed (no successful update yet, a
        configuration space without a free cell): their distance channels come from images of zeros, every other mapper's state is
        right."""
        ms = self._mappers(mappers)
        self._nothing_pending(ms, 'get_states')
        P, C = len(ms), self.num_channels
        want = (P, arch.STATE_WIDTH, arch.STATE_WIDTH, C)
        pool = None
        if into is not None:
            if out is not None:
                raise ValueError('get_states: `into` and `out` name two destinations; pass one')
            into, pool = local_maps.check_into(into, 'get_states', P, C, pools)
        local_maps.check_pools_argument('get_states', out, into, pools)
        if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == want and out.is_contiguous()):
            raise ValueError('out must be a contiguous float32 device tensor of shape %s, got %s' % (
                want, '%s %s' % (out.dtype, tuple(out.shape)) if isinstance(out, torch.Tensor) else type(out).__name__))
        if isinstance(robots, RobotArrays):
            return self._get_states_arrays(robots, ms, out, into, pool, want)
        states = self._robots(robots, sorted(set(self.env_of[m] for m in ms)))
        f = self.flags
        own = [(self.env_of[m], m - self.env_begin[self.env_of[m]]) for m in ms]
        pixel = local_maps.position_to_pixel_indices

        # ---- the host side of every stage first: a wrong argument launches nothing
        sources, grid = [], []                                   # stage 1: (pixel, mapper) of every distance image
        if f['use_shortest_path_to_receptacle_map']:
            sources += [pixel(self.receptacle_positions[e][0], self.receptacle_positions[e][1], self.env_shapes[e]) for e, _ in own]
            grid += ms
        if f['use_shortest_path_map']:
            sources += [pixel(states[e][r].position[0], states[e][r].position[1], self.env_shapes[e]) for e, r in own]
            grid += ms
        jobs, order = [], {}                                     # stage 2: (key, problem, paths, encoding) of every drawn map
        if f['use_history_map']:
            jobs += [(('history', p), p, self._drawn(states[e], r, 'history'), 'history') for p, (e, r) in enumerate(own)]
        if f['use_intention_map']:
            jobs += [(('intention', p), p, self._drawn(states[e], r, self.intention_map_encoding), self.intention_map_encoding)
                     for p, (e, r) in enumerate(own)]
        constants = {}
        if f['use_intention_channels']:
            for p, (e, r) in enumerate(own):
                me = states[e][r]
                dists = [_distance(me.position, other.position) for other in states[e]]
                order[p] = [int(k) for k in np.argsort(dists) if k != r]                       # envs.py:2350-2358
                for q, k in enumerate(order[p]):
                    other = states[e][k]
                    if not other.idle and other.target is None:
                        raise ValueError('a robot that is not idle needs its target for the intention channels')
                    if self.intention_channel_encoding == 'spatial':                          # envs.py:2360-2366
                        jobs.append((('channel', p, q), p, [] if other.idle else [other.target], 'circle'))
                        continue
                    relative_position = (0, 0)                                              # envs.py:2368-2375
                    if not other.idle:
                        dist = _distance(me.position, other.target)
                        theta = me.heading - math.atan2(other.target[1] - me.position[1], other.target[0] - me.position[0])
                        relative_position = (dist * math.sin(theta), dist * math.cos(theta))
                    constants[(p, q)] = [float(np.float32(self.intention_channel_nonspatial_scale * coord)) for coord in relative_position]
        if self.device is None:
            self._allocate()
        if out is not None and out.device != self.device:
            raise ValueError('out must be a contiguous float32 device tensor of shape %s on %s' % (want, self.device))
        for ring in local_maps.rings(pool) if pool is not None else ():
            if ring.pool.device != self.device:
                raise ValueError('get_states(into=): the pool lives on %s, the maps on %s' % (ring.pool.device, self.device))

        # ---- stage 1: the distance images, every source snapped through the closest cells on the device
        status, images = None, []
        if sources:
            grids = [self._view(self._cspace, m) for m in range(self.num_mappers)]
            closest = [self._view(self._closest, m, (2,)) for m in range(self.num_mappers)]
            images, status, uniform, shapes, _ = grid_paths._enqueue(
                grids, sources, arch.LOCAL_MAP_PIXELS_PER_METER, True, self.shortest_path_map_scale, None, grid, closest, grid,
                self.occupancy_status, grid)
            images = list(images) if uniform else _batch.views(images.view(-1), shapes)

        # ---- stage 2: history maps, intention maps and the maps behind the spatial intention channels: one launch per room shape
        # (one_drawing_launch: one simq_intention_maps_shapes launch for all of them, `drawn` views of its flat tensor)
        drawn = {}
        drawn_shapes = sorted(set(self.shapes[ms[p]] for _, p, _, _ in jobs))
        if self.one_drawing_launch and len(drawn_shapes) > 1:
            args, maps, keep = intention_drawing._prepare_shapes([j[2] for j in jobs], [self.shapes[ms[j[1]]] for j in jobs], [j[3] for j in jobs],
                                                                 self.intention_map_scale, self.intention_map_line_thickness, None)
            lib.call('simq_intention_maps_shapes', *args)
            del keep
            drawn.update({j[0]: maps[k] for k, j in enumerate(jobs)})
            drawn_shapes = []
        for shape in drawn_shapes:
            mine = [j for j in jobs if self.shapes[ms[j[1]]] == shape]
            args, maps, keep = intention_drawing._prepare([j[2] for j in mine], shape, [j[3] for j in mine], self.intention_map_scale,
                                                          self.intention_map_line_thickness, None)
            lib.call('simq_intention_maps', *args)
            del keep
            drawn.update({j[0]: maps[k] for k, j in enumerate(mine)})

        # ---- stage 3: crop and rotation of every channel into the states
        maps, index = [], {}

        def use(key, tensor):
            if key not in index:
                index[key] = len(maps)
                maps.append(tensor)
            return index[key]
        channels = []
        for p, (e, r) in enumerate(own):
            ch, d = [('overhead', use(('overhead', p), self._view(self._overhead, ms[p])))], 0
            if f['use_robot_map']:
                ch.append('robots')
            if f['use_distance_to_receptacle_map']:
                ch.append(('distance', use(('receptacle', id(self.distance_to_receptacle_maps[e])), self.distance_to_receptacle_maps[e])))
            for flag in ('use_shortest_path_to_receptacle_map', 'use_shortest_path_map'):
                if f[flag]:
                    ch.append(('distance', use(('image', d, p), images[d * P + p])))
                    d += 1
            for flag, name in (('use_history_map', 'history'), ('use_intention_map', 'intention')):
                if f[flag]:
                    ch.append(('map', use((name, p), drawn[(name, p)])))
            if f['use_intention_channels']:
                for q in range(len(order[p])):
                    if self.intention_channel_encoding == 'spatial':
                        ch.append(('map', use(('channel', p, q), drawn[('channel', p, q)])))
                    else:
                        ch += [('constant', v) for v in constants[(p, q)]]
            channels.append(ch)
        stamps = {e: self._stamps(e, s) for e, s in states.items()}
        poses = [(states[e][r].position, states[e][r].heading) for e, r in own]
        args, out, keep = local_maps._prepare(maps, channels, poses, [stamps[e] for e, _ in own], self.masks, out, None, into=into, pools=pools)
        if pool is None:
            lib.call('simq_local_state_images', *args)
        else:
            local_maps.write_into(pool, into, args)
            out = into
        del keep
        # what the stages left on the device, until the next call: {('image', 0 or 1, p)}: the distance images in the order of the
        # flags, {('history', p), ('intention', p), ('channel', p, q)}: the drawn maps (p: position in `mappers`, q: channel)
        self.stage_maps = {key: maps[k] for key, k in index.items() if key[0] in ('image', 'history', 'intention', 'channel')}

        if status is not None:
            bad, codes = _batch.bad_problems(status)                                        # the one read-back of the call
            if bad.size:
                raise SimqError('BatchedMapper.get_states: no distance images for mapper(s) %s (simq_grid_distance_images_snapped status %s; '
                                '%d: no update since the last reset, 1: a configuration space without a free cell); their distance '
                                'channels come from images of zeros'
                                % (self._named(sorted(set(int(p) % P for p in bad)), ms), codes[:8].tolist(), NOT_UPDATED))
        return out

    # ---- get_states from a RobotArrays: the same three calls with the descriptor tables built as arrays -------------------------
    def _plan(self, ms):
        """What the array form needs of the tuple `ms` and not of a call's robots (_Plan), made once per tuple.  The eight tuples used last are
        kept (the dict is in order of last use); a tuple that is not among them pays for a new plan -- DESIGN.md section 19 has the cost."""
        key = tuple(ms)
        plan = self._plans.pop(key, None)
        if plan is None:
            if len(self._plans) >= 8:
                del self._plans[next(iter(self._plans))]
            plan = _Plan(self, ms)
        self._plans[key] = plan
        return plan

    def _get_states_arrays(self, ra, ms, out, into, pool, want):
        """get_states for `robots` a RobotArrays, after the checks of `mappers`, `out` and `into`: the calls of the list form with equal
        arguments and descriptor bytes (tests/test_gpu_robot_arrays.py), formed without a Python loop over the states."""
        if ra.num_mappers != self.num_mappers:
            raise ValueError('the RobotArrays hold %d mappers, the object has %d' % (ra.num_mappers, self.num_mappers))
        f, P, C = self.flags, len(ms), self.num_channels
        plan = self._plan(ms)
        pixels = local_maps.pixel_indices_many
        spatial = f['use_intention_channels'] and self.intention_channel_encoding == 'spatial'

        # ---- the host side of every stage first: a wrong argument launches nothing
        robot_i, robot_j = pixels(ra.position[plan.robots, 0], ra.position[plan.robots, 1], (plan.robot_rows, plan.robot_cols))
        degrees = ra.heading[plan.robots] * local_maps.RAD_TO_DEG
        own_i, own_j = robot_i[plan.own_row], robot_j[plan.own_row]
        idle = ra.idle[plan.others]                                  # of the pairs (p, another robot of p's environment), p by p
        busy = plan.others[~idle]
        for flag, name, encoding in (('use_history_map', 'history_path', 'history'),
                                     ('use_intention_map', 'target' if self.intention_map_encoding == 'circle' else 'intention_path',
                                      self.intention_map_encoding)):
            held = getattr(ra, name)
            if f[flag] and busy.size and (held is None or (np.isnan(held[busy]).any() if name == 'target' else
                                                           (held[1][busy + 1] == held[1][busy]).any())):
                raise ValueError('a robot that is not idle needs its %s for the %r encoding' % (name, encoding))
        order = constants = None
        if f['use_intention_channels']:
            R = plan.R
            mine = ra.position[plan.env_rows]                        # [P, R, 2]: the robots of p's environment
            me = ra.position[plan.ms]
            order = closest_order(mine, me, plan.robot)
            ranked = (plan.env_rows[:, :1] + order).reshape(-1)      # the mapper behind channel (p, q)
            ranked_busy = ~ra.idle[ranked]
            if ranked_busy.any() and (ra.target is None or np.isnan(ra.target[ranked[ranked_busy]]).any()):
                raise ValueError('a robot that is not idle needs its target for the intention channels')
            if not spatial:                                          # envs.py:2368-2375, in Python floats as there
                scale, constants = self.intention_channel_nonspatial_scale, []
                targets = ra.target[ranked].tolist() if ra.target is not None else None
                for k, (p, is_busy) in enumerate(zip(np.repeat(np.arange(P), R - 1).tolist(), ranked_busy.tolist())):
                    relative_position = (0, 0)
                    if is_busy:
                        (x, y), heading, target = me[p].tolist(), float(ra.heading[ms[p]]), targets[k]
                        dist = math.sqrt((target[0] - x)**2 + (target[1] - y)**2)
                        theta = heading - math.atan2(target[1] - y, target[0] - x)
                        relative_position = (dist * math.sin(theta), dist * math.cos(theta))
                    constants += [scale * coord for coord in relative_position]
                constants = np.asarray(constants, np.float64).astype(np.float32)

        # stage 1: (pixel, mapper) of every distance image
        c_grid = None
        if plan.grid is not None:
            c_grid = plan.grid.copy()
            if f['use_shortest_path_map']:
                c_grid['src_i'][-P:], c_grid['src_j'][-P:] = own_i, own_j

        # stage 2: every drawn robot's segments once per encoding, then each problem's rows by index
        launches = []
        if plan.jobs:
            intention_drawing.check_drawing(self.intention_map_scale, self.intention_map_line_thickness)
            drawn = np.unique(busy)
            tables, begin, count, at = [], {}, {}, 0
            for flag, encoding in (('use_history_map', 'history'), ('use_intention_map', self.intention_map_encoding), (spatial, 'circle')):
                if encoding in begin or not (flag is True or f.get(flag)):
                    continue
                rows, cols = plan.rows_of[drawn], plan.cols_of[drawn]
                if not drawn.size:
                    table, n = np.zeros(0, intention_drawing.SEGMENT), np.zeros(0, np.int64)
                elif encoding == 'circle':
                    table, n = intention_drawing.circle_segments(ra.target[drawn], rows, cols, self.intention_map_scale), np.ones(len(drawn), np.int64)
                else:
                    points, offsets = ra.history_path if encoding == 'history' else ra.intention_path
                    table, n = intention_drawing.path_segments(points, offsets[drawn], offsets[drawn + 1], rows, cols, encoding,
                                                               self.intention_map_scale)
                begin[encoding], count[encoding] = np.zeros(self.num_mappers, np.int64), np.zeros(self.num_mappers, np.int64)
                begin[encoding][drawn], count[encoding][drawn] = at + intention_drawing._starts(n), n
                tables.append(table)
                at += len(table)
            tables = np.concatenate([t.view(np.uint8) for t in tables]).view(intention_drawing.SEGMENT)    # (bytes: no promotion of the fields)
            for shape, sel in plan.jobs:
                who = []                                             # the robots each problem draws, problem by problem
                for flag, encoding in (('use_history_map', 'history'), ('use_intention_map', self.intention_map_encoding)):
                    if f[flag]:
                        who.append((encoding, plan.others[sel['pairs']]))
                if spatial:
                    who.append(('circle', ranked.reshape(P, -1)[sel['p']].reshape(-1)))
                first = np.concatenate([begin[e][m] for e, m in who])
                n = np.concatenate([count[e][m] for e, m in who])
                c_segs = tables[intention_drawing.ragged(first, n)]
                seg_count = np.bincount(sel['problem'], weights=n, minlength=sel['n']).astype(np.int64)
                if shape is None:                                    # all room shapes in one call: every problem with its own
                    c_probs = intention_drawing.shaped_problems(sel['shapes'], sel['at'], intention_drawing._starts(seg_count), seg_count,
                                                                self.intention_map_line_thickness - 1)
                else:
                    c_probs = np.zeros(sel['n'], intention_drawing.PROBLEM)
                    c_probs['seg_count'] = seg_count
                    c_probs['seg_begin'] = intention_drawing._starts(c_probs['seg_count'])
                launches.append((shape, c_segs, c_probs))

        # stage 3: the robots as they are stamped, the problems, the channel values of this call
        c_robots = plan.stamps.copy()
        c_robots['rot'] = local_maps.rotation_table(degrees - 90, local_maps.WIDTH)
        c_robots['pixel_i'], c_robots['pixel_j'] = robot_i, robot_j
        lifting = plan.lifters & ra.lifting[plan.robots]
        c_robots['mask'] = np.where(lifting, plan.cube_mask, c_robots['seg_mask'])
        c_robots['map_value'] = np.where(plan.lifters & ~lifting, 0.5, 1.0)
        c_probs3 = plan.problems.copy()
        c_probs3['rot'] = local_maps.rotation_table(90 - degrees[plan.own_row], local_maps.CROP)
        c_probs3['pixel_i'], c_probs3['pixel_j'] = own_i, own_j
        c_chans = plan.channels
        if constants is not None:
            c_chans = c_chans.copy()
            c_chans['value'][plan.constant_at] = constants

        if self.device is None:
            self._allocate()
        dev = self.device
        if out is not None and out.device != dev:
            raise ValueError('out must be a contiguous float32 device tensor of shape %s on %s' % (want, dev))
        for ring in local_maps.rings(pool) if pool is not None else ():
            if ring.pool.device != dev:
                raise ValueError('get_states(into=): the pool lives on %s, the maps on %s' % (ring.pool.device, dev))
        fixed = plan.on_device(self)
        c_maps = fixed['maps'].copy()
        buffers, as_ctypes = {}, local_maps.as_ctypes

        # ---- stage 1
        status = None
        if c_grid is not None:
            images = torch.empty(plan.grid_want, dtype=torch.float32, device=dev)
            d_probs = torch.empty(c_grid.nbytes, dtype=torch.uint8, device=dev)
            status = torch.empty(len(c_grid), dtype=torch.int32, device=dev)
            lib.call('simq_grid_distance_images_snapped', ctypes.c_void_p(fixed['grids']), ctypes.c_int64(plan.grid_cells),
                     ctypes.c_void_p(fixed['closest']), ctypes.c_int64(2 * plan.grid_cells), as_ctypes(c_grid, grid_paths.SnappedProblem),
                     len(c_grid), ptr(d_probs), ptr(images), ctypes.c_int64(images.numel()), ctypes.c_float(float(arch.LOCAL_MAP_PIXELS_PER_METER)),
                     1, ctypes.c_float(float(self.shortest_path_map_scale)), ptr(self.occupancy_status), self.occupancy_status.numel(),
                     ptr(status), stream_ptr(dev))
            c_maps['d_data'][plan.image_maps] = images.data_ptr() + 4 * plan.image_at
            buffers['image'] = (images.view(-1), plan.image_at.tolist(), plan.image_shapes)

        # ---- stage 2: one launch per room shape, or (one_drawing_launch) one for all of them
        for (shape, c_segs, c_probs), (_, sel) in zip(launches, plan.jobs):
            if shape is None:
                flat = torch.empty(sel['cells'], dtype=torch.float32, device=dev)
                args, d_desc = intention_drawing.shapes_call(c_segs, c_probs, flat, dev)
                lib.call('simq_intention_maps_shapes', *args)
                c_maps['d_data'][sel['maps']] = flat.data_ptr() + 4 * sel['at']
                buffers['drawn'] = (flat, sel['at'].tolist(), sel['shape_list'])
                continue
            maps = torch.empty((len(c_probs),) + shape, dtype=torch.float32, device=dev)
            d_desc = torch.empty(max(int(lib.c.simq_intention_desc_bytes(len(c_segs), len(c_probs))), 8), dtype=torch.uint8, device=dev)
            lib.call('simq_intention_maps', as_ctypes(c_segs, intention_drawing.Segment) if len(c_segs) else None, len(c_segs),
                     as_ctypes(c_probs, intention_drawing.Problem), len(c_probs), shape[0], shape[1], self.intention_map_line_thickness - 1,
                     ptr(d_desc), ctypes.c_int64(d_desc.numel()), ptr(maps), ctypes.c_int64(maps.numel()), stream_ptr(dev))
            c_maps['d_data'][sel['maps']] = maps.data_ptr() + 4 * shape[0] * shape[1] * np.arange(len(c_probs), dtype=np.int64)
            buffers[shape] = maps

        # ---- stage 3
        n_maps, n_robots = len(c_maps), len(c_robots)
        args = (as_ctypes(c_maps, local_maps.LocalMap), n_maps, ptr(self.masks), self.masks.shape[0], as_ctypes(c_robots, local_maps.LocalRobot),
                n_robots, as_ctypes(c_probs3, local_maps.LocalProblem), P, as_ctypes(c_chans, local_maps.LocalChannel), C)
        if pool is None:
            if out is None:
                out = torch.empty(want, dtype=torch.float32, device=dev)
            d_desc = torch.empty(max(int(lib.c.simq_local_state_desc_bytes(n_maps, n_robots, P, C)), 8), dtype=torch.uint8, device=dev)
            lib.call('simq_local_state_images', *args, ptr(d_desc), ctypes.c_int64(d_desc.numel()), ptr(out), ctypes.c_int64(out.numel()),
                     stream_ptr(dev))
        else:
            local_maps.write_into(pool, into, args)
            out = into
        self.stage_maps = _StageMaps(plan.stage_keys, buffers)

        if status is not None:
            bad, codes = _batch.bad_problems(status)                                        # the one read-back of the call
            if bad.size:
                raise SimqError('BatchedMapper.get_states: no distance images for mapper(s) %s (simq_grid_distance_images_snapped status %s; '
                                '%d: no update since the last reset, 1: a configuration space without a free cell); their distance '
                                'channels come from images of zeros'
                                % (self._named(sorted(set(int(p) % P for p in bad)), ms), codes[:8].tolist(), NOT_UPDATED))
        return out

    # ---- Mapper.shortest_path and Mapper.distance_to_receptacle on the stored tensors -----------------------------------------
    def shortest_paths(self, source_positions, target_positions, mappers=None, simplify=None):
        """Mapper.shortest_path (envs.py:2186-2187) of the named mappers: simq.shortest_paths on this object's tensors (simplify: None for
        scikit-image, 'exact' for the integer rule on the device behind the search, or a callable(coords, tolerance))."""
        from .waypoints import shortest_paths
        ms = self._mappers(mappers)
        self._nothing_pending(ms, 'shortest_paths')
        return shortest_paths(self.configuration_space, self.cspace_thin, self.closest_cspace_indices, source_positions, target_positions,
                              ms, simplify, **({'large_windows': True} if self.large_rooms else {}))

    # ---- Robot.store_new_action on the stored tensors --------------------------------------------------------------------------
    def _action_constants(self):
        """What store_new_actions needs of every mapper and of no call, as arrays [M], made once: its robot's type, output channels
        and END_EFFECTOR_LOCATION + CUBE_WIDTH / 2; its map's shape and cell offset; and the window simq_action_waypoints searches,
        the bounding box of its room mask, a host constant per room -- the configuration space is zero outside the mask
        (envs.py:2453), so the box holds every free cell."""
        if not self._windows:
            from .actions import constants_of, free_box
            types = [t for env in self.robot_types for t in env]
            boxes = {}
            for e in range(self.num_envs):
                key = (self.room_widths[e], self.room_lengths[e])
                if key not in boxes:
                    boxes[key] = free_box(room_mask(*key))
            channels, reach = constants_of(types)
            self._windows = dict(
                types=np.asarray(types), channels=channels, reach=reach, rows=np.asarray([s[0] for s in self.shapes], np.int32),
                cols=np.asarray([s[1] for s in self.shapes], np.int32), at=np.asarray(self._at[:-1], np.int64),
                box=np.asarray([boxes[(self.room_widths[e], self.room_lengths[e])] for e in self.env_of], np.int32))
        return self._windows

    def store_new_actions(self, actions, robots, mappers=None, use_shortest_path_movement=True):
        """Robot.store_new_action (envs.py:856-902) of the named mappers' robots (all when omitted) in one call: actions[p] is the
        integer step_many returned for the robot of mapper mappers[p]; robots is get_states' argument in either form (only position
        and heading of the named robots are read); robot types and maps are the object's.  Returns simq.actions.NewActions: arrays,
        whose as_lists() gives per robot the reference's action, target_end_effector_position, waypoint_positions and
        waypoint_headings bit for bit.

        One simq_action_waypoints launch on the maps where they lie, windowed by the room mask's box, with `occupancy_status` as its
        upstream status, and one read-back (one more round only for a robot with more than actions.WAY_CAPACITY waypoints); with
        use_shortest_path_movement=False nothing is launched.  Raises ValueError for a wrong argument, without a device; SimqError
        for pending deferred frames, and -- after the call has completed -- naming the mappers whose problem ended with another status
        than traced or straight, or whose word of `occupancy_status` is not 0 (NOT_UPDATED: no update since the last reset, 1: a
        configuration space without a free cell)."""
        from . import actions as act
        ms = self._mappers(mappers)
        self._nothing_pending(ms, 'store_new_actions')
        P, fixed = len(ms), self._action_constants()
        if isinstance(robots, RobotArrays):
            if robots.num_mappers != self.num_mappers:
                raise ValueError('the RobotArrays hold %d mappers, the object has %d' % (robots.num_mappers, self.num_mappers))
            given, positions, headings = None, robots.position[ms], robots.heading[ms]
        else:
            own = [(self.env_of[m], m - self.env_begin[self.env_of[m]]) for m in ms]
            states = self._robots(robots, sorted(set(e for e, _ in own)))
            given = [states[e][r].position for e, r in own]
            positions = np.asarray([(p[0], p[1]) for p in given], np.float64).reshape(P, 2)
            headings = np.asarray([states[e][r].heading for e, r in own], np.float64)
        positions, headings, actions, _, _ = act._as_inputs(positions, headings, actions, fixed['types'][ms].tolist())
        action, targets = act._targets(actions, positions, headings, fixed['channels'][ms])
        rows, cols, reach = fixed['rows'][ms], fixed['cols'][ms], fixed['reach'][ms]
        if not use_shortest_path_movement:
            none = np.zeros(P, np.int64)
            return act._finish(action, positions, headings, targets, reach, np.full(P, act.STRAIGHT), none, np.zeros((0, 2), np.int64), rows,
                               cols, given)
        probs = np.zeros(P, act.ACTION_PROBLEM)
        probs['rows'], probs['cols'] = rows, cols
        probs['src_i'], probs['src_j'] = local_maps.pixel_indices_many(positions[:, 0], positions[:, 1], (rows, cols))
        probs['tgt_i'], probs['tgt_j'] = local_maps.pixel_indices_many(targets[:, 0], targets[:, 1], (rows, cols))
        at = fixed['at'][ms]
        probs['cspace_offset'], probs['thin_offset'], probs['closest_offset'], probs['upstream'] = at, at, 2 * at, ms
        probs['box_i0'], probs['box_j0'], probs['box_rows'], probs['box_cols'] = fixed['box'][ms].T
        if act.search is None and self.device is None:
            self._allocate()
        bases = None if self.device is None else (self._cspace, self._thin, self._closest)
        large = {}
        if self.large_rooms:                                         # (the default call is the call as it was)
            large = dict(large_windows=True, work=None if self.device is None else (self._action_work, self._action_work_at[ms]))
        status, counts, _, pixels, words = act.run_problems(probs, bases, None if self.device is None else self.occupancy_status,
                                                            what='BatchedMapper.store_new_actions', **large)
        bad = np.flatnonzero((words != 0) | ((status != act.TRACED) & (status != act.STRAIGHT)))
        codes = status[bad]
        if bad.size:
            raise SimqError('BatchedMapper.store_new_actions: no waypoints for mapper(s) %s (simq_action_waypoints status %s; %d: no update '
                            'since the last reset, 1 from the occupancy maps: a configuration space without a free cell, 2: a bad pixel or '
                            'window); every other robot of the call was computed' % (self._named(bad.tolist(), ms), codes[:8].tolist(), NOT_UPDATED))
        return act._finish(action, positions, headings, targets, reach, status, counts, pixels, rows, cols, given)

    def distances_to_receptacle(self, positions, mappers=None, shortest_path=True):
        """Mapper.distance_to_receptacle (envs.py:2189-2194) for the named mappers' position lists: simq.distances_to_receptacle on this
        object's tensors, with the receptacle of each mapper's environment."""
        from .grid_queries import distances_to_receptacle
        ms = self._mappers(mappers)
        self._nothing_pending(ms, 'distances_to_receptacle')
        if any(self.receptacle_positions[self.env_of[m]] is None for m in ms):
            raise ValueError('distances_to_receptacle needs the receptacle_position the object was built with')
        return distances_to_receptacle(self.configuration_space, self.closest_cspace_indices,
                                       [self.receptacle_positions[self.env_of[m]] for m in ms], positions, ms, shortest_path)
