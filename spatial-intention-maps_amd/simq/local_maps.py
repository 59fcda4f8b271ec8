"""Local state images on the GPU: the crop / rotation stage of the reference's ``Mapper.get_state``.

The reference (envs.py:2067-2215) turns every global map -- overhead map, robot map, shortest-path distance images, intention maps --
into a 96 x 96 robot-centred, heading-aligned image with ``scipy.ndimage.rotate(crop, angle, order=0)`` and stacks them into a
``[96, 96, C]`` float32 state.  ``simq_local_state_images`` (csrc/local_maps.hip) writes the states of many robots in one launch, bit for
bit equal to that sequence, reading the global maps where they already are on the device (e.g. the tensor
``simq.grid_distance_images`` returned) and writing NHWC states where they are consumed (a batch for ``FCN.infer_argmax_batch``, a slice
of ``DeviceReplayBuffer.states``).  The rotation matrices are computed here exactly as ``rotate`` computes them (``scipy.special``'s
``cosdg`` / ``sindg``, float64) and handed to the library as doubles; the library itself does no trigonometry.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _batch
from ._lib import SimqError, lib, ptr, stream_ptr

WIDTH = 96                       # Mapper.LOCAL_MAP_PIXEL_WIDTH (envs.py:2010)
PIXELS_PER_METER = 96.0          # Mapper.LOCAL_MAP_PIXELS_PER_METER (envs.py:2012)
CROP = 136                       # round_up_to_even(sqrt(2) * 96) (envs.py:2201)
KINDS = {'map': 0, 'distance': 1, 'robots': 2, 'overhead': 3, 'constant': 4}

# One robot of an environment as the robot map / overhead map draw it (envs.py:2250-2275): its pose, the index of its mask in the bank
# (Mapper.robot_masks: per robot class, plus the lifting robot carrying a cube), the overhead map's segmentation value of its group and
# the robot map's value (1, or 0.5 for a LiftingRobot that is not lifting).  The overhead map always draws the class's own mask
# (envs.py:2254-2256), the robot map the mask with the cube while a LiftingRobot lifts (envs.py:2258-2260): seg_mask names the former when
# it differs from `mask` (None: the same).
RobotStamp = collections.namedtuple('RobotStamp', ('position', 'heading', 'mask', 'seg_value', 'map_value', 'seg_mask'), defaults=(1.0, None))


class Rotation(ctypes.Structure):
    """simq_local_rotation of include/simq.h."""
    _fields_ = [('r', ctypes.c_double * 4), ('offset', ctypes.c_double * 2), ('shape', ctypes.c_int32 * 2)]


class LocalMap(ctypes.Structure):
    """simq_local_map of include/simq.h."""
    _fields_ = [('d_data', ctypes.c_void_p), ('rows', ctypes.c_int32), ('cols', ctypes.c_int32)]


class LocalRobot(ctypes.Structure):
    """simq_local_robot of include/simq.h."""
    _fields_ = [('rot', Rotation), ('pixel_i', ctypes.c_int32), ('pixel_j', ctypes.c_int32), ('mask', ctypes.c_int32),
                ('seg_value', ctypes.c_float), ('map_value', ctypes.c_float), ('seg_mask', ctypes.c_int32)]


class LocalProblem(ctypes.Structure):
    """simq_local_problem of include/simq.h."""
    _fields_ = [('rot', Rotation), ('pixel_i', ctypes.c_int32), ('pixel_j', ctypes.c_int32), ('rows', ctypes.c_int32),
                ('cols', ctypes.c_int32), ('robot_begin', ctypes.c_int32), ('robot_count', ctypes.c_int32)]


class LocalChannel(ctypes.Structure):
    """simq_local_channel of include/simq.h."""
    _fields_ = [('kind', ctypes.c_int32), ('map', ctypes.c_int32), ('value', ctypes.c_float), ('reserved_', ctypes.c_int32)]


def _special():
    try:
        from scipy import special
    except ImportError as e:
        raise SimqError('simq local state images take their rotation matrices from scipy.special.cosdg / sindg, as the reference\'s '
                        'scipy.ndimage.rotate does, and scipy is not importable here (%s)' % e) from None
    return special


def rotation(angle, n):
    """(R [2, 2], offset [2], shape [2]) of ``scipy.ndimage.rotate(image [n, n], angle)`` with reshape=True, float64, in rotate's own
    sequence of operations (the matrix products included, so the doubles are the ones scipy forms on this machine)."""
    special = _special()
    c, s = special.cosdg(angle), special.sindg(angle)
    rot = np.array([[c, s], [-s, c]])
    in_shape = np.asarray((n, n))
    bounds = rot @ [[0, 0, n, n], [0, n, 0, n]]
    shape = (np.ptp(bounds, axis=1) + 0.5).astype(int)
    offset = (in_shape - 1) / 2 - rot @ ((shape - 1) / 2)
    return rot, offset, shape


def _rotation_struct(angle, n):
    rot, offset, shape = rotation(angle, n)
    return Rotation((ctypes.c_double * 4)(*rot.reshape(-1)), (ctypes.c_double * 2)(*offset), (ctypes.c_int32 * 2)(*[int(x) for x in shape]))


def position_to_pixel_indices(position_x, position_y, image_shape):
    """Mapper.position_to_pixel_indices (envs.py:2391-2396) of one position, as Python ints."""
    pixel_i = np.floor(image_shape[0] / 2 - position_y * PIXELS_PER_METER).astype(np.int32)
    pixel_j = np.floor(image_shape[1] / 2 + position_x * PIXELS_PER_METER).astype(np.int32)
    return int(np.clip(pixel_i, 0, image_shape[0] - 1)), int(np.clip(pixel_j, 0, image_shape[1] - 1))


# The descriptor tables as numpy structured arrays: numpy derives the field offsets and the item size from the ctypes structures, so a
# table filled column by column has the bytes of the ctypes array filled entry by entry (tests/test_robot_arrays_cpu.py).
ROTATION, LOCAL_MAP, LOCAL_ROBOT, LOCAL_PROBLEM, LOCAL_CHANNEL = (np.dtype(t) for t in (Rotation, LocalMap, LocalRobot, LocalProblem, LocalChannel))
RAD_TO_DEG = 180.0 / math.pi     # math.degrees(x) is x * (180.0 / pi) in C doubles; headings * RAD_TO_DEG is that product elementwise


def as_ctypes(table, struct):
    """The ctypes array (struct * len(table)) over the bytes of a structured numpy table, without a copy: what lib.call takes."""
    return (struct * len(table)).from_buffer(table)


def rotation_many(angles, n):
    """`rotation(angle, n)` for every angle of a float64 array [K]: (R [K, 2, 2], offset [K, 2], shape [K, 2]), each row the doubles
    and ints `rotation` gives for that angle.  The sequence is rotation()'s own with every product left to numpy's matmul -- a
    restatement in plain arithmetic, or np.einsum, rounds differently."""
    special = _special()
    angles = np.asarray(angles, np.float64).reshape(-1)
    c, s = special.cosdg(angles), special.sindg(angles)
    rot = np.empty((len(angles), 2, 2))
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1] = c, s, -s, c
    bounds = rot @ [[0, 0, n, n], [0, n, 0, n]]
    shape = (np.ptp(bounds, axis=2) + 0.5).astype(int)
    half = (shape - 1) / 2
    offset = (n - 1) / 2 - (rot @ half[:, :, None])[:, :, 0]
    return rot, offset, shape


def rotation_table(angles, n):
    """rotation_many as a ROTATION table [K]."""
    rot, offset, shape = rotation_many(angles, n)
    table = np.zeros(len(rot), ROTATION)
    table['r'], table['offset'], table['shape'] = rot.reshape(-1, 4), offset, shape
    return table


def pixel_indices_many(x, y, shape):
    """`position_to_pixel_indices` elementwise: int32 arrays (pixel_i, pixel_j) for float64 arrays x, y; shape: (rows, cols), each one
    int for all positions or an int array with one entry per position.  Product, difference, floor and clip are one ufunc call each, so
    no two of them contract into a fused multiply-add."""
    rows, cols = shape
    scaled_y, scaled_x = np.multiply(y, PIXELS_PER_METER), np.multiply(x, PIXELS_PER_METER)
    pixel_i = np.floor(np.subtract(rows / 2, scaled_y)).astype(np.int32)
    pixel_j = np.floor(np.add(cols / 2, scaled_x)).astype(np.int32)
    # (np.clip on whole numbers, without its per-call set-up)
    return (np.minimum(np.maximum(pixel_i, 0), rows - 1).astype(np.int32, copy=False),
            np.minimum(np.maximum(pixel_j, 0), cols - 1).astype(np.int32, copy=False))


def distances(dx, dy):
    """math.sqrt(dx**2 + dy**2) elementwise.  Python's `** 2` is libm's pow, which np.float_power(x, 2.0) matches and x * x does not."""
    return np.sqrt(np.float_power(dx, 2.0) + np.float_power(dy, 2.0))


def _is_spec(x):
    return isinstance(x, str) or (isinstance(x, (tuple, list)) and len(x) >= 1 and isinstance(x[0], str))


def _channel(spec, n_maps):
    name, arg = (spec, None) if isinstance(spec, str) else (spec[0], spec[1] if len(spec) > 1 else None)
    if name not in KINDS or (not isinstance(spec, str) and len(spec) > 2):
        raise ValueError('a channel is (kind, argument) with kind one of %s, got %r' % (sorted(KINDS), spec))
    if name == 'robots':
        if arg is not None:
            raise ValueError("the 'robots' channel takes no argument, got %r" % (spec,))
        return LocalChannel(KINDS[name], 0, 0.0, 0), None
    if arg is None:
        raise ValueError('channel %r needs %s' % (spec, 'a value' if name == 'constant' else 'the index of a map'))
    if name == 'constant':
        return LocalChannel(KINDS[name], 0, float(arg), 0), None
    k = int(arg)
    if not 0 <= k < n_maps:
        raise ValueError('channel %r names map %d of %d' % (spec, k, n_maps))
    return LocalChannel(KINDS[name], k, 0.0, 0), k


def local_state_images(maps, channels, poses, robots=None, masks=None, out=None, map_shape=None, into=None, pools=None):
    """The [P, 96, 96, C] float32 states of P robots in one launch.

    maps: a sequence of global maps [rows, cols] float32 -- device tensors are read in place (rows of one [G, rows, cols] tensor
    included, e.g. what grid_distance_images returned), numpy arrays are uploaded; or one such [G, rows, cols] tensor / array.
    poses: P pairs (position, heading) of the robots the states belong to; position = (x, y[, z]) in meters, converted with
    Mapper.position_to_pixel_indices (envs.py:2391-2396).
    channels: for every problem its C channels, or one list of C channels used by all problems.  A channel is
      ('map', k)       Mapper._get_local_map(maps[k])                                               envs.py:2199-2210
      ('distance', k)  Mapper._get_local_distance_map(maps[k]): minus the local image's minimum      envs.py:2212-2215
      'robots'         _get_local_map(_create_global_robot_map(seg=False))                          envs.py:2250-2275
      ('overhead', k)  _get_local_map(_create_global_overhead_map()), maps[k] the map without robots envs.py:2243-2248
      ('constant', v)  v everywhere (the nonspatial intention channels)                             envs.py:2368-2375
    robots: for every problem the RobotStamp sequence of its environment (problems of one environment may share one list object, which is
    then described to the device once), or None when no channel draws robots.  masks: the bank [M, 96, 96] float32 the stamps index
    (Mapper.robot_masks), numpy or device tensor.  map_shape: (rows, cols) of the global maps for problems whose channels name no map
    (one pair, or P pairs).
    out: a contiguous float32 device tensor [P, 96, 96, C] to write into -- a slice of a replay ring's `states`, a batch buffer.
    into: instead of `out`, P handles of one AliasedDeviceReplayBuffer (reserve(P)) whose states have C channels: state p is written
    into the pool slot of into[p] (simq_local_state_images_slots), inside the pool's stream order, and the handles are returned.  A
    pool of bf16 states (dtype='bf16') receives the fp32 state rounded once to nearest even (simq_local_state_images_slots_bf16).
    pools: with `into`, 1 to 16 distinct AliasedDeviceReplayBuffers of C channels on one device, of any mix of dtype: the handles may
    then belong to any of them, in any interleaving, and state p goes into the slot of into[p] in its own pool -- still one launch
    (simq_local_state_images_pools, also for one listed pool), inside the stream order of every pool that receives a state.

    Raises SimqError, launching nothing, when the 136 x 136 crop around a robot or the stamp of a robot leaves its map (the reference
    would silently wrap or clip the slice), and for any other descriptor the library refuses."""
    check_pools_argument('local_state_images', out, into, pools)
    if into is None:
        args, out, keep = _prepare(maps, channels, poses, robots, masks, out, map_shape)
        lib.call('simq_local_state_images', *args)
        del keep                                 # (uploaded maps / masks / descriptors: alive until the launch is queued)
        return out
    if out is not None:
        raise ValueError('local_state_images: `into` and `out` name two destinations; pass one')
    poses = list(poses)
    count = None
    if pools is not None:                        # (the listed rings are checked against the channel count before a device is asked for)
        channels = list(channels)
        count = len(channels) if all(_is_spec(c) for c in channels) else len(channels[0]) if channels else 0
    into, pool = check_into(into, 'local_state_images', len(poses), count, pools=pools)
    args, _, keep = _prepare(maps, channels, poses, robots, masks, None, map_shape, into=into, pools=pools)
    write_into(pool, into, args)
    del keep
    return into


def check_pools_argument(what, out, into, pools):
    """`pools=` lists the rings that `into=`'s handles belong to: ValueError where it comes with `out` or without `into`."""
    if pools is not None and out is not None:
        raise ValueError('%s: `pools` lists the rings of `into`; `out` is a tensor of its own: pass one destination' % what)
    if pools is not None and into is None:
        raise ValueError('%s: `pools` without `into`: the handles say which slot of which pool a state goes to' % what)


def check_into(into, what, count=None, channels=None, pools=None):
    """(handles, their pool) of an `into=` argument; ValueError for anything but distinct live handles of one pool (and, once the
    caller knows them, `count` of them for states of `channels` channels).  pools (not None): (handles, the listed pools as a list),
    the handles each of one of them (learner.pools_of)."""
    from .learner import pool_of, pools_of
    into = list(into)
    if pools is not None:
        return into, pools_of(into, pools, count, channels, '%s(into=, pools=)' % what)
    return into, pool_of(into, count, channels, '%s(into=)' % what)


def rings(pool):
    """check_into's second result as a list of rings."""
    return pool if isinstance(pool, list) else [pool]


def write_into(pool, handles, args):
    """simq_local_state_images_slots for _prepare(into=)'s arguments: the slot table and the scratch come from the pool, which puts the
    launch into its stream order.  pool a list (check_into(pools=)): simq_local_state_images_pools, one call for all of them."""
    n_maps, n_robots, P, C = args[1], args[5], args[7], args[9]
    if isinstance(pool, list):
        from .learner import AliasedDeviceReplayBuffer
        AliasedDeviceReplayBuffer.write_pool_slots('simq_local_state_images_pools', pool, handles, lambda table, dests, d_desc: args[:10] + (
            table, len(table), dests, ptr(d_desc), ctypes.c_int64(d_desc.numel()), stream_ptr(d_desc.device)),
            lib.c.simq_local_state_pools_desc_bytes(n_maps, n_robots, P, C, len(pool)))
        return
    # (a pool of bf16 states: the entry that rounds every element once as it stores it)
    entry = 'simq_local_state_images_slots_bf16' if pool.pool.dtype == torch.bfloat16 else 'simq_local_state_images_slots'
    pool.write_slots(entry, handles, lambda slots, d_desc: args[:10] + (
        slots, ptr(d_desc), ctypes.c_int64(d_desc.numel()), ptr(pool.pool), ctypes.c_int64(pool.pool.shape[0]), stream_ptr(pool.pool.device)),
        lib.c.simq_local_state_slots_desc_bytes(n_maps, n_robots, P, C))


def _prepare(maps, channels, poses, robots, masks, out, map_shape, into=None, pools=None):
    """The argument tuple of simq_local_state_images for local_state_images' inputs, the output tensor and the device tensors the
    call reads (tools/local_maps_rate.py times the library call alone with it).  into (checked handles of one pool): no output tensor
    and no descriptor scratch are made; the first ten arguments are those of simq_local_state_images_slots (write_into).  pools:
    check_into's, for handles of several pools."""
    dev = _batch.device('local state images')
    maps, _ = _batch.as_maps(maps, 'maps', _batch.check_map)      # (numpy maps are uploaded, device tensors read in place)
    poses = list(poses)
    P = len(poses)
    if P < 1:
        raise ValueError('local_state_images needs at least one pose')
    channels = list(channels)
    if channels and all(_is_spec(c) for c in channels):
        channels = [channels] * P
    if len(channels) != P:
        raise ValueError('%d channel lists for %d poses' % (len(channels), P))
    C = len(channels[0])
    if C < 1 or any(len(c) != C for c in channels):
        raise ValueError('every problem needs the same number (>= 1) of channels')
    if robots is not None and len(robots) != P:
        raise ValueError('%d robot lists for %d poses' % (len(robots), P))

    # maps: device tensors as they are, numpy ones uploaded (kept alive until the launch is queued)
    d_maps = [m if isinstance(m, torch.Tensor) and m.device == dev else
              (m.to(dev) if isinstance(m, torch.Tensor) else torch.from_numpy(m).to(dev)) for m in maps]
    c_maps = (LocalMap * max(len(d_maps), 1))()
    for k, m in enumerate(d_maps):
        c_maps[k] = LocalMap(m.data_ptr(), m.shape[0], m.shape[1])

    c_chans = (LocalChannel * (P * C))()
    shapes = []
    for p, specs in enumerate(channels):
        shape = None
        for c, spec in enumerate(specs):
            c_chans[p * C + c], k = _channel(spec, len(d_maps))
            if k is not None and shape is None:
                shape = tuple(d_maps[k].shape)
        if map_shape is not None:
            one = map_shape if np.ndim(map_shape) == 1 else map_shape[p]
            given = (int(one[0]), int(one[1]))
            if shape is not None and shape != given:
                raise ValueError('problem %d: map_shape %s but its maps are %s' % (p, given, shape))
            shape = given
        if shape is None:
            raise ValueError('problem %d names no map: pass map_shape=(rows, cols)' % p)
        shapes.append(shape)

    # robots: each distinct list object once
    c_robots_list, env_range = [], {}
    ranges = []
    for p in range(P):
        env = robots[p] if robots is not None else None
        if not env:
            ranges.append((0, 0))
            continue
        key = (id(env), shapes[p])
        if key not in env_range:
            begin = len(c_robots_list)
            for st in env:
                st = st if isinstance(st, RobotStamp) else RobotStamp(*st)
                pi, pj = position_to_pixel_indices(st.position[0], st.position[1], shapes[p])
                c_robots_list.append(LocalRobot(_rotation_struct(math.degrees(st.heading) - 90, WIDTH), pi, pj, int(st.mask),
                                                float(st.seg_value), float(st.map_value),
                                                int(st.mask if st.seg_mask is None else st.seg_mask)))
            env_range[key] = (begin, len(c_robots_list) - begin)
        ranges.append(env_range[key])
    n_robots = len(c_robots_list)
    c_robots = (LocalRobot * max(n_robots, 1))(*c_robots_list)
    d_masks, n_masks = None, 0
    if masks is not None:
        if isinstance(masks, torch.Tensor):
            if masks.dtype != torch.float32 or masks.dim() != 3 or tuple(masks.shape[1:]) != (WIDTH, WIDTH) or not masks.is_contiguous():
                raise ValueError('masks must be a contiguous float32 [M, 96, 96] bank, got %s %s' % (masks.dtype, tuple(masks.shape)))
            d_masks = masks.to(dev)
        else:
            masks = np.ascontiguousarray(masks)
            if masks.dtype != np.float32 or masks.ndim != 3 or masks.shape[1:] != (WIDTH, WIDTH):
                raise ValueError('masks must be a float32 [M, 96, 96] bank, got %s %s' % (masks.dtype, masks.shape))
            d_masks = torch.from_numpy(masks).to(dev)
        n_masks = d_masks.shape[0]
    if n_robots and not n_masks:
        raise ValueError('robots need the bank of masks they index (masks=)')

    c_probs = (LocalProblem * P)()
    for p, (pose, shape, (begin, count)) in enumerate(zip(poses, shapes, ranges)):
        try:
            position, heading = pose
            x, y = position[0], position[1]
        except (TypeError, ValueError, IndexError):
            raise ValueError('a pose is ((x, y), heading), got %r' % (pose,)) from None
        pi, pj = position_to_pixel_indices(x, y, shape)
        c_probs[p] = LocalProblem(_rotation_struct(90 - math.degrees(heading), CROP), pi, pj, shape[0], shape[1], begin, count)

    want = (P, WIDTH, WIDTH, C)
    if into is not None:
        check_into(into, 'local_state_images', P, C, pools)
        return (c_maps if d_maps else None, len(d_maps), ptr(d_masks), n_masks, c_robots if n_robots else None, n_robots, c_probs, P, c_chans,
                C), None, (d_maps, d_masks)
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=dev)
    elif not _batch.out_fits(out, torch.float32, dev, want):
        raise ValueError('out must be a contiguous float32 tensor of shape %s on %s' % (want, dev))
    desc_bytes = lib.c.simq_local_state_desc_bytes(len(d_maps), n_robots, P, C)
    d_desc = torch.empty(max(int(desc_bytes), 8), dtype=torch.uint8, device=dev)
    args = (c_maps if d_maps else None, len(d_maps), ptr(d_masks), n_masks, c_robots if n_robots else None, n_robots, c_probs, P, c_chans, C,
            ptr(d_desc), ctypes.c_int64(d_desc.numel()), ptr(out), ctypes.c_int64(out.numel()), stream_ptr(dev))
    return args, out, (d_maps, d_masks, d_desc)


def local_map(global_map, position, heading):
    """Drop-in for Mapper._get_local_map (envs.py:2199-2210) with the robot's pose passed in: the float32 [96, 96] numpy image."""
    return local_state_images([global_map], [('map', 0)], [(position, heading)])[0, :, :, 0].cpu().numpy()


def local_distance_map(global_map, position, heading):
    """Drop-in for Mapper._get_local_distance_map (envs.py:2212-2215): local_map minus its minimum."""
    return local_state_images([global_map], [('distance', 0)], [(position, heading)])[0, :, :, 0].cpu().numpy()
