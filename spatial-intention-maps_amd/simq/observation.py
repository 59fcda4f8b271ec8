"""Observation maps on the GPU: a camera frame into the persistent overhead and occupancy maps.

The reference turns the simulator's depth buffer and body-id segmentation into a point cloud (``Camera.capture_image``,
envs.py:1926-1954), sorts the points by height and scatters their segmentation values into ``global_overhead_map_without_robots``
(``Mapper.update``, envs.py:2053-2061) and the obstacle points into ``occupancy_map`` (``OccupancyMap.update``, envs.py:2444-2449), per
robot per step, on the host.  ``simq_observation_update`` (csrc/observation_maps.hip) does it for many frames in one launch, updating
both maps in place on the device, bit for bit equal to that sequence; the rules are stated in include/simq.h.  The updated occupancy
map is what ``simq.occupancy_maps`` reads and the overhead map is the base map of the ``overhead`` channel of
``simq.local_state_images``: neither ever needs to be a host array.  ``simq_observation_update_sequences`` applies several frames per
pair of maps in one launch, in the order given (``observation_update_sequences``; ``BatchedMapper.defer`` / ``flush`` use it).

The camera's unit vectors and pixel tables are formed here, on the host, in the reference's own sequence of numpy float32 operations
(``camera_geometry``); the library has no trigonometry and no normalisation.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _batch
from ._lib import SimqError, lib, ptr, stream_ptr

MAX_POINTS = 1 << 22             # SIMQ_OBSERVATION_MAX_POINTS of include/simq.h
MAX_SEQUENCE = 1023              # SIMQ_OBSERVATION_MAX_SEQUENCE: the frames of one map in one launch

# What the projection of one camera pose needs: float32 vectors [3], the tables pixel_x [width] and pixel_y [height], and the three
# depth constants far * near, far, far - near as float32.
CameraGeometry = collections.namedtuple('CameraGeometry', ('position', 'principal', 'right', 'up', 'pixel_x', 'pixel_y', 'far_near', 'far',
                                                           'far_minus_near'))
# The body ids Camera._ensure_initialized collects (envs.py:1911-1915); receptacle None: an environment without one.
IdRanges = collections.namedtuple('IdRanges', ('min_obstacle', 'max_obstacle', 'receptacle', 'min_cube', 'max_cube'))


class ObservationProblem(ctypes.Structure):
    """simq_observation_problem of include/simq.h."""
    _fields_ = [('depth_offset', ctypes.c_int64), ('ids_offset', ctypes.c_int64), ('px_offset', ctypes.c_int64), ('py_offset', ctypes.c_int64),
                ('overhead_offset', ctypes.c_int64), ('occupancy_offset', ctypes.c_int64),
                ('cam', ctypes.c_float * 3), ('principal', ctypes.c_float * 3), ('right', ctypes.c_float * 3), ('up', ctypes.c_float * 3),
                ('far_near', ctypes.c_float), ('far', ctypes.c_float), ('far_minus_near', ctypes.c_float),
                ('min_obstacle', ctypes.c_int32), ('max_obstacle', ctypes.c_int32), ('receptacle', ctypes.c_int32),
                ('has_receptacle', ctypes.c_int32), ('min_cube', ctypes.c_int32), ('max_cube', ctypes.c_int32),
                ('height', ctypes.c_int32), ('width', ctypes.c_int32), ('rows', ctypes.c_int32), ('cols', ctypes.c_int32),
                ('reserved_', ctypes.c_int32)]


def camera_geometry(camera_position, camera_target, camera_up, near, far, aspect, image_height, fov=60):
    """The CameraGeometry of one camera pose: what Camera._get_camera_params returns (position, target, up), the class's NEAR, FAR and
    ASPECT, Camera.image_pixel_height and Camera.FOV (degrees, vertical).  Every array is float32 and is formed in the sequence of numpy
    operations of envs.py:1931-1943, so the values are the ones the reference multiplies the depth with on this machine; the image
    width is int(aspect * image_height) as in Camera.__init__ (envs.py:1895)."""
    near, far, aspect, fov = float(near), float(far), float(aspect), float(fov)   # (Python scalars, as the class constants are)
    height = int(image_height)
    width = int(aspect * height)
    if height < 1 or width < 1:
        raise ValueError('camera_geometry: an image of %d x %d' % (height, width))
    position = np.array(camera_position, dtype=np.float32)
    principal = np.array(camera_target, dtype=np.float32) - position
    principal = principal / np.linalg.norm(principal)
    up = np.array(camera_up, dtype=np.float32)
    up = up - np.dot(up, principal) * principal
    up = up / np.linalg.norm(up)
    right = np.cross(principal, up)
    right = right / np.linalg.norm(right)
    limit_y = math.tan(math.radians(fov / 2))
    limit_x = limit_y * aspect
    pixel_x = (2 * limit_x) * (np.arange(width, dtype=np.float32) / width - 0.5)
    pixel_y = (2 * limit_y) * (0.5 - (np.arange(height, dtype=np.float32) + 1) / height)
    arrays = [np.ascontiguousarray(a, np.float32) for a in (position, principal, right, up, pixel_x, pixel_y)]
    for a, shape in zip(arrays, ((3,), (3,), (3,), (3,), (width,), (height,))):
        if a.shape != shape:
            raise ValueError('camera_geometry: position, target and up are 3-vectors')
    # a Python scalar meets the float32 depth buffer as a float32 (envs.py:1928)
    return CameraGeometry(*arrays, np.float32(far * near), np.float32(far), np.float32(far - near))


def _frames(frames, dtype, what):
    """The 2-D frames of a sequence or of one [P, height, width] array / tensor (and as_maps' block, which the interleaved layout of
    depth and id frames has no use for)."""
    return _batch.as_maps(frames, what, lambda f, name: _batch.check_map(f, name, dtype),
                          'a sequence of 2-D %s frames or one [P, height, width] array' % dtype.__name__)


def _maps(maps, tdtype, dev, what):
    """The 2-D device maps of one [P, rows, cols] tensor or of a sequence of 2-D tensors: updated in place, so nothing is copied."""
    if isinstance(maps, torch.Tensor):
        if maps.dim() != 3:
            raise ValueError('%s is one [P, rows, cols] device tensor or a sequence of 2-D device tensors, got %d dimensions' % (what, maps.dim()))
    elif isinstance(maps, np.ndarray):
        raise ValueError('%s must live on the device: it is updated in place (simq.observe takes numpy maps)' % what)
    try:
        maps = list(maps)
    except TypeError:
        raise ValueError('%s is one [P, rows, cols] device tensor or a sequence of 2-D device tensors, got %s' % (what, type(maps).__name__)) from None
    for k, m in enumerate(maps):
        if not isinstance(m, torch.Tensor) or m.dtype != tdtype or m.dim() != 2 or not m.is_contiguous() or m.device != dev:
            raise ValueError('%s[%d] must be a 2-D contiguous %s tensor on %s, updated in place' % (what, k, str(tdtype).replace('torch.', ''), dev))
    return maps


def _per_problem(values, P, cls, what):
    if isinstance(values, cls):
        return [values] * P
    values = list(values)
    if len(values) != P or not all(isinstance(v, cls) for v in values):
        raise ValueError('%s is one %s or one per frame (%d frames)' % (what, cls.__name__, P))
    return values


def _checked_frames(depth, ids, geometries, id_ranges, entry='observation_update'):
    """The frames, geometries and id ranges of a call as lists of P, checked as far as no device is needed."""
    depth, _ = _frames(depth, np.float32, 'depth')
    ids, _ = _frames(ids, np.int32, 'ids')
    P = len(depth)
    if P < 1 or len(ids) != P:
        raise ValueError('%s needs at least one frame and as many id frames as depth frames (%d, %d)' % (entry, P, len(ids)))
    return depth, ids, _per_problem(geometries, P, CameraGeometry, 'geometries'), _per_problem(id_ranges, P, IdRanges, 'id_ranges'), P


def _layout(depth, ids, geometries):
    """One buffer of 4-byte words: each distinct geometry's tables once, then every frame's depth and ids.  Returns the arrays in that
    order, their word count, {id(geometry): (px_offset, py_offset)} and per frame (depth_offset, ids_offset)."""
    P = len(depth)
    tables, words, parts = {}, 0, []
    for g in geometries:
        if id(g) not in tables:
            tables[id(g)] = (words, words + g.pixel_x.size)
            parts += [np.ascontiguousarray(g.pixel_x, np.float32), np.ascontiguousarray(g.pixel_y, np.float32)]
            words += g.pixel_x.size + g.pixel_y.size
    offsets = []
    for p in range(P):
        shape = tuple(depth[p].shape)
        if tuple(ids[p].shape) != shape or shape != (geometries[p].pixel_y.size, geometries[p].pixel_x.size):
            raise ValueError('frame %d: depth %s, ids %s, but its geometry is for %d x %d images' % (
                p, shape, tuple(ids[p].shape), geometries[p].pixel_y.size, geometries[p].pixel_x.size))
        n = shape[0] * shape[1]
        if n < 1 or n > MAX_POINTS:
            raise ValueError('frame %d: %d x %d (1 .. %d points)' % (p, shape[0], shape[1], MAX_POINTS))
        offsets.append((words, words + n))
        parts += [depth[p], ids[p]]
        words += 2 * n
    return parts, words, tables, offsets


def _map_bases(overhead_maps, occupancy_maps):
    """The maps where they are: offsets from the lowest address of each kind.  Returns (base_o, overhead_floats, base_c, occupancy_bytes)."""
    base_o = min(m.data_ptr() for m in overhead_maps)
    base_c = min(m.data_ptr() for m in occupancy_maps)
    if any((m.data_ptr() - base_o) % 4 for m in overhead_maps):
        raise ValueError('overhead_maps: the maps must be 4-byte aligned to each other')
    overhead_floats = max((m.data_ptr() - base_o) // 4 + m.numel() for m in overhead_maps)
    occupancy_bytes = max(m.data_ptr() - base_c + m.numel() for m in occupancy_maps)
    return base_o, overhead_floats, base_c, occupancy_bytes


def _describe(q, g, r, frame_at, table_at, frame_shape, overhead_offset, occupancy_offset, map_shape):
    """Fills the ObservationProblem q: the frame at word offsets frame_at = (depth, ids) with its tables at table_at = (px, py)."""
    q.depth_offset, q.ids_offset = frame_at
    q.px_offset, q.py_offset = table_at
    q.overhead_offset, q.occupancy_offset = overhead_offset, occupancy_offset
    for name, v in (('cam', g.position), ('principal', g.principal), ('right', g.right), ('up', g.up)):
        setattr(q, name, (ctypes.c_float * 3)(*[float(x) for x in v]))
    q.far_near, q.far, q.far_minus_near = float(g.far_near), float(g.far), float(g.far_minus_near)
    q.min_obstacle, q.max_obstacle, q.min_cube, q.max_cube = int(r.min_obstacle), int(r.max_obstacle), int(r.min_cube), int(r.max_cube)
    q.has_receptacle = 0 if r.receptacle is None else 1
    q.receptacle = 0 if r.receptacle is None else int(r.receptacle)
    q.height, q.width = frame_shape
    q.rows, q.cols = map_shape


def _prepare(depth, ids, geometries, id_ranges, overhead_maps, occupancy_maps):
    """The argument tuple of simq_observation_update, the status tensor and the device tensors the call reads
    (tools/observation_maps_rate.py times the upload and the library call with it)."""
    depth, ids, geometries, id_ranges, P = _checked_frames(depth, ids, geometries, id_ranges)
    dev = _batch.device('observation maps')
    overhead_maps = _maps(overhead_maps, torch.float32, dev, 'overhead_maps')
    occupancy_maps = _maps(occupancy_maps, torch.uint8, dev, 'occupancy_maps')
    if len(overhead_maps) != P or len(occupancy_maps) != P:
        raise ValueError('%d frames but %d overhead maps and %d occupancy maps' % (P, len(overhead_maps), len(occupancy_maps)))
    parts, words, tables, offsets = _layout(depth, ids, geometries)
    frames, _ = _batch.pack(parts, torch.int32, dev)
    base_o, overhead_floats, base_c, occupancy_bytes = _map_bases(overhead_maps, occupancy_maps)
    probs = (ObservationProblem * P)()
    for p in range(P):
        om, cm = overhead_maps[p], occupancy_maps[p]
        if tuple(om.shape) != tuple(cm.shape):
            raise ValueError('problem %d: an overhead map of %s but an occupancy map of %s' % (p, tuple(om.shape), tuple(cm.shape)))
        _describe(probs[p], geometries[p], id_ranges[p], offsets[p], tables[id(geometries[p])], depth[p].shape,
                  (om.data_ptr() - base_o) // 4, cm.data_ptr() - base_c, om.shape)
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    args = (ptr(frames), ctypes.c_int64(words), probs, P, ptr(d_probs), ctypes.c_void_p(base_o), ctypes.c_int64(overhead_floats),
            ctypes.c_void_p(base_c), ctypes.c_int64(occupancy_bytes), ptr(status), stream_ptr(dev))
    return args, status, (frames, d_probs, overhead_maps, occupancy_maps)


def _enqueue(depth, ids, geometries, id_ranges, overhead_maps, occupancy_maps):
    """observation_update without its status read-back: queues the launch and returns the int32 device tensor it writes.  (The frames
    and descriptors it uploaded may go as soon as the launch is queued: the allocator hands their memory to work of this stream only.)"""
    args, status, keep = _prepare(depth, ids, geometries, id_ranges, overhead_maps, occupancy_maps)
    lib.call('simq_observation_update', *args)
    del keep
    return status


def observation_update(depth, ids, geometries, id_ranges, overhead_maps, occupancy_maps):
    """Mapper.update (envs.py:2053-2065) for P camera frames in one launch: both maps of every problem are updated in place on the device.

    depth: P depth buffers [height, width] float32 as the simulator returns them (numpy arrays, uploaded; or contiguous device tensors),
    or one [P, height, width] array / tensor; frames of different cameras may be mixed.  ids: the same for the body-id segmentation,
    int32.  geometries: one CameraGeometry (camera_geometry) per frame, or one for all; frames that share a geometry object share its
    tables on the device.  id_ranges: one IdRanges per frame, or one for all.  overhead_maps: one float32 [P, rows, cols] device tensor
    or P 2-D float32 device tensors of any shapes (Mapper.global_overhead_map_without_robots); occupancy_maps: the same in uint8
    (OccupancyMap.occupancy_map), each of its overhead map's shape.  Nothing but the frames, the tables and the descriptors is uploaded.

    Separately allocated maps are described to the library as offsets from the lowest address of their kind, so the buffer it is told
    of reaches from the lowest map to the end of the highest and takes in whatever the allocator placed between them.  The library
    checks and writes the maps' own spans only, but it refuses a buffer of 2^40 elements or more: maps of one call whose allocations
    lie that far apart (in practice: on different devices or in different address ranges) must go into one tensor or into two calls.

    Returns (overhead_maps, occupancy_maps) as given.  Raises ValueError for a wrong dtype, rank, contiguity or device, SimqError for
    what the library refuses (two problems naming one map among it; nothing is launched) and for the frames that held a point that is
    not finite: their maps are unchanged, every other problem of the call is updated."""
    status = _enqueue(depth, ids, geometries, id_ranges, overhead_maps, occupancy_maps)
    bad, codes = _batch.bad_problems(status)
    if bad.size:
        if (codes == 1).all():
            raise SimqError('simq_observation_update: %d frame(s) hold a point that is not finite (a depth buffer outside what the near and far '
                            'planes allow); their maps are unchanged (problems %s)' % (bad.size, bad[:8].tolist()))
        raise SimqError('simq_observation_update: %d problem(s) failed (status %s at problems %s)' % (bad.size, codes[:8].tolist(), bad[:8].tolist()))
    return overhead_maps, occupancy_maps


def sequence_launches(map_index):
    """How frames that name the maps `map_index` (ints, in the order the frames are given) go into launches of
    simq_observation_update_sequences: a list of (frames, begin) -- `frames` the positions of the launch's frames in `map_index`, map by
    map and within a map in the order given (a stable sort), `begin` the int32 table of its sequences.  A map with more than
    MAX_SEQUENCE frames continues in the next launch, so launch l holds of every map its frames l * MAX_SEQUENCE .. of that order."""
    index = np.asarray(map_index, np.int64)
    order = np.argsort(index, kind='stable')
    by_map = index[order]
    first = np.flatnonzero(np.concatenate([[True], by_map[1:] != by_map[:-1]]))          # where each map's frames begin in `order`
    rank = np.arange(len(order)) - np.repeat(first, np.diff(np.concatenate([first, [len(order)]])))
    out = []
    for l in range(int(rank.max()) // MAX_SEQUENCE + 1):
        mine = rank // MAX_SEQUENCE == l
        frames, maps = order[mine], by_map[mine]
        begin = np.concatenate([[0], np.flatnonzero(maps[1:] != maps[:-1]) + 1, [len(frames)]]).astype(np.int32)
        out.append((frames, begin))
    return out


def call_sequences(frames, words, probs, begin, bases, status, dev):
    """One simq_observation_update_sequences launch: the descriptors `probs` (ObservationProblem array) and the table `begin` (int32
    array) go up in the call; `status` is the int32 device tensor of len(probs) words it writes."""
    begin = np.ascontiguousarray(begin, np.int32)
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    d_begin = torch.empty(len(begin), dtype=torch.int32, device=dev)
    base_o, overhead_floats, base_c, occupancy_bytes = bases
    lib.call('simq_observation_update_sequences', ptr(frames), ctypes.c_int64(words), probs, len(probs), begin.ctypes.data_as(ctypes.c_void_p),
             len(begin) - 1, ptr(d_probs), ptr(d_begin), ctypes.c_void_p(base_o), ctypes.c_int64(overhead_floats), ctypes.c_void_p(base_c),
             ctypes.c_int64(occupancy_bytes), ptr(status), stream_ptr(dev))


def _enqueue_sequences(depth, ids, geometries, id_ranges, overhead_maps, occupancy_maps, map_index):
    """observation_update_sequences without its status read-back: returns the int32 device tensor of one word per frame in the order
    of the launches, and the position of every frame of the call in it."""
    depth, ids, geometries, id_ranges, P = _checked_frames(depth, ids, geometries, id_ranges, 'observation_update_sequences')
    try:
        index = [int(k) for k in map_index]
    except TypeError:
        raise ValueError('map_index holds the map of each frame, got %s' % type(map_index).__name__) from None
    if len(index) != P:
        raise ValueError('map_index holds the map of each frame: %d entries for %d frames' % (len(index), P))
    dev = _batch.device('observation maps')
    overhead_maps = _maps(overhead_maps, torch.float32, dev, 'overhead_maps')
    occupancy_maps = _maps(occupancy_maps, torch.uint8, dev, 'occupancy_maps')
    G = len(overhead_maps)
    if G < 1 or len(occupancy_maps) != G:
        raise ValueError('%d overhead maps and %d occupancy maps: one pair per map' % (G, len(occupancy_maps)))
    if min(index) < 0 or max(index) >= G:
        raise ValueError('map_index names maps in 0 .. %d, got %s' % (G - 1, [k for k in index if k < 0 or k >= G][:8]))
    for k, (om, cm) in enumerate(zip(overhead_maps, occupancy_maps)):
        if tuple(om.shape) != tuple(cm.shape):
            raise ValueError('map %d: an overhead map of %s but an occupancy map of %s' % (k, tuple(om.shape), tuple(cm.shape)))
    parts, words, tables, offsets = _layout(depth, ids, geometries)
    frames, _ = _batch.pack(parts, torch.int32, dev)
    bases = _map_bases(overhead_maps, occupancy_maps)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    where, at = np.empty(P, np.int64), 0
    for mine, begin in sequence_launches(index):
        probs = (ObservationProblem * len(mine))()
        for q, p in zip(probs, mine.tolist()):
            om, cm = overhead_maps[index[p]], occupancy_maps[index[p]]
            _describe(q, geometries[p], id_ranges[p], offsets[p], tables[id(geometries[p])], depth[p].shape, (om.data_ptr() - bases[0]) // 4,
                      cm.data_ptr() - bases[2], om.shape)
        call_sequences(frames, words, probs, begin, bases, status[at:at + len(mine)], dev)
        where[mine] = at + np.arange(len(mine))
        at += len(mine)
    return status, where


def observation_update_sequences(depth, ids, geometries, id_ranges, overhead_maps, occupancy_maps, map_index):
    """Mapper.update for P camera frames of G pairs of maps, P >= G, in one launch: what successive observation_update calls -- the
    frames of each map one after the other in the order given -- leave in the maps, bit for bit (include/simq.h: the last frame that
    reaches an overhead pixel decides it, an occupancy byte is the OR over the frames).

    depth, ids, geometries, id_ranges: as observation_update takes them, one per frame.  overhead_maps, occupancy_maps: one
    [G, rows, cols] device tensor or G 2-D device tensors each, as there.  map_index: the map pair of each frame, 0 .. G - 1.  The frames
    of one map are applied in the order they are given; frames of different maps may interleave (they are ordered by map with a stable
    sort).  A map with more than MAX_SEQUENCE frames is finished by successive launches.  A map no frame names is left alone.

    Returns (overhead_maps, occupancy_maps) as given, after one status read-back.  Raises ValueError and SimqError as observation_update
    does; a frame that holds a point that is not finite is skipped -- the other frames of its map are applied as if it were absent --
    and named, by its position in the call, in the SimqError raised after every other frame has been applied."""
    status, where = _enqueue_sequences(depth, ids, geometries, id_ranges, overhead_maps, occupancy_maps, map_index)
    codes = status.cpu().numpy()[where]                                                  # the one read-back; in the caller's order
    bad = np.flatnonzero(codes != 0)
    if bad.size:
        if (codes[bad] == 1).all():
            raise SimqError('simq_observation_update_sequences: %d frame(s) hold a point that is not finite (a depth buffer outside what the '
                            'near and far planes allow); they are skipped, every other frame is applied (frames %s)' % (bad.size, bad[:8].tolist()))
        raise SimqError('simq_observation_update_sequences: %d frame(s) failed (status %s at frames %s)'
                        % (bad.size, codes[bad][:8].tolist(), bad[:8].tolist()))
    return overhead_maps, occupancy_maps


def observe(depth, ids, geometry, id_ranges, overhead_map, occupancy_map):
    """Mapper.update for one frame and one pair of numpy maps (float32 and uint8 [rows, cols]): returns the two updated arrays, the
    arguments are left as they are."""
    dev = _batch.device('observation maps')
    for m, dtype, what in ((overhead_map, np.float32, 'overhead_map'), (occupancy_map, np.uint8, 'occupancy_map')):
        if not isinstance(m, np.ndarray) or m.dtype != dtype or m.ndim != 2:
            raise ValueError('%s must be a 2-D %s numpy array' % (what, dtype.__name__))
    om = torch.from_numpy(np.ascontiguousarray(overhead_map)).to(dev)
    cm = torch.from_numpy(np.ascontiguousarray(occupancy_map)).to(dev)
    observation_update([depth], [ids], geometry, id_ranges, [om], [cm])
    return om.cpu().numpy(), cm.cpu().numpy()
