"""simq.RobotArrays without a device: every vector form the array path of BatchedMapper.get_states is built from against the scalar
code of the list form, bit for bit -- rotation_many, pixel_indices_many, the distances, the closest-robot order, the segment tables --
the structured dtypes against the ctypes structures, from_states, and the refusals."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest
import torch

import mapper_oracle

RNG = np.random.RandomState(19)
SHAPES = ((184, 232), (232, 232))


@pytest.fixture(scope='module')
def episodes(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))
    assert len(files) == 2, files
    return [mapper_oracle.load_fixture(f) for f in files]


def build(episodes, **cfg):
    from simq import mapper
    masks = {name: episodes[0]['masks'][k] for k, name in enumerate(episodes[0]['mask_names'])}
    return mapper.BatchedMapper([f['room_width'] for f in episodes], [f['room_length'] for f in episodes], [f['types'] for f in episodes], masks,
                                [f['groups'] for f in episodes], [f['receptacle_position'] for f in episodes], **cfg)


def states_of(episodes, t):
    from simq import mapper
    return [[mapper.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'], r['history_path'])
             for r in ep['rounds'][t]['robots']] for ep in episodes]


# ---- rotations ------------------------------------------------------------------------------------------------------------------------
def same_rotations(lm, angles, n):
    rot, offset, shape = lm.rotation_many(angles, n)
    assert rot.dtype == offset.dtype == np.float64 and rot.shape == (len(angles), 2, 2) and offset.shape == shape.shape == (len(angles), 2)
    table = lm.rotation_table(angles, n)
    for k, a in enumerate(angles.tolist()):
        r, o, s = lm.rotation(a, n)
        assert r.tobytes() == rot[k].tobytes() and o.tobytes() == offset[k].tobytes() and s.tolist() == shape[k].tolist(), (n, a)
        assert bytes(lm._rotation_struct(a, n)) == table[k].tobytes(), (n, a)


@pytest.mark.parametrize('n', [96, 136])
def test_rotation_many_equals_rotation_bit_for_bit(n):
    from simq import local_maps as lm
    same_rotations(lm, RNG.uniform(-720, 720, 20000), n)
    same_rotations(lm, np.arange(-720.0, 720.5, 15.0), n)
    same_rotations(lm, np.array([0.0, -0.0]), n)
    headings = np.concatenate([-RNG.uniform(-math.pi, math.pi, 999), [math.pi]])           # (-pi, pi]
    degrees = headings * lm.RAD_TO_DEG
    assert degrees.tolist() == [math.degrees(h) for h in headings.tolist()]
    same_rotations(lm, 90 - degrees, n)
    same_rotations(lm, degrees - 90, n)
    assert (90 - degrees).tolist() == [90 - math.degrees(h) for h in headings.tolist()]


# ---- pixels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_pixel_indices_many_equals_position_to_pixel_indices(shape):
    from simq import local_maps as lm
    k = np.arange(-140, 141) / 96                                   # pixel boundaries
    x = np.concatenate([RNG.uniform(-1.2, 1.2, 4000), RNG.uniform(-30, 30, 500), [-0.0, 0.0, 0.5, -0.5, 1e6, -1e6], k, k[::-1]])
    y = np.concatenate([RNG.uniform(-1.2, 1.2, 4000), RNG.uniform(-30, 30, 500), [0.0, -0.0, -0.5, 0.5, -1e6, 1e6], k[::-1], k])
    i, j = lm.pixel_indices_many(x, y, shape)
    assert i.dtype == j.dtype == np.int32
    want = [lm.position_to_pixel_indices(a, b, shape) for a, b in zip(x.tolist(), y.tolist())]
    assert list(zip(i.tolist(), j.tolist())) == want
    assert (i == 0).any() and (i == shape[0] - 1).any() and (j == 0).any() and (j == shape[1] - 1).any()
    # one shape per position
    rows, cols = np.where(np.arange(len(x)) % 2, 184, 232).astype(np.int32), np.full(len(x), 232, np.int32)
    i2, j2 = lm.pixel_indices_many(x, y, (rows, cols))
    assert list(zip(i2.tolist(), j2.tolist())) == [lm.position_to_pixel_indices(a, b, (int(r), 232)) for a, b, r in zip(x.tolist(), y.tolist(), rows)]


# ---- distances and the closest-robot order ----------------------------------------------------------------------------------------------
def test_vector_distance_equals_the_scalar_one():
    from simq import local_maps as lm, mapper, intention_drawing
    a, b = RNG.uniform(-2, 2, (200000, 2)), RNG.uniform(-2, 2, (200000, 2))
    got = lm.distances(b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]).tolist()
    for k, (p, q) in enumerate(zip(a.tolist(), b.tolist())):
        assert got[k] == math.sqrt((q[0] - p[0])**2 + (q[1] - p[1])**2), k
    assert got[:500] == [mapper._distance(p, q) for p, q in zip(a[:500].tolist(), b[:500].tolist())]
    assert got[:500] == [intention_drawing._length(p, q) for p, q in zip(a[:500].tolist(), b[:500].tolist())]


def test_closest_order_rows_equal_argsort_of_the_list_forms_list():
    from simq import mapper
    P, R = 300, 5
    positions = RNG.uniform(-1, 1, (P, R, 2))
    positions[0] = [[0.0, 0.0], [0.25, 0.0], [-0.25, 0.0], [0.0, 0.25], [0.0, -0.25]]      # four robots equidistant from robot 0
    positions[1] = [[0.5, 0.5], [0.1, 0.2], [0.1, 0.2], [0.3, 0.1], [0.1, 0.2]]            # three robots on one spot
    positions[2, :, :] = 0.125                                                            # everyone on one spot
    own = RNG.randint(0, R, P)
    own[:3] = [0, 0, 3]
    me = positions[np.arange(P), own]
    got = mapper.closest_order(positions, me, own)
    assert got.shape == (P, R - 1)
    for p in range(P):
        mine = [tuple(w) for w in positions[p].tolist()]
        dists = [mapper._distance(mine[own[p]], other) for other in mine]
        assert got[p].tolist() == [int(k) for k in np.argsort(dists) if k != own[p]], p


# ---- segments ---------------------------------------------------------------------------------------------------------------------------
def packed(paths):
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return np.array([w for p in paths for w in p], np.float64).reshape(-1, 2), offsets


def scalar_table(idr, paths, shape, encoding, scale):
    rows = [s for path in paths for s in idr.segments([path], shape, encoding, scale)]
    return bytes((idr.Segment * max(len(rows), 1))(*[idr.Segment(start, stop, step, r0, c0, r1, c1, mode, drop, v, 0)
                                                      for r0, c0, r1, c1, mode, drop, v, start, stop, step in rows]))[:len(rows) * ctypes.sizeof(idr.Segment)]


@pytest.mark.parametrize('scale', [1.0, 0.7])
@pytest.mark.parametrize('shape', SHAPES)
def test_segment_tables_equal_segments_byte_for_byte(shape, scale):
    from simq import intention_drawing as idr
    way = lambda n: [tuple(w) for w in RNG.uniform(-0.6, 0.6, (n, 2)).tolist()]
    paths = [way(1), way(2), way(3) + way(1) * 2 + way(2), way(40), [(0.1, 0.2)] * 3, way(7), [(-5.0, 9.0), (5.0, -9.0)],
             [(0.010416666666666666, -0.0), (0.0, 0.020833333333333332), (0.0, 0.020833333333333332)]]
    paths[2][4] = paths[2][3]                                       # a repeated waypoint: a segment of no pixels' length (div = 0)
    points, offsets = packed(paths)
    for encoding in ('ramp', 'binary', 'line', 'history'):
        table, count = idr.path_segments(points, offsets[:-1], offsets[1:], shape[0], shape[1], encoding, scale)
        assert table.dtype == idr.SEGMENT and count.tolist() == [len(idr.segments([p], shape, encoding, scale)) for p in paths]
        assert table.tobytes() == scalar_table(idr, paths, shape, encoding, scale), encoding
        if encoding in ('ramp', 'history'):
            assert count[0] == 0 and count[3] == 39 and (table['step'] == 0.0).any()
        # a subset in another order, each path with its own map shape
        pick = np.array([3, 0, 5, 2])
        sub, n = idr.path_segments(points, offsets[pick], offsets[pick + 1], np.full(4, shape[0]), np.full(4, shape[1]), encoding, scale)
        assert sub.tobytes() == scalar_table(idr, [paths[k] for k in pick], shape, encoding, scale) and n.tolist() == count[pick].tolist()
    targets = np.array(way(50) + [(9.0, -9.0), (-0.0, 0.0)])
    table = idr.circle_segments(targets, shape[0], shape[1], scale)
    assert table.tobytes() == scalar_table(idr, [tuple(t) for t in targets.tolist()], shape, 'circle', scale)
    with pytest.raises(ValueError, match='empty waypoint list'):
        idr.path_segments(points, offsets[:2], offsets[:2], shape[0], shape[1], 'ramp', scale)
    assert idr.ragged([5, 0, 9], [2, 0, 3]).tolist() == [5, 6, 9, 10, 11]


# ---- the structured dtypes ----------------------------------------------------------------------------------------------------------------
def test_structured_dtypes_match_the_ctypes_structures():
    from simq import grid_paths, intention_drawing as idr, local_maps as lm

    def same(dtype, struct):
        assert dtype.itemsize == ctypes.sizeof(struct), struct
        assert set(dtype.names) == {name for name, _ in struct._fields_}, struct
        for name, ctype in struct._fields_:
            sub, offset = dtype.fields[name][:2]
            assert offset == getattr(struct, name).offset and sub.itemsize == ctypes.sizeof(ctype), (struct, name)
            if issubclass(ctype, ctypes.Structure):
                same(sub, ctype)
            elif issubclass(ctype, ctypes.Array):
                assert sub.shape == (ctype._length_,) and sub.base == np.dtype(ctype._type_), (struct, name)
            else:
                assert sub == np.dtype(ctype), (struct, name)
    pairs = ((lm.ROTATION, lm.Rotation), (lm.LOCAL_MAP, lm.LocalMap), (lm.LOCAL_ROBOT, lm.LocalRobot), (lm.LOCAL_PROBLEM, lm.LocalProblem),
             (lm.LOCAL_CHANNEL, lm.LocalChannel), (idr.SEGMENT, idr.Segment), (idr.PROBLEM, idr.Problem),
             (grid_paths.SNAPPED_PROBLEM, grid_paths.SnappedProblem))
    for dtype, struct in pairs:
        same(dtype, struct)
    # a table handed to the library is the array's own memory
    table = np.zeros(3, lm.LOCAL_CHANNEL)
    table['kind'], table['value'] = [4, 1, 0], [0.5, 0.0, -1.0]
    c = lm.as_ctypes(table, lm.LocalChannel)
    assert bytes(c) == table.tobytes() == bytes((lm.LocalChannel * 3)(lm.LocalChannel(4, 0, 0.5, 0), lm.LocalChannel(1, 0, 0.0, 0), lm.LocalChannel(0, 0, -1.0, 0)))
    assert ctypes.addressof(c) == table.ctypes.data


# ---- RobotArrays ------------------------------------------------------------------------------------------------------------------------
def test_from_states_round_trips_the_fixture(episodes):
    import simq
    from simq import mapper
    assert simq.RobotArrays is mapper.RobotArrays
    bm = build(episodes)
    lifting = []
    for t in range(len(episodes[0]['rounds'])):
        robots = states_of(episodes, t)
        ra = mapper.RobotArrays.from_states(bm, robots)
        assert ra.num_mappers == 6 and ra.position.dtype == ra.heading.dtype == np.float64 and ra.idle.dtype == ra.lifting.dtype == np.bool_
        flat = [r for env in robots for r in env]
        assert any(r.idle for r in flat)
        lifting += [r.lift_state == 'lifting' for r in flat]
        for m, r in enumerate(flat):
            assert tuple(ra.position[m].tolist()) == tuple(r.position[:2]) and ra.heading[m] == r.heading and ra.idle[m] == r.idle
            assert ra.lifting[m] == (r.lift_state == 'lifting')
            assert np.isnan(ra.target[m]).all() if r.target is None else tuple(ra.target[m].tolist()) == tuple(r.target[:2])
            for name in ('intention_path', 'history_path'):
                points, offsets = getattr(ra, name)
                assert [tuple(w) for w in points[offsets[m]:offsets[m + 1]].tolist()] == [tuple(w[:2]) for w in (getattr(r, name) or [])]
        # one environment left out: its rows are NaN, the other's are the same
        half = mapper.RobotArrays.from_states(bm, [None, robots[1]])
        assert np.isnan(half.position[:3]).all() and np.array_equal(half.position[3:], ra.position[3:])
        assert half.intention_path[1].tolist() == [0, 0, 0] + (ra.intention_path[1][3:] - ra.intention_path[1][3]).tolist()
    assert any(lifting) and not all(lifting)
    none = mapper.RobotArrays.from_states(bm, [[mapper.RobotState((0.0, 0.0), 0.0, None, None, True)] * 3] * 2)
    assert none.target is None and none.intention_path is None and none.history_path is None and none.idle.all()
    with pytest.raises(ValueError, match='Python floats and np.float64'):
        mapper.RobotArrays.from_states(bm, [[mapper.RobotState((np.float32(0.0), 0.0), 0.0, None, None, True)] * 3] * 2)
    with pytest.raises(ValueError, match='Python floats and np.float64'):
        mapper.RobotArrays.from_states(bm, [[mapper.RobotState((0.0, 0.0), 1, None, None, True)] * 3] * 2)
    with pytest.raises(ValueError, match='environment 1 has 3 robots, got 2 robot states'):
        mapper.RobotArrays.from_states(bm, [robots[0], robots[1][:2]])


def test_arrays_of_another_type_or_shape_are_refused():
    from simq.mapper import RobotArrays
    M = 4
    pos, head, flags = np.zeros((M, 2)), np.zeros(M), np.zeros(M, bool)
    points, offsets = np.zeros((5, 2)), np.array([0, 1, 1, 3, 5])
    RobotArrays(pos, head, flags, flags, pos, (points, offsets), (points, offsets))
    RobotArrays(pos, head)
    for bad in (dict(position=pos.astype(np.float32)), dict(position=np.zeros((M, 3))), dict(position=np.zeros(M)), dict(position=pos.tolist()),
                dict(heading=head.astype(np.float32)), dict(heading=np.zeros(M + 1)), dict(heading=np.zeros((M, 1))),
                dict(lifting=np.zeros(M, np.uint8)), dict(idle=np.zeros(M, np.int64)), dict(idle=np.zeros(M - 1, bool)),
                dict(target=pos.astype(np.float32)), dict(target=np.zeros((M + 1, 2))),
                dict(intention_path=(points.astype(np.float32), offsets)), dict(intention_path=(points, offsets.astype(np.int32))),
                dict(intention_path=(points, offsets[:-1])), dict(history_path=(np.zeros((5, 3)), offsets)), dict(history_path=points),
                dict(intention_path=(points, np.array([0, 2, 1, 3, 5]))), dict(intention_path=(points, np.array([0, 1, 1, 3, 4]))),
                dict(history_path=(points, np.array([0, 1, 1, 3, 6]))), dict(history_path=(points, np.array([1, 1, 1, 3, 5])))):
        with pytest.raises(ValueError, match='RobotArrays'):
            RobotArrays(**dict(dict(position=pos, heading=head, lifting=flags, idle=flags), **bad))


def test_get_states_refuses_what_the_list_form_refuses_before_any_device(episodes):
    from simq import mapper
    from simq._lib import SimqError
    RobotArrays = mapper.RobotArrays
    robots = states_of(episodes, 0)
    parts = lambda ra: dict(position=ra.position, heading=ra.heading, lifting=ra.lifting, idle=ra.idle, target=ra.target,
                            intention_path=ra.intention_path, history_path=ra.history_path)
    cases = ((dict(use_history_map=True), 'history_path', r"needs its history_path for the 'history' encoding"),
             (dict(use_intention_map=True), 'intention_path', r"needs its intention_path for the 'ramp' encoding"),
             (dict(use_intention_map=True, intention_map_encoding='circle'), 'target', r"needs its target for the 'circle' encoding"),
             (dict(use_intention_channels=True), 'target', 'needs its target for the intention channels'),
             (dict(use_intention_channels=True, intention_channel_encoding='nonspatial'), 'target', 'needs its target for the intention channels'))
    for cfg, name, message in cases:
        bm = build(episodes, **cfg)
        ra = RobotArrays.from_states(bm, robots)
        without = RobotArrays(**dict(parts(ra), **{name: None}))
        with pytest.raises(ValueError, match=message):
            bm.get_states(without)
        with pytest.raises(ValueError, match=message):              # the list form, in the same words
            bm.get_states([[r._replace(**{name: None}) for r in env] for env in robots])
        everyone_idle = RobotArrays(**dict(parts(without), idle=np.ones(6, bool)))
        if not torch.cuda.is_available():                           # nothing is missing; no quiet CPU path (departure (b))
            with pytest.raises(SimqError, match='need an MI355X'):
                bm.get_states(everyone_idle)
            with pytest.raises(SimqError, match='need an MI355X'):
                bm.get_states(ra, mappers=[4, 1])
    # an empty path of a robot that is drawn stands for a missing one; a mapper that is not read may hold anything
    bm = build(episodes, use_intention_map=True)
    ra = RobotArrays.from_states(bm, robots)
    busy = int(np.flatnonzero(~ra.idle[:3])[0])
    points, offsets = ra.intention_path
    emptied = offsets.copy()
    emptied[busy + 1:] -= offsets[busy + 1] - offsets[busy]
    cut = RobotArrays(**dict(parts(ra), intention_path=(np.concatenate([points[:offsets[busy]], points[offsets[busy + 1]:]]), emptied)))
    with pytest.raises(ValueError, match=r"needs its intention_path for the 'ramp' encoding"):
        bm.get_states(cut)
    if not torch.cuda.is_available():
        with pytest.raises(SimqError, match='need an MI355X'):      # its own state draws the others only
            bm.get_states(cut, mappers=[busy])
    # a wrong count, and the checks of `mappers`, `out` and `into` of the list form
    with pytest.raises(ValueError, match='hold 5 mappers, the object has 6'):
        bm.get_states(RobotArrays(np.zeros((5, 2)), np.zeros(5)))
    with pytest.raises(ValueError, match='mappers must name distinct mappers'):
        bm.get_states(ra, mappers=[1, 1])
    with pytest.raises(ValueError, match='out must be a contiguous float32 device tensor'):
        bm.get_states(ra, out=torch.empty((6, 96, 96, 1)))
    with pytest.raises(ValueError, match='`into` and `out`'):
        bm.get_states(ra, into=[], out=torch.empty((6, 96, 96, 2)))
