"""CPU: rooms over the LDS caps -- simq_occupancy_maps_large and simq_action_waypoints_large: the bindings, the
descriptors and the workspace sizes, every refusal of both entry points with fake device pointers (no kernel is launched here), what
they accept that the capped entries refuse, the host functions that split a call between an LDS entry and its large form, the three
keywords, BatchedMapper's per-mapper routing without a device, and tests/golden/large_rooms.npz against the oracles."""
import ctypes
import os

import numpy as np
import pytest

import large_rooms_cases as lr
import mapper_oracle
import occupancy_maps_oracle as occ_oracle
import store_new_action_oracle as act_oracle
import grid_simplify_oracle as so
import grid_waypoints_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARENA = []


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_exports_are_declared_bound_and_laid_out(L):
    from simq.actions import ActionWaypointLargeProblem, ActionWaypointProblem
    from simq.occupancy import OccupancyLargeProblem, OccupancyProblem
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, declared in (('simq_occupancy_maps_large', 'int simq_occupancy_maps_large('),
                           ('simq_occupancy_maps_large_work_bytes', 'int64_t simq_occupancy_maps_large_work_bytes('),
                           ('simq_action_waypoints_large', 'int simq_action_waypoints_large('),
                           ('simq_action_waypoints_large_work_bytes', 'int64_t simq_action_waypoints_large_work_bytes(')):
        assert declared in text and name in L.EXPORTS and hasattr(raw, name), name
    assert '#define SIMQ_OCCUPANCY_LARGE_MAX_DIM 2048' in text
    assert ctypes.sizeof(OccupancyLargeProblem) == ctypes.sizeof(OccupancyProblem) + 8 == 48
    assert OccupancyLargeProblem.work_offset.offset == 24 and OccupancyLargeProblem.work_offset.size == 8
    assert [n for n, _ in OccupancyLargeProblem._fields_ if n != 'work_offset'] == [n for n, _ in OccupancyProblem._fields_]
    assert (OccupancyLargeProblem.occupancy_offset.offset, OccupancyLargeProblem.mask_offset.offset, OccupancyLargeProblem.out_offset.offset,
            OccupancyLargeProblem.rows.offset, OccupancyLargeProblem.cols.offset, OccupancyLargeProblem.radius.offset,
            OccupancyLargeProblem.thin_radius.offset) == (0, 8, 16, 32, 36, 40, 44)
    assert ctypes.sizeof(ActionWaypointLargeProblem) == ctypes.sizeof(ActionWaypointProblem) + 8 == 88
    assert ActionWaypointLargeProblem.work_offset.offset == 32 and ActionWaypointLargeProblem.work_offset.size == 8
    assert [n for n, _ in ActionWaypointLargeProblem._fields_ if n != 'work_offset'] == [n for n, _ in ActionWaypointProblem._fields_]
    assert (ActionWaypointLargeProblem.way_offset.offset, ActionWaypointLargeProblem.way_capacity.offset, ActionWaypointLargeProblem.rows.offset,
            ActionWaypointLargeProblem.box_i0.offset, ActionWaypointLargeProblem.upstream.offset) == (24, 40, 44, 68, 84)


def test_work_bytes_equal_their_restatement(L):
    from simq import actions, occupancy
    fn = L.lib.c.simq_occupancy_maps_large_work_bytes
    for rows, cols in ((1, 1), (1, 2), (3, 5), (8, 1), (184, 262), (257, 1), (290, 290), (300, 257), (1096, 1096), (2048, 2), (2048, 2047),
                       (2047, 2048)):
        want = -(-(2 * rows * cols) // 16) * 16                                # one uint16 per cell, rounded up to 16
        assert fn(rows, cols) == occupancy.large_work_bytes(rows, cols) == want and want % 16 == 0 and want >= 2 * rows * cols, (rows, cols)
    assert fn(1, 1) == 16 and fn(290, 290) == 168208
    for bad in ((0, 4), (4, 0), (-1, 4), (2049, 1), (1, 2049), (2048, 2048)):
        assert fn(*bad) == -1, bad
    fn = L.lib.c.simq_action_waypoints_large_work_bytes
    for rows, cols in ((0, 0), (1, 1), (94, 94), (94, 142), (140, 140), (148, 148), (256, 256), (1, 32765), (2047, 2047), (2048, 2047)):
        cells, ring = (rows + 2) * (cols + 2), rows * cols + 1
        want = -(-(4 * cells + 4 * ring + cells + cells) // 16) * 16           # distances, ring, parents, flags
        assert fn(rows, cols) == actions.large_work_bytes(rows, cols) == want == L.lib.c.simq_grid_paths_large_work_bytes(rows, cols)
    for bad in ((-1, 4), (4, -1), (2048, 2048), (32766, 1), (1, 32766)):
        assert fn(*bad) == -1, bad


def arena(L, n):
    """A base address for n fake buffers 16 MiB apart; where there is a device they lie in one real allocation, so that a call that
    passes the checks launches inside the extents it declared."""
    import torch
    base = 1 << 32
    if torch.cuda.is_available():
        ARENA.append(torch.zeros(((n + 1) << 24) + 4096, dtype=torch.uint8, device='cuda'))
        base = (ARENA[-1].data_ptr() + (1 << 20) + 4095) // 4096 * 4096
    return base


def occupancy_harness(L):
    from simq.occupancy import OccupancyLargeProblem
    base = arena(L, 7)
    bufs = dict(maps=base, probs=base + (1 << 24), cspace=base + (2 << 24), thin=base + (3 << 24), closest=base + (4 << 24),
                status=base + (5 << 24), work=base + (6 << 24))

    def call(descs, n=None, maps_bytes=1 << 22, cspace_bytes=1 << 22, closest_ints=1 << 22, work_bytes=1 << 23, **ptrs):
        a = {k: ctypes.c_void_p(v) if v else None for k, v in dict(bufs, **ptrs).items()}
        arr = (OccupancyLargeProblem * len(descs))(*descs)
        return L.lib.c.simq_occupancy_maps_large(a['maps'], maps_bytes, arr, len(descs) if n is None else n, a['probs'], a['cspace'], a['thin'],
                                                 cspace_bytes, a['closest'], closest_ints, a['status'], a['work'], work_bytes, None)

    def prob(**kw):
        f = dict(occupancy_offset=0, mask_offset=1 << 21, out_offset=0, work_offset=0, rows=10, cols=12, radius=5, thin_radius=3)
        f.update(kw)
        return OccupancyLargeProblem(*[f[n] for n, _ in OccupancyLargeProblem._fields_])

    return call, prob, bufs


def action_harness(L):
    from simq.actions import ActionWaypointLargeProblem
    base = arena(L, 10)
    bufs = dict(cspace=base, thin=base + (1 << 24), closest=base + (2 << 24), probs=base + (3 << 24), ways=base + (4 << 24),
                counts=base + (5 << 24), ends=base + (6 << 24), upstream=base + (7 << 24), status=base + (8 << 24), work=base + (9 << 24))

    def call(descs, n=None, cspace_bytes=1 << 22, thin_bytes=1 << 22, closest_ints=1 << 22, way_pairs=1 << 16, n_upstream=4,
             work_bytes=1 << 22, **ptrs):
        a = {k: ctypes.c_void_p(v) if v else None for k, v in dict(bufs, **ptrs).items()}
        arr = (ActionWaypointLargeProblem * len(descs))(*descs)
        return L.lib.c.simq_action_waypoints_large(a['cspace'], cspace_bytes, a['thin'], thin_bytes, a['closest'], closest_ints, arr,
                                                   len(descs) if n is None else n, a['probs'], a['ways'], way_pairs, a['counts'], a['ends'],
                                                   a['upstream'], n_upstream, a['status'], a['work'], work_bytes, None)

    def prob(**kw):
        f = dict(cspace_offset=0, thin_offset=-1, closest_offset=-1, way_offset=0, work_offset=0, way_capacity=16, rows=10, cols=12, src_i=3,
                 src_j=4, tgt_i=5, tgt_j=6, box_i0=1, box_j0=1, box_rows=8, box_cols=10, upstream=-1)
        f.update(kw)
        return ActionWaypointLargeProblem(*[f[n] for n, _ in ActionWaypointLargeProblem._fields_])

    return call, prob, bufs


def refuser(L, call, who):
    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1, word
        err = L.last_error()
        assert err.startswith(who + ':') and word in err, (word, err)
    return refused


def accepter(L, call):
    """A call passes every host check exactly when it reaches the descriptor upload, its first HIP call: without a device that one
    fails (-2, naming the upload), with one the call launches and returns 0.  Either way the answer is not the refusal -1."""
    import torch

    def accepted(*args, **kw):
        rc = call(*args, **kw)
        if torch.cuda.is_available():
            assert rc == 0, L.last_error()
            torch.cuda.synchronize()
        else:
            assert rc == -2 and 'upload_descriptors' in L.last_error(), (rc, L.last_error())
    return accepted


def test_occupancy_maps_large_refuses_bad_descriptors_before_any_device_call(L):
    call, prob, bufs = occupancy_harness(L)
    refused = refuser(L, call, 'occupancy_maps_large')
    need = L.lib.c.simq_occupancy_maps_large_work_bytes(10, 12)
    assert need == 240
    refused('NULL', [prob()], cspace=0)
    refused('n = 0', [prob()], n=0)
    refused('is 0 x 12', [prob(rows=0)])
    refused('is 10 x 0', [prob(cols=0)])
    refused('is 2049 x 1 (rows, cols in 1 .. 2048)', [prob(rows=2049, cols=1)])
    refused('is 1 x 2049 (rows, cols in 1 .. 2048)', [prob(rows=1, cols=2049)])
    refused('2^22', [prob(rows=2048, cols=2048)], maps_bytes=1 << 24, cspace_bytes=1 << 23, closest_ints=1 << 24)
    refused('radius = 17', [prob(radius=17)])
    refused('thin_radius = 17', [prob(thin_radius=17)])
    refused('radius = -1', [prob(radius=-1)])
    refused('occupancy bytes', [prob(occupancy_offset=(1 << 22) - 119)])
    refused('room mask bytes', [prob(mask_offset=-1)])
    refused('output bytes', [prob(out_offset=1)], cspace_bytes=120)
    refused('closest ints', [prob()], closest_ints=239)
    refused("outputs overlap", [prob(), prob(out_offset=119, work_offset=need)])
    refused('d_cspace overlaps d_thin', [prob()], thin=bufs['cspace'] + 64)
    refused('d_status overlaps d_maps', [prob()], status=bufs['maps'] + 16)
    refused('d_problems must be 8-byte', [prob()], probs=bufs['probs'] + 4)
    # the workspace
    refused('NULL', [prob()], work=0)
    refused('d_work must be 16-byte aligned', [prob()], work=bufs['work'] + 8)
    refused('work_offset', [prob(work_offset=8)])
    refused('work_offset', [prob(work_offset=-16)])
    refused('work_offset', [prob()], work_bytes=need - 1)
    refused('work_offset', [prob(work_offset=(1 << 23) - need + 16)])
    refused('overlap in d_work', [prob(), prob(out_offset=120, work_offset=need - 16)])
    refused('overlap in d_work', [prob(work_offset=need - 16), prob(out_offset=120)])
    for other in ('cspace', 'thin', 'closest', 'status', 'maps', 'probs'):
        refused('overlaps d_work', [prob()], work=bufs[other])
    refused('d_status overlaps d_work', [prob()], status=bufs['work'] + need - 4, work_bytes=need)


def test_action_waypoints_large_refuses_bad_descriptors_before_any_device_call(L):
    call, prob, bufs = action_harness(L)
    refused = refuser(L, call, 'action_waypoints_large')
    need = L.lib.c.simq_action_waypoints_large_work_bytes(8, 10)
    assert need == 1056
    refused('NULL', [prob()], ways=0)
    refused('n = 0', [prob()], n=0)
    refused('is 0 x 12', [prob(rows=0)])
    refused('2^22', [prob(rows=2048, cols=2048)])
    refused('2^22', [prob(rows=2049, cols=2049)])
    refused('source (10, 4) outside', [prob(src_i=10)])
    refused('target (5, -1) outside', [prob(tgt_j=-1)])
    refused('cspace_offset', [prob()], cspace_bytes=119)
    refused('thin_offset', [prob(thin_offset=1)], thin_bytes=120)
    refused('closest_offset', [prob(closest_offset=0)], closest=0)
    refused('window', [prob(box_i0=3, box_rows=8)])
    refused('window', [prob(box_cols=-1)])
    refused('each side at most 32765', [prob(rows=1, cols=32766, src_i=0, tgt_i=0, box_i0=0, box_j0=0, box_rows=1, box_cols=32766)])
    refused('each side at most 32765', [prob(rows=32766, cols=1, src_j=0, tgt_j=0, box_i0=0, box_j0=0, box_rows=32766, box_cols=1)])
    refused('way_capacity', [prob(way_capacity=0)])
    refused('way_offset', [prob(way_offset=1)], way_pairs=16)
    refused('upstream = 4', [prob(upstream=4)])
    refused('d_upstream', [prob()], upstream=0)
    refused('overlap in d_ways', [prob(), prob(way_offset=15, work_offset=need)])
    refused('d_ways and d_counts overlap', [prob()], counts=bufs['ways'] + 64)
    refused('d_ways is not 8-byte aligned', [prob()], ways=bufs['ways'] + 4)
    # the workspace
    refused('NULL', [prob()], work=0)
    refused('d_work is not 16-byte aligned', [prob()], work=bufs['work'] + 8)
    refused('work_offset', [prob(work_offset=8)])
    refused('work_offset', [prob(work_offset=-16)])
    refused('work_offset', [prob()], work_bytes=need - 1)
    refused('work_offset', [prob(work_offset=(1 << 22) - need + 16)])
    refused('overlap in d_work', [prob(), prob(way_offset=16, work_offset=need - 16)])
    refused('overlap in d_work', [prob(work_offset=need - 16), prob(way_offset=16)])
    for other in ('cspace', 'thin', 'closest', 'upstream', 'probs', 'ways', 'counts', 'ends', 'status'):
        refused('d_work overlap', [prob(thin_offset=0, closest_offset=0, upstream=0)], work=bufs[other])
    refused('d_status and d_work overlap', [prob()], status=bufs['work'] + need - 4, work_bytes=need)


def test_the_large_entries_accept_what_the_capped_ones_refuse(L):
    from simq.actions import ActionWaypointProblem
    from simq.occupancy import OccupancyProblem
    call, prob, bufs = occupancy_harness(L)
    accepted = accepter(L, call)
    c = L.lib.c
    # 257 x 1: refused by the capped entry, taken here; so is a map under the old cap
    small = (OccupancyProblem * 1)(OccupancyProblem(0, 1 << 21, 0, 257, 1, 5, 3))
    p = {k: ctypes.c_void_p(v) for k, v in bufs.items()}
    assert c.simq_occupancy_maps(p['maps'], 1 << 22, small, 1, p['probs'], p['cspace'], p['thin'], 1 << 22, p['closest'], 1 << 22, p['status'],
                                 None) == -1
    assert 'is 257 x 1 (rows, cols in 1 .. 256)' in L.last_error()
    accepted([prob(rows=257, cols=1)])
    accepted([prob(rows=1, cols=257)])
    accepted([prob()])
    accepted([prob(rows=184, cols=262), prob(rows=290, cols=290, out_offset=184 * 262, occupancy_offset=184 * 262,
                                             work_offset=c.simq_occupancy_maps_large_work_bytes(184, 262))])
    accepted([prob()], status=bufs['work'] + 240, work_bytes=240)                          # d_work ends where d_status begins

    call, prob, bufs = action_harness(L)
    accepted = accepter(L, call)
    big = dict(rows=200, cols=200, box_i0=0, box_j0=0, box_rows=140, box_cols=140)
    assert 142 * 142 > 20000
    capped = (ActionWaypointProblem * 1)(ActionWaypointProblem(0, -1, -1, 0, 16, 200, 200, 3, 4, 5, 6, 0, 0, 140, 140, -1))
    p = {k: ctypes.c_void_p(v) for k, v in bufs.items()}
    assert c.simq_action_waypoints(p['cspace'], 1 << 22, p['thin'], 1 << 22, p['closest'], 1 << 22, capped, 1, p['probs'], p['ways'], 1 << 16,
                                   p['counts'], p['ends'], p['upstream'], 4, p['status'], None) == -1
    assert 'over SIMQ_GRID_PATH_MAX_BOX_CELLS' in L.last_error()
    fn = c.simq_action_waypoints_large_work_bytes
    accepted([prob(**big)])
    accepted([prob(**big), prob(**dict(big, way_offset=16, work_offset=fn(140, 140)))], work_bytes=2 * fn(140, 140))
    accepted([prob()])                                                                     # a window under the cap
    accepted([prob(box_i0=0, box_j0=0, box_rows=0, box_cols=0)], work_bytes=32)            # the empty window


def test_the_three_splits():
    from simq import actions, occupancy, waypoints
    # occupancy maps: by the sides of the map
    fits, edge, tall, wide = (184, 232), (256, 256), (257, 1), (184, 262)
    assert occupancy.split_by_shape([fits, edge, (1, 1)]) == ([0, 1, 2], [])
    assert occupancy.split_by_shape([tall, wide, (290, 290)]) == ([], [0, 1, 2])
    rng = np.random.RandomState(0)
    shapes = [(fits, edge, tall, wide)[k] for k in rng.randint(4, size=40)]
    fit, over = occupancy.split_by_shape(shapes)
    assert fit == [p for p, s in enumerate(shapes) if s in (fits, edge)] and over == [p for p, s in enumerate(shapes) if s in (tall, wide)]
    assert fit and over
    order, n_fit = occupancy.launch_order(shapes, True)
    assert order == fit + over and n_fit == len(fit)
    assert waypoints.restore_order(order, [('launched', p) for p in order]) == [('launched', p) for p in range(40)]
    assert occupancy.launch_order(shapes, False) == (list(range(40)), 40)               # all to simq_occupancy_maps, which refuses
    assert occupancy.entry_calls(40, 40) == [('simq_occupancy_maps', 0, 40)]            # an empty part makes no call
    assert occupancy.entry_calls(0, 40) == [('simq_occupancy_maps_large', 0, 40)]
    assert occupancy.entry_calls(n_fit, 40) == [('simq_occupancy_maps', 0, n_fit), ('simq_occupancy_maps_large', n_fit, 40)]
    # action waypoints: by the cells of the window with its halo
    small, edge, big, long = (3, 4, 50, 60), (0, 0, 98, 198), (71, 71, 148, 148), (1, 0, 1, 22000)
    assert 100 * 200 == actions.MAX_BOX_CELLS == waypoints.MAX_BOX_CELLS and 150 * 150 > actions.MAX_BOX_CELLS
    assert actions.split_by_window([small, edge, (0, 0, 0, 0)]) == ([0, 1, 2], [])
    assert actions.split_by_window([big, long, (0, 0, 98, 199)]) == ([], [0, 1, 2])
    boxes = [(small, edge, big, long)[k] for k in rng.randint(4, size=40)]
    assert actions.split_by_window(boxes) == waypoints.split_by_window(boxes)
    fit, over = actions.split_by_window(boxes)
    assert fit and over and sorted(fit + over) == list(range(40))
    table = np.zeros(40, actions.ACTION_PROBLEM)
    table['box_i0'], table['box_j0'], table['box_rows'], table['box_cols'] = np.asarray(boxes).T
    order, n_fit = actions.launch_order(table, True)
    assert order.tolist() == fit + over and n_fit == len(fit)
    assert waypoints.restore_order(order.tolist(), order.tolist()) == list(range(40))
    assert np.array_equal(order[np.argsort(order)], np.arange(40))
    order, n_fit = actions.launch_order(table, False)
    assert order.tolist() == list(range(40)) and n_fit == 40                            # all to simq_action_waypoints, which refuses
    assert actions.entry_calls(40, 40) == [('simq_action_waypoints', 0, 40)]
    assert actions.entry_calls(0, 40) == [('simq_action_waypoints_large', 0, 40)]
    assert actions.entry_calls(n_fit - 7, 40) == [('simq_action_waypoints', 0, 33), ('simq_action_waypoints_large', 33, 40)]


def test_each_keyword_takes_a_bool_only(L):
    import simq
    occ, mask = np.zeros((6, 7), np.uint8), np.ones((6, 7), np.uint8)
    cs, closest = np.ones((6, 7), np.uint8), np.zeros((2, 6, 7), np.int32)
    masks = {'pushing_robot': np.zeros((96, 96), np.float32)}
    for bad in ('yes', 1, 0, None):
        with pytest.raises(ValueError, match='large_maps'):
            simq.occupancy_maps([occ], [mask], 3, 2, large_maps=bad)
        with pytest.raises(ValueError, match='large_maps'):
            simq.configuration_space(occ, mask, 3, 2, large_maps=bad)
        with pytest.raises(ValueError, match='large_windows'):
            simq.store_new_actions([cs], [cs], [closest], [(0., 0.)], np.zeros(1), [5], 'pushing_robot', large_windows=bad)
        with pytest.raises(ValueError, match='large_rooms'):
            simq.BatchedMapper(1.0, 1.0, [['pushing_robot']], masks, large_rooms=bad)


def test_batched_mapper_routes_per_mapper_without_a_device(L):
    import simq
    masks = {t: np.zeros((96, 96), np.float32) for t in ('pushing_robot', 'lifting_robot', 'lifting_robot_with_cube')}
    types = [['pushing_robot', 'lifting_robot']] * 3
    bm = simq.BatchedMapper([1.0, 0.5, 1.6], [1.0, 1.3, 1.6], types, masks, large_rooms=True)
    assert bm.shapes == [(232, 232)] * 2 + [(184, 262)] * 2 + [(290, 290)] * 2 and bm.large_rooms is True
    assert bm.occupancy_entry == ['simq_occupancy_maps'] * 2 + ['simq_occupancy_maps_large'] * 4
    assert bm.action_entry == ['simq_action_waypoints'] * 4 + ['simq_action_waypoints_large'] * 2
    box = bm._action_constants()['box']
    assert box[2].tolist() == [70, 71, 44, 120] and box[4].tolist() == [71, 71, 148, 148] and 150 * 150 > 20000 >= 46 * 122
    c = L.lib.c
    assert np.diff(bm._occupancy_work_at).tolist() == [0, 0] + [c.simq_occupancy_maps_large_work_bytes(184, 262)] * 2 + \
        [c.simq_occupancy_maps_large_work_bytes(290, 290)] * 2
    assert np.diff(bm._action_work_at).tolist() == [0] * 4 + [c.simq_action_waypoints_large_work_bytes(148, 148)] * 2
    plain = simq.BatchedMapper([1.0, 0.5, 1.6], [1.0, 1.3, 1.6], types, masks)
    assert plain.large_rooms is False and plain.occupancy_entry == ['simq_occupancy_maps'] * 6 and plain.action_entry == ['simq_action_waypoints'] * 6
    assert not plain._occupancy_work_at.any() and not plain._action_work_at.any()
    with pytest.raises(ValueError, match='robot type'):                               # the arguments are still checked
        simq.BatchedMapper(1.6, 1.6, [['flying_robot']], masks, large_rooms=True)
    with pytest.raises(ValueError, match='mappers must name'):
        bm.store_new_actions([1, 2], None, mappers=[0, 0])


def test_fixture_rooms_are_the_reference_rooms(golden_dir):
    rooms, cases = lr.load(golden_dir)
    assert len(rooms) == len(lr.ROOMS) == 2
    for room, shape, (width, length) in zip(rooms, lr.SHAPES, lr.ROOMS):
        assert room['shape'] == shape == mapper_oracle.padded_room_shape(width, length)
        want = mapper_oracle.room_mask(width, length)
        assert room['room_mask'].dtype == np.uint8 and room['room_mask'].tobytes() == want.tobytes() and room['room_mask'].shape == want.shape
        assert len(room['maps']) >= 4 and {m['robot_type'] for m in room['maps']} == set(lr.ROBOT_TYPES)
        for m in room['maps']:
            assert m['configuration_space'].any(), m['name']                         # (an empty one has no defined result)
            assert m['radius'] == mapper_oracle.radii(m['robot_type'])[0] and m['thin_radius'] == mapper_oracle.radii(m['robot_type'])[1]
    assert rooms[0]['shape'][1] > 256 >= rooms[0]['shape'][0] and min(rooms[1]['shape']) > 256
    assert wo.free_box(rooms[0]['room_mask']) == (70, 71, 44, 120) and wo.free_box(rooms[1]['room_mask']) == (71, 71, 148, 148)
    assert 20 <= len(cases) <= 30


def test_occupancy_oracle_equals_the_fixture(golden_dir):
    rooms, _ = lr.load(golden_dir)
    for room in rooms:
        for m in room['maps']:
            got = occ_oracle.update(m['occupancy'], room['room_mask'], m['radius'], m['thin_radius'])
            for mine, want in zip(got, (m['configuration_space'], m['cspace_thin'], m['closest'])):
                assert mine.dtype == want.dtype and mine.shape == want.shape and mine.tobytes() == want.tobytes(), m['name']


def test_store_new_action_oracle_equals_the_fixture_and_its_classes(golden_dir):
    rooms, cases = lr.load(golden_dir)
    have = [dict.fromkeys(act_oracle.CLASSES, 0) for _ in rooms]
    caches = {}
    for c in cases:
        m = rooms[c['room']]['maps'][c['map']]
        assert m['robot_type'] == c['robot_type']
        path = None
        if c['use_shortest_path_movement']:
            cache = caches.setdefault((c['room'], c['map']), {})
            path = lambda a, b, m=m, cache=cache: wo.occupancy_shortest_path(m['configuration_space'], m['cspace_thin'], m['closest'], a, b,
                                                                             so.exact, cache)                          # noqa: E731
        action, target, ways, headings, signed = act_oracle.store_new_action(c['a'], c['position'], c['heading'], c['robot_type'], path)
        assert act_oracle.same_bits([action, target, ways, headings], [c['action'], c['target'], c['waypoints'], c['headings']]), c
        if path is not None:
            shape = rooms[c['room']]['shape']
            src = wo.position_to_pixel_indices(c['position'][0], c['position'][1], shape)
            tgt = wo.position_to_pixel_indices(target[0], target[1], shape)
            traced = not wo.is_straight(m['cspace_thin'], src, tgt) and len(ways) > 2
            for kind in act_oracle.kinds(len(ways), signed, traced):
                have[c['room']][kind] += 1
    assert min(have[1].values()) >= lr.PER_CLASS_LARGEST == 3, have                  # a fixture of straight lines would not test the search
    assert min(have[0].values()) >= 1, have
