"""CPU: Robot.store_new_action for many robots (simq/actions.py, simq_action_waypoints) without a device: the scalar oracle against the
fixture the reference's own function wrote, the array and list forms against both through the `search` hook that stands in for the
device, the host arithmetic against scalar `math`, every refusal of the C entry with fake pointers, and the argument checks."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import store_new_action_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


@pytest.fixture(scope='module')
def cases(golden_dir):
    return oracle.load_cases(golden_dir)


def oracle_search(golden_dir, mine):
    """The `search` hook over the cases `mine`: the oracle's pixel waypoints for the pixels the host computed."""
    def search(problems):
        status, counts, ends, pixels = [], [], [], [np.zeros((0, 2), np.int32)]
        assert len(problems) == len(mine)
        for c, q in zip(mine, problems):
            cspace, thin, closest = oracle.maps(golden_dir, c['room'])
            m = c['map']
            s, w, e = oracle.pixel_waypoints(cspace[m], thin[m], closest[m], (int(q['src_i']), int(q['src_j'])), (int(q['tgt_i']), int(q['tgt_j'])),
                                             oracle._PARENTS.setdefault((golden_dir, c['room'], m), {}))
            status.append(s)
            counts.append(len(w))
            ends.append(e)
            pixels.append(w)
        return np.asarray(status, np.int32), np.asarray(counts, np.int32), np.asarray(ends, np.int32), np.concatenate(pixels)
    return search


def attributes(c):
    return [c['action'], c['target'], c['waypoints'], c['headings']]


def test_fixture_covers_the_classes(cases):
    have = dict.fromkeys(oracle.CLASSES, 0)
    for c in cases:
        if c['use_shortest_path_movement']:
            n = len(c['waypoints'])
            back = n > 2 and c['waypoints'][-2] == c['waypoints'][-1]
            reach = oracle.END_EFFECTOR_LOCATION[c['robot_type']] + oracle.CUBE_WIDTH / 2
            short = back if n > 2 else oracle.distance(c['position'], c['target']) - reach < 0
            for k in oracle.kinds(n, -1.0 if short else 1.0, n > 2):
                have[k] += 1
    assert min(have.values()) >= 8, have
    assert {c['room'] for c in cases} == set(oracle.ROOMS) and {c['robot_type'] for c in cases} == set(oracle.ROBOT_TYPES)
    assert sum(not c['use_shortest_path_movement'] for c in cases) >= 8
    assert {c['action'][0] for c in cases} == {0, 1}
    assert min(c['heading'] for c in cases) < -3 and max(c['heading'] for c in cases) > 3


def test_oracle_equals_the_fixture(cases, golden_dir):
    for c in cases:
        sp = oracle.shortest_path_on(golden_dir, c['room'], c['map']) if c['use_shortest_path_movement'] else None
        got = oracle.store_new_action(c['a'], c['position'], c['heading'], c['robot_type'], sp)
        assert oracle.same_bits(list(got[:4]), attributes(c)), (c['room'], c['map'], c['a'])
        assert got[2][0] is c['position']


@pytest.mark.parametrize('as_arrays', [False, True])
def test_array_and_list_forms_equal_the_fixture(cases, golden_dir, monkeypatch, as_arrays):
    import simq
    from simq import actions
    for room in oracle.ROOMS:
        for sp in (True, False):
            mine = [c for c in cases if c['room'] == room and c['use_shortest_path_movement'] == sp]
            cspace, thin, closest = oracle.maps(golden_dir, room)
            monkeypatch.setattr(actions, 'search', oracle_search(golden_dir, mine))
            positions = [c['position'] for c in mine]
            if as_arrays:
                positions = np.asarray([p[:2] for p in positions], np.float64)
            got = simq.store_new_actions(cspace, thin, closest, positions, np.asarray([c['heading'] for c in mine]), [c['a'] for c in mine],
                                         [c['robot_type'] for c in mine], map_index=[c['map'] for c in mine], use_shortest_path_movement=sp)
            assert isinstance(got, simq.NewActions) and len(got) == len(mine)
            assert (got.action.dtype, got.offsets.dtype, got.status.dtype) == (np.int64, np.int64, np.int32)
            assert got.action.shape == (len(mine), 3) and got.target_end_effector_position.shape == (len(mine), 2)
            assert got.offsets[0] == 0 and got.offsets[-1] == len(got.waypoint_positions) == len(got.waypoint_headings)
            lists = got.as_lists()
            for p, (c, g) in enumerate(zip(mine, lists)):
                assert oracle.same_bits(list(g), attributes(c)), (room, sp, p)
                assert all(type(x) is int for x in g[0]) and type(g[1][2]) is int and all(type(h) is float for h in g[3])
                if not as_arrays:
                    assert g[2][0] is c['position']
                lo, hi = got.offsets[p], got.offsets[p + 1]
                assert np.array_equal(got.waypoint_positions[lo:hi], np.asarray([w[:2] for w in c['waypoints']]))
                assert got.waypoint_headings[lo:hi].tobytes() == np.asarray(c['headings']).tobytes()
            assert (got.status[[len(c['waypoints']) > 2 for c in mine]] == actions.TRACED).all()
            if not sp:
                assert (got.status == actions.STRAIGHT).all()


def test_host_arithmetic_equals_scalar_math():
    """Steps 2, 4, 5 and 6 of the rule on 10^5 seeded inputs: the array forms against the scalar expressions of the reference."""
    from simq import actions, arch
    rng = np.random.RandomState(2025)
    n = 100000
    a = rng.randint(0, 2 * 96 * 96, n)
    pos = rng.uniform(-1.5, 1.5, (n, 2))
    heading = rng.uniform(-math.pi, math.pi, n)
    heading[:4] = (math.pi, -math.pi, 0.0, -0.0)
    action, target = actions._targets(a, pos, heading, np.full(n, 2))
    want_action = np.stack(np.unravel_index(a, (2, 96, 96)), axis=1)
    assert np.array_equal(action, want_action)
    want = np.empty((n, 2))
    for k in range(n):
        dx, dy = ((action[k, 2] + 0.5) - 96 / 2) / 96.0, (96 / 2 - (action[k, 1] + 0.5)) / 96.0
        dist = math.sqrt(dx**2 + dy**2)
        theta = heading[k] + math.atan2(-dx, dy)
        want[k] = pos[k, 0] + dist * math.cos(theta), pos[k, 1] + dist * math.sin(theta)
    assert target.tobytes() == want.tobytes()
    # headings between successive points, with the range restricted: targets near the position give every quadrant and both axes
    b = pos + rng.uniform(-1, 1, (n, 2)) * (rng.rand(n, 1) < 0.9)
    b[:100, 0] = pos[:100, 0]                                               # straight up / down
    b[100:200, 1] = pos[100:200, 1]                                         # straight left / right: atan2 gives pi or -0.0
    got = actions.headings_between(pos, b)
    want = np.asarray([oracle.restrict_heading_range(math.atan2(b[k, 1] - pos[k, 1], b[k, 0] - pos[k, 0])) for k in range(n)])
    assert got.tobytes() == want.tobytes()
    # the offset of the last waypoint and the backing-up rule through _finish, three waypoints each: pos -> b -> target
    types = [oracle.ROBOT_TYPES[k % 4] for k in range(n)]
    counts = np.full(n, 3, np.int32)
    pixels = np.zeros((3 * n, 2), np.int64)
    pixels[1::3] = rng.randint(0, 184, (n, 2))
    near = rng.rand(n) < 0.5                                                # half of the targets within reach of the middle waypoint
    mid = np.stack([((pixels[1::3, 1] + 0.5) - 232 / 2) / 96.0, (184 / 2 - (pixels[1::3, 0] + 0.5)) / 96.0], axis=1)
    target = np.where(near[:, None], mid + rng.uniform(-0.08, 0.08, (n, 2)), target)
    rows, cols = np.full(n, 184, np.int32), np.full(n, 232, np.int32)
    got = actions._finish(action, pos, heading, target, actions.constants_of(types)[1], np.zeros(n, np.int32), counts, pixels, rows, cols, None)
    assert np.array_equal(got.offsets, 3 * np.arange(n + 1))
    backed = 0
    way, head = got.waypoint_positions.reshape(n, 3, 2), got.waypoint_headings.reshape(n, 3)
    for k in range(n):
        w = [tuple(pos[k]), tuple(mid[k]), tuple(target[k])]
        h = [heading[k]] + [oracle.restrict_heading_range(math.atan2(w[i][1] - w[i - 1][1], w[i][0] - w[i - 1][0])) for i in (1, 2)]
        signed = oracle.distance(w[1], w[2]) - (arch.get_end_effector_location(types[k]) + 0.044 / 2)
        w[2] = (w[1][0] + signed * math.cos(h[2]), w[1][1] + signed * math.sin(h[2]))
        if signed < 0:
            w[1] = w[2]
            h[1] = oracle.restrict_heading_range(math.atan2(w[1][1] - w[0][1], w[1][0] - w[0][0]))
            backed += 1
        assert way[k].tobytes() == np.asarray(w).tobytes() and head[k].tobytes() == np.asarray(h).tobytes(), k
    assert n // 8 < backed < n // 2


def test_header_binding_and_constants(L):
    from simq import arch
    from simq.actions import ActionWaypointProblem, MAX_BOX_CELLS
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    assert 'simq_action_waypoints' in L.EXPORTS and hasattr(ctypes.CDLL(L.LIB_PATH), 'simq_action_waypoints')
    assert ctypes.sizeof(ActionWaypointProblem) == 80 and ActionWaypointProblem.way_capacity.offset == 32 and \
        ActionWaypointProblem.upstream.offset == 76
    assert MAX_BOX_CELLS == int(text.split('#define SIMQ_GRID_PATH_MAX_BOX_CELLS')[1].split()[0])
    for t in oracle.ROBOT_TYPES:                                            # arch.get_robot_radius is what it was (envs.py:807-808)
        assert arch.get_end_effector_location(t) == oracle.END_EFFECTOR_LOCATION[t]
        assert arch.get_robot_radius(t) == math.sqrt(0.03**2 + (-0.0135 + arch.ROBOT_BASE_LENGTH[t])**2)
    assert arch.CUBE_WIDTH == oracle.CUBE_WIDTH
    with pytest.raises(Exception):
        arch.get_end_effector_location('hovering_robot')


def test_c_abi_rejects_bad_descriptors_before_any_device_call(L):
    """Every check of simq_action_waypoints runs on the host before the descriptor copy / launch (the fake device pointers below are
    never dereferenced)."""
    from simq.actions import ActionWaypointProblem
    c = L.lib.c
    base = 1 << 32
    bufs = dict(cspace=base, thin=base + (1 << 24), closest=base + (2 << 24), probs=base + (4 << 24), ways=base + (5 << 24),
                counts=base + (6 << 24), ends=base + (7 << 24), upstream=base + (8 << 24), status=base + (9 << 24))

    def call(descs, n=None, cspace_bytes=1 << 20, thin_bytes=1 << 20, closest_ints=1 << 20, way_pairs=1 << 16, n_upstream=4, **ptrs):
        a = {k: ctypes.c_void_p(v) if v else None for k, v in dict(bufs, **ptrs).items()}
        arr = (ActionWaypointProblem * len(descs))(*descs)
        return c.simq_action_waypoints(a['cspace'], cspace_bytes, a['thin'], thin_bytes, a['closest'], closest_ints, arr,
                                       len(descs) if n is None else n, a['probs'], a['ways'], way_pairs, a['counts'], a['ends'], a['upstream'],
                                       n_upstream, a['status'], None)

    def prob(**kw):
        f = dict(cspace_offset=0, thin_offset=0, closest_offset=0, way_offset=0, way_capacity=16, rows=10, cols=12, src_i=1, src_j=1, tgt_i=8,
                 tgt_j=10, box_i0=1, box_j0=1, box_rows=8, box_cols=10, upstream=-1)
        f.update(kw)
        return ActionWaypointProblem(*[f[n] for n, _ in ActionWaypointProblem._fields_])

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1, word
        assert word in L.last_error(), (word, L.last_error())

    def accepted(*args, **kw):
        """Every check passed: with a device the fake addresses must not get that far (the GPU test covers what is accepted)."""
        if not torch.cuda.is_available():
            assert call(*args, **kw) == -2, L.last_error()

    for name in ('cspace', 'probs', 'ways', 'counts', 'ends', 'status'):
        refused('NULL', [prob()], **{name: 0})
    refused('n = 0', [prob()], n=0)
    refused('extents', [prob()], way_pairs=0)
    refused('extents', [prob()], cspace_bytes=0)
    refused('extents', [prob()], thin_bytes=-1)
    refused('d_upstream and n_upstream', [prob()], upstream=0)
    refused('d_upstream and n_upstream', [prob()], n_upstream=0)
    refused('2^22', [prob(rows=2048, cols=2048)])
    refused('rows, cols >= 1', [prob(cols=0)])
    refused('source (10, 1)', [prob(src_i=10)])
    refused('source (1, -1)', [prob(src_j=-1)])
    refused('target (8, 12)', [prob(tgt_j=12)])
    refused('target (-1, 10)', [prob(tgt_i=-1)])
    refused('cspace_offset', [prob()], cspace_bytes=119)
    refused('cspace_offset', [prob(cspace_offset=-1)])
    refused('thin_offset', [prob()], thin_bytes=119)
    refused('thin_offset', [prob(thin_offset=-2)])
    refused('thin_offset', [prob()], thin=0, thin_bytes=0)
    refused('closest_offset', [prob()], closest_ints=239)
    refused('closest_offset', [prob(closest_offset=1)], closest_ints=240)
    refused('closest_offset', [prob()], closest=0, closest_ints=0)
    refused('window', [prob(box_i0=3)])
    refused('window', [prob(box_cols=12)])
    refused('window', [prob(box_rows=-1)])
    refused('SIMQ_GRID_PATH_MAX_BOX_CELLS', [prob(rows=100, cols=200, box_i0=0, box_j0=0, box_rows=98, box_cols=199)])
    refused('way_capacity', [prob(way_capacity=0)])
    refused('way_offset', [prob(way_offset=1)], way_pairs=16)
    refused('way_offset', [prob(way_offset=-1)])
    refused('upstream = 4', [prob(upstream=4)])
    refused('upstream = -2', [prob(upstream=-2)])
    refused('upstream = 0', [prob(upstream=0)], upstream=0, n_upstream=0)
    refused('overlap in d_ways', [prob(), prob(way_offset=15)])
    refused('d_cspace and d_ways overlap', [prob()], ways=bufs['cspace'] + 64)
    refused('d_thin and d_status overlap', [prob()], status=bufs['thin'] + 16)
    refused('d_closest and d_counts overlap', [prob()], counts=bufs['closest'] + 4)
    refused('d_upstream and d_status overlap', [prob()], status=bufs['upstream'])
    refused('d_upstream and d_endpoints overlap', [prob()], ends=bufs['upstream'] + 12)
    refused('d_problems and d_ways overlap', [prob()], probs=bufs['ways'] + 8)
    refused('d_counts and d_endpoints overlap', [prob()], ends=bufs['counts'])
    refused('d_counts and d_status overlap', [prob()], status=bufs['counts'])
    refused('d_ways is not 8-byte aligned', [prob()], ways=bufs['ways'] + 4)
    refused('d_problems is not 8-byte aligned', [prob()], probs=bufs['probs'] + 4)
    refused('d_closest is not 4-byte aligned', [prob()], closest=bufs['closest'] + 2)
    refused('d_upstream is not 4-byte aligned', [prob()], upstream=bufs['upstream'] + 2)
    refused('d_counts is not 4-byte aligned', [prob()], counts=bufs['counts'] + 2)
    refused('d_endpoints is not 4-byte aligned', [prob()], ends=bufs['ends'] + 1)
    refused('d_status is not 4-byte aligned', [prob()], status=bufs['status'] + 1)
    # what passes: the defaults; no thin map and no closest cells when no problem uses them; the window at the cap; inputs that share
    # bytes with each other; two written buffers one byte apart (d_counts ends where d_status begins)
    accepted([prob()])
    accepted([prob(thin_offset=-1, closest_offset=-1)], thin=0, thin_bytes=0, closest=0, closest_ints=0)
    accepted([prob(rows=100, cols=200, box_i0=0, box_j0=0, box_rows=98, box_cols=198)])
    accepted([prob()], thin=bufs['cspace'])
    accepted([prob(), prob(way_offset=16)], status=bufs['counts'] + 8)
    refused('d_counts and d_status overlap', [prob(), prob(way_offset=16)], status=bufs['counts'] + 4)
    accepted([prob(upstream=3)], upstream=bufs['status'] - 16)
    refused('d_upstream and d_status overlap', [prob(upstream=3)], upstream=bufs['status'] - 12)


def test_functional_form_checks_its_arguments(golden_dir):
    import simq
    cspace, thin, closest = oracle.maps(golden_dir, '184x232')
    pos, head = np.zeros((2, 2)), np.zeros(2)
    ok = dict(cspace=cspace, cspace_thin=thin, closest=closest, positions=pos, headings=head, actions=[5, 6], robot_types='pushing_robot',
              map_index=[0, 0])
    for word, change in (('outside [0, 1 * 96 * 96)', dict(actions=[5, 9216])), ('outside [0, 2 * 96 * 96)', dict(actions=[-1, 6], robot_types='lifting_robot')),
                         ('actions must be 2 integers', dict(actions=[5])), ('actions must be 2 integers', dict(actions=[5.0, 6.0])),
                         ('headings must be float64 [2]', dict(headings=np.zeros(3))), ('headings must be float64 [2]', dict(headings=np.zeros(2, np.float32))),
                         ('positions must be float64', dict(positions=np.zeros((2, 2), np.float32))), ('robot_types must name', dict(robot_types=['pushing_robot'])),
                         ('robot_types must name', dict(robot_types=['pushing_robot', 'hovering_robot'])),
                         ('map_index must name', dict(map_index=[0, 13])), ('13 maps but 2 robots', dict(map_index=None)),
                         ('one each per map', dict(cspace_thin=thin[:3])), ('window is (i0, j0, rows, cols)', dict(window=[(0, 0, 1, 1)] * 2)),
                         ('upstream must be a contiguous int32', dict(upstream=np.zeros(13, np.int32)))):
        with pytest.raises(ValueError) as e:
            simq.store_new_actions(**dict(ok, **change))
        assert word in str(e.value), (word, str(e.value))
    # without shortest paths nothing of the maps is read and no device is needed
    got = simq.store_new_actions(None, None, None, pos, head, [5, 6], 'pushing_robot', use_shortest_path_movement=False)
    assert got.offsets.tolist() == [0, 2, 4]
    if not torch.cuda.is_available():
        with pytest.raises(simq.actions.SimqError, match='MI355X'):
            simq.store_new_actions(**ok)


def small_mapper(envs=2):
    import simq
    masks = {name: np.zeros((96, 96), np.float32) for name in oracle.ROBOT_TYPES + ('lifting_robot_with_cube',)}
    return simq.BatchedMapper(0.5, 1.0, [list(oracle.ROBOT_TYPES)] * envs, masks)


def test_batched_mapper_checks_its_arguments(monkeypatch):
    import simq
    from simq import actions
    bm = small_mapper()
    robots = simq.RobotArrays(np.zeros((8, 2)), np.zeros(8))
    states = [[simq.RobotState((0.1 * r, 0.0, 0), 0.5, oracle.ROBOT_TYPES[r]) for r in range(4)] for _ in range(2)]
    for word, args, kw in (('outside [0, 1 * 96 * 96)', ([9216] * 8, robots), {}), ('actions must be 8 integers', ([1] * 7, robots), {}),
                           ('actions must be 2 integers', ([1] * 8, robots), dict(mappers=[3, 1])),
                           ('mappers must name distinct mappers', ([1, 1], robots), dict(mappers=[3, 3])),
                           ('the RobotArrays hold 4 mappers', ([1] * 8, simq.RobotArrays(np.zeros((4, 2)), np.zeros(4))), {}),
                           ('one list of RobotState per environment', ([1] * 8, states[:1]), {}),
                           ('environment 1 has 4 robots', ([1] * 8, [states[0], states[1][:3]]), {})):
        with pytest.raises(ValueError) as e:
            bm.store_new_actions(*args, **kw)
        assert word in str(e.value), (word, str(e.value))
    # both argument forms without shortest paths: nothing is launched, no device is needed, and the forms agree
    a = [7000, 9216 + 50, 40, 18000, 1, 2, 3, 4]
    lists = bm.store_new_actions(a, states, use_shortest_path_movement=False)
    arrays = bm.store_new_actions(a, simq.RobotArrays.from_states(bm, states), use_shortest_path_movement=False)
    assert oracle.same_bits(lists.as_lists(), arrays.as_lists())
    for p, got in enumerate(lists.as_lists()):
        r = states[p // 4][p % 4]
        want = oracle.store_new_action(a[p], r.position, r.heading, oracle.ROBOT_TYPES[p % 4])
        assert oracle.same_bits(list(got), list(want[:4])) and got[2][0] is r.position
    # the window is the room mask's box, a host constant, and the descriptors name the object's tensors where they lie
    seen = []
    monkeypatch.setattr(actions, 'search', lambda probs: seen.append(probs.copy()) or (np.ones(len(probs), np.int32), np.zeros(len(probs), np.int32),
                                                                                     np.zeros((len(probs), 4), np.int32), np.zeros((0, 2), np.int32)))
    bm.store_new_actions([5, 6], robots, mappers=[6, 1])
    q = seen[0]
    mask = simq.mapper.room_mask(0.5, 1.0)
    ii, jj = np.nonzero(mask)
    assert mask.shape == (184, 232) and q['box_i0'].tolist() == [ii.min()] * 2 and q['box_rows'].tolist() == [ii.max() - ii.min() + 1] * 2
    assert q['box_j0'].tolist() == [jj.min()] * 2 and q['box_cols'].tolist() == [jj.max() - jj.min() + 1] * 2
    assert q['cspace_offset'].tolist() == [6 * 184 * 232, 184 * 232] and q['closest_offset'].tolist() == [12 * 184 * 232, 2 * 184 * 232]
    assert q['thin_offset'].tolist() == q['cspace_offset'].tolist() and q['upstream'].tolist() == [6, 1]
    # pending deferred frames are refused as shortest_paths refuses them
    bm._pending[1].append(object())
    with pytest.raises(simq.mapper.SimqError, match='deferred frames'):
        bm.store_new_actions([5, 6], robots, mappers=[6, 1])
