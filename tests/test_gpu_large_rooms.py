"""GPU: rooms over the LDS caps.  simq_occupancy_maps_large and simq_action_waypoints_large through the C ABI --
the reference's own results in the rooms of tests/golden/large_rooms.npz, the numpy oracles on shapes that cross a byte or a 16-bit
limit, and each large entry against its LDS form byte for byte wherever both accept -- then the three keywords (large_maps,
large_windows, large_rooms) and one BatchedMapper over rooms on both sides of both caps as a chain.  Everything is compared bit for
bit."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import grid_simplify_oracle as so
import grid_waypoints_oracle as wo
import large_rooms_cases as lr
import mapper_oracle
import observation_maps_oracle as obs_oracle
import occupancy_maps_oracle as occ_oracle
import store_new_action_oracle as act_oracle
from test_gpu_grid_paths_large import degenerate_problems, reachable_near, seeded

pytestmark = pytest.mark.gpu

SENTINEL, BYTE_SENTINEL = -7, 0xC3
RANGES = obs_oracle.IdRanges(3, 9, 10, 11, 20)


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    import simq.actions  # noqa: F401
    import simq.occupancy  # noqa: F401
    return simq


def device():
    return torch.device('cuda', torch.cuda.current_device())


def counts_of(*names):
    from simq._lib import lib
    return [int(lib.c.simq_launch_count(n.encode())) for n in names]


def reset_counts():
    from simq._lib import lib
    lib.call('simq_launch_counts_reset')


# ---- 1: simq_occupancy_maps_large through the C ABI ---------------------------------------------------------------------------------
def occ_raw(entry, problems):
    """One call of `entry` ('simq_occupancy_maps' or 'simq_occupancy_maps_large') over (occupancy, room mask, radius, thin radius)
    problems: the outputs prefilled with a sentinel, the workspaces end to end and filled with 0xA5.  Returns {name: host array} and
    the cell offset of every problem."""
    from simq._lib import lib, ptr, stream_ptr
    from simq.occupancy import OccupancyLargeProblem, OccupancyProblem
    dev, P = device(), len(problems)
    at = np.concatenate([[0], np.cumsum([o.size for o, _, _, _ in problems])]).tolist()
    total = at[-1]
    packed = np.concatenate([np.asarray(o, np.uint8).reshape(-1) for o, _, _, _ in problems] +
                            [np.asarray(m, np.uint8).reshape(-1) for _, m, _, _ in problems])
    d_maps = torch.from_numpy(packed).to(dev)
    large = entry == 'simq_occupancy_maps_large'
    need = [int(lib.c.simq_occupancy_maps_large_work_bytes(*o.shape)) for o, _, _, _ in problems] if large else [0] * P
    assert min(need) >= 0
    woff = np.concatenate([[0], np.cumsum(need)]).tolist()
    descs = []
    for p, (o, _, radius, thin_radius) in enumerate(problems):
        fields = [at[p], total + at[p], at[p]] + ([woff[p]] if large else []) + [o.shape[0], o.shape[1], radius, thin_radius]
        descs.append((OccupancyLargeProblem if large else OccupancyProblem)(*fields))
    probs = ((OccupancyLargeProblem if large else OccupancyProblem) * P)(*descs)
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    out = dict(cspace=torch.full((total,), BYTE_SENTINEL, dtype=torch.uint8, device=dev),
               thin=torch.full((total,), BYTE_SENTINEL, dtype=torch.uint8, device=dev),
               closest=torch.full((2 * total,), SENTINEL, dtype=torch.int32, device=dev),
               status=torch.full((P,), SENTINEL, dtype=torch.int32, device=dev))
    extra = ()
    if large:
        work = torch.full((max(woff[-1], 16),), 0xA5, dtype=torch.uint8, device=dev)
        extra = (ptr(work), ctypes.c_int64(woff[-1]))
    lib.call(entry, ptr(d_maps), ctypes.c_int64(packed.size), probs, P, ptr(d_probs), ptr(out['cspace']), ptr(out['thin']), ctypes.c_int64(total),
             ptr(out['closest']), ctypes.c_int64(2 * total), ptr(out['status']), *extra, stream_ptr(dev))
    return {k: v.cpu().numpy() for k, v in out.items()}, at


def occ_results(host, at, problems, p):
    shape = problems[p][0].shape
    n = problems[p][0].size
    return (host['cspace'][at[p]:at[p] + n].reshape(shape), host['thin'][at[p]:at[p] + n].reshape(shape),
            host['closest'][2 * at[p]:2 * at[p] + 2 * n].reshape((2,) + shape))


def assert_occupancy(host, at, problems, p, want, status=0):
    got = occ_results(host, at, problems, p)
    assert host['status'][p] == status, (p, host['status'][p])
    for name, mine, theirs in zip(('configuration_space', 'cspace_thin', 'closest'), got, want):
        assert mine.dtype == theirs.dtype and np.array_equal(mine, theirs), (p, name)


def test_occupancy_large_equals_the_reference_in_the_large_rooms(S, golden_dir):
    rooms, _ = lr.load(golden_dir)
    problems = [(m['occupancy'], room['room_mask'], m['radius'], m['thin_radius']) for room in rooms for m in room['maps']]
    want = [(m['configuration_space'], m['cspace_thin'], m['closest']) for room in rooms for m in room['maps']]
    assert {p[0].shape for p in problems} == set(lr.SHAPES)
    host, at = occ_raw('simq_occupancy_maps_large', problems)
    for p in range(len(problems)):
        assert_occupancy(host, at, problems, p, want[p])


def edge_problems():
    """(name, occupancy, mask, radius, thin radius) on shapes that cross a limit of the LDS kernel."""
    rng = np.random.RandomState(8)
    out = []
    for name, shape in (('257x1', (257, 1)), ('1x257', (1, 257)), ('257x3', (257, 3)), ('2048x2', (2048, 2))):
        occ = (rng.rand(*shape) < 0.04).astype(np.uint8)
        mask = np.ones(shape, np.uint8)
        mask[:2] = 0
        if shape[0] == 1:
            mask[:] = 1
            mask[:, :3] = 0
        out.append((name, occ, mask, 2, 1))
    # 300 x 257 with the only free cells at rows >= 256 and at columns >= 256: every answer crosses both byte limits
    occ = np.zeros((300, 257), np.uint8)
    occ[rng.randint(0, 250, 12), rng.randint(0, 250, 12)] = 1
    occ[270, 256] = 1
    mask = np.zeros((300, 257), np.uint8)
    mask[256:, 256:] = 1
    out.append(('300x257', occ, mask, 3, 2))
    for radius in (0, 16):
        occ = (rng.rand(64, 64) < 0.01).astype(np.uint8)
        if radius == 16:                                                # two obstacles: a disk of 16 leaves free cells between them
            occ[:] = 0
            occ[8, 9], occ[50, 44] = 1, 1
        mask = np.zeros((64, 64), np.uint8)
        mask[3:60, 2:62] = 1
        out.append(('64x64_r%d' % radius, occ, mask, radius, radius))
    occ = np.zeros((70, 300), np.uint8)
    occ[::9, ::9] = 1
    out.append(('empty', occ, np.ones((70, 300), np.uint8), 8, 3))
    return out


def test_occupancy_large_equals_the_oracle_across_the_byte_limits(S):
    named = edge_problems()
    problems = [q[1:] for q in named]
    host, at = occ_raw('simq_occupancy_maps_large', problems)
    for p, (name, occ, mask, radius, thin_radius) in enumerate(named):
        want = occ_oracle.update(occ, mask, radius, thin_radius)
        if name == 'empty':
            assert not want[0].any() and (want[2] == -1).all()
        else:
            assert want[0].any(), name
        assert_occupancy(host, at, problems, p, want, status=1 if name == 'empty' else 0)
    cs, _, closest = occ_results(host, at, problems, [q[0] for q in named].index('300x257'))
    free = np.argwhere(cs != 0)
    assert len(free) >= 30 and free.min() >= 256 and closest.min() >= 256 and (closest[1] == 256).all() and len(np.unique(closest[0])) >= 30


def tie_counts(cspace):
    """Of the blocked pixels with exactly two nearest free cells: how many have them in different rows of one column, and how many
    in different columns."""
    free = np.argwhere(cspace != 0)
    same_column = other_column = 0
    for i, j in np.argwhere(cspace == 0):
        d = (free[:, 0] - i) ** 2 + (free[:, 1] - j) ** 2
        near = free[d == d.min()]
        if len(near) == 2:
            same_column += near[0][1] == near[1][1]
            other_column += near[0][1] != near[1][1]
    return int(same_column), int(other_column)


def test_occupancy_large_breaks_ties_as_scipy_does(S):
    """Two free rows (columns) an even distance apart: the pixels midway have two nearest free cells, in one column (in two columns);
    the feature transform takes the smaller row (the smaller column)."""
    rows = np.zeros((41, 300), np.uint8)
    rows[10, :], rows[30, :] = 1, 1
    cols = np.zeros((300, 41), np.uint8)
    cols[:, 10], cols[:, 30] = 1, 1
    problems = [(np.zeros_like(rows), rows, 0, 0), (np.zeros_like(cols), cols, 0, 0)]
    want = [occ_oracle.update(*q) for q in problems]
    assert np.array_equal(want[0][0], rows) and np.array_equal(want[1][0], cols)
    a, b = tie_counts(rows), tie_counts(cols)
    assert a[0] >= 50 and b[1] >= 50, (a, b)
    assert (want[0][2][0, 20] == 10).all() and (want[1][2][1, :, 20] == 10).all()
    host, at = occ_raw('simq_occupancy_maps_large', problems)
    for p in range(2):
        assert_occupancy(host, at, problems, p, want[p])


def test_occupancy_entries_write_the_same_bytes(S, golden_dir):
    """Every map of the two occupancy fixtures under the cap through both entry points: all three outputs and the status words."""
    files = sorted(glob.glob(os.path.join(golden_dir, 'occupancy_maps_*.npz')))
    assert len(files) == 2
    for f in files:
        fixture = occ_oracle.load_fixture(f)
        problems = [(m['occupancy'], m['room_mask'], m['radius'], m['thin_radius']) for m in fixture]
        lds, at = occ_raw('simq_occupancy_maps', problems)
        hbm, _ = occ_raw('simq_occupancy_maps_large', problems)
        for k in ('cspace', 'thin', 'closest', 'status'):
            assert np.array_equal(lds[k], hbm[k]), (f, k)
        assert (hbm['cspace'] <= 1).all() and (hbm['thin'] <= 1).all() and set(hbm['status'].tolist()) <= {0, 1}
        for p, m in enumerate(fixture):
            if m['configuration_space'].any():
                assert_occupancy(hbm, at, problems, p, (m['configuration_space'], m['cspace_thin'], m['closest']))


# ---- 2: simq_action_waypoints_large through the C ABI -------------------------------------------------------------------------------
def act_raw(entry, problems, capacities, upstream=None):
    """One call of `entry` ('simq_action_waypoints' or 'simq_action_waypoints_large') over problems (grid, source, target) or dicts
    (grid, src, tgt, and optionally thin, box, upstream), the grid of each its own map: every output prefilled with SENTINEL, the
    workspaces end to end and filled with 0xA5.  Returns {name: host array}."""
    from simq._lib import lib, ptr, stream_ptr
    from simq.actions import ActionWaypointLargeProblem, ActionWaypointProblem
    dev, P = device(), len(problems)
    problems = [q if isinstance(q, dict) else dict(grid=q[0], src=q[1], tgt=q[2]) for q in problems]
    at = np.concatenate([[0], np.cumsum([(q['grid'].size + 15) // 16 * 16 for q in problems])]).tolist()
    cspace, thin = np.zeros(at[-1], np.uint8), np.zeros(at[-1], np.uint8)
    for p, q in enumerate(problems):
        cspace[at[p]:at[p] + q['grid'].size] = q['grid'].reshape(-1)
        if q.get('thin') is not None:
            thin[at[p]:at[p] + q['grid'].size] = q['thin'].reshape(-1)
    large = entry == 'simq_action_waypoints_large'
    boxes = [q.get('box', wo.free_box(q['grid'])) for q in problems]
    need = [int(lib.c.simq_action_waypoints_large_work_bytes(b[2], b[3])) for b in boxes] if large else [0] * P
    assert min(need) >= 0
    woff = np.concatenate([[0], np.cumsum(need)]).tolist()
    poff = np.concatenate([[0], np.cumsum(capacities)]).tolist()
    descs = []
    for p, q in enumerate(problems):
        offsets = [at[p], at[p] if q.get('thin') is not None else -1, -1, poff[p]] + ([woff[p]] if large else [])
        descs.append((ActionWaypointLargeProblem if large else ActionWaypointProblem)(
            *offsets, capacities[p], q['grid'].shape[0], q['grid'].shape[1], *q['src'], *q['tgt'], *boxes[p], q.get('upstream', -1)))
    probs = ((ActionWaypointLargeProblem if large else ActionWaypointProblem) * P)(*descs)
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    d_cspace, d_thin = torch.from_numpy(cspace).to(dev), torch.from_numpy(thin).to(dev)
    d_up = None if upstream is None else torch.tensor(upstream, dtype=torch.int32, device=dev)
    out = dict(ways=torch.full((poff[-1], 2), SENTINEL, dtype=torch.int32, device=dev),
               counts=torch.full((P,), SENTINEL, dtype=torch.int32, device=dev),
               ends=torch.full((P, 4), SENTINEL, dtype=torch.int32, device=dev),
               status=torch.full((P,), SENTINEL, dtype=torch.int32, device=dev))
    extra = ()
    if large:
        work = torch.full((max(woff[-1], 16),), 0xA5, dtype=torch.uint8, device=dev)
        extra = (ptr(work), ctypes.c_int64(woff[-1]))
    lib.call(entry, ptr(d_cspace), ctypes.c_int64(cspace.size), ptr(d_thin), ctypes.c_int64(thin.size), None, ctypes.c_int64(0), probs, P,
             ptr(d_probs), ptr(out['ways']), ctypes.c_int64(poff[-1]), ptr(out['counts']), ptr(out['ends']), ptr(d_up),
             0 if d_up is None else d_up.numel(), ptr(out['status']), *extra, stream_ptr(dev))
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host['starts'] = poff
    return host


def both_entries(problems, capacities, upstream=None):
    lds = act_raw('simq_action_waypoints', problems, capacities, upstream)
    hbm = act_raw('simq_action_waypoints_large', problems, capacities, upstream)
    for k in ('ways', 'counts', 'ends', 'status'):
        assert np.array_equal(lds[k], hbm[k]), k
    return hbm


def grid_oracle(grid, s, t):
    """The waypoints of the exact rule on a plain grid (no line test, no snap)."""
    return so.waypoints(grid, wo.dense_path(wo.spfa(grid, s)[1], s, t))


def test_action_entries_write_the_same_bytes(S):
    """The 60 random grids and the fifteen degenerate problems of test_gpu_grid_paths_large.py through both entry points: every byte
    of d_ways, d_counts, d_endpoints and d_status, the sentinels included; against the oracle; a clear line (status 1), a capacity
    of one pair (status 3) and an upstream word that is not 0."""
    for problems in (wo.random_grids(), degenerate_problems()):
        capacities = [max(2, g.size) for g, _, _ in problems]
        got = both_entries(problems, capacities)
        assert (got['status'] == 0).all()
        for p, (grid, s, t) in enumerate(problems):
            want = grid_oracle(grid, s, t)
            a = got['starts'][p]
            assert got['counts'][p] == len(want) and np.array_equal(got['ways'][a:a + len(want)], want), p
            assert (got['ways'][a + len(want):got['starts'][p + 1]] == SENTINEL).all(), p
            assert got['ends'][p].tolist() == list(s) + list(t), p
    problems = wo.random_grids()[:16]
    need = both_entries(problems, [g.size for g, _, _ in problems])['counts']
    # a thin map of ones: the line of every second problem is clear
    lines = [dict(grid=g, src=s, tgt=t, thin=np.ones_like(g) if p % 2 else g) for p, (g, s, t) in enumerate(problems)]
    got = both_entries(lines, [g.size for g, _, _ in problems])
    assert (got['status'][1::2] == 1).all() and (got['counts'][1::2] == 0).all() and set(got['status'][0::2].tolist()) <= {0, 1}
    assert (got['status'] == 0).sum() >= 4
    # one pair of capacity: status 3 with the need, one pair written
    got = both_entries(problems, [1] * len(problems))
    assert np.array_equal(got['counts'], need) and np.array_equal(got['status'], np.where(need > 1, 3, 0)) and (need > 1).sum() >= 8
    # an upstream word that is not 0 is passed on: status = the word, count 0, nothing else written
    named = [dict(grid=g, src=s, tgt=t, upstream=p % 2) for p, (g, s, t) in enumerate(problems)]
    got = both_entries(named, [g.size for g, _, _ in problems], upstream=[0, 5])
    assert (got['status'][1::2] == 5).all() and (got['counts'][1::2] == 0).all() and (got['ends'][1::2] == SENTINEL).all()
    assert (got['status'][0::2] == 0).all() and np.array_equal(got['counts'][0::2], need[0::2])


@pytest.mark.parametrize('n', [142, 258])
def test_action_large_windows_over_the_cap_equal_the_oracle(S, n):
    """142 x 142: just over the LDS cap.  258 x 258: 67 600 cells with the halo, so ring entries and window indices pass 2^16."""
    from simq.actions import MAX_BOX_CELLS
    grid, source, o_dist, o_parents, _ = seeded(n)
    assert (n + 2) * (n + 2) > MAX_BOX_CELLS and ((n + 2) * (n + 2) > 1 << 16) == (n == 258)
    targets = [reachable_near(o_dist, c) for c in ((0, 0), (0, n - 1), (n - 1, 0), (n // 2, n // 3))] + [source]
    problems = [(grid, source, t) for t in targets]
    got = act_raw('simq_action_waypoints_large', problems, [64] * len(problems))
    assert (got['status'] == 0).all()
    for p, t in enumerate(targets):
        want = so.waypoints(grid, wo.dense_path(o_parents, source, t))
        a = got['starts'][p]
        assert got['counts'][p] == len(want) <= 64 and np.array_equal(got['ways'][a:a + len(want)], want), (n, t)
        assert got['ends'][p].tolist() == list(source) + list(t)
    assert got['counts'].max() >= 4 and got['counts'][-1] == 1


def serpentine(n):
    """Free rows 0, 2, 4, ... of an n x n grid joined at alternating ends: one corridor from (0, 0) to the last free row."""
    grid = np.ones((n, n), np.uint8)
    grid[1::2, :] = 0
    grid[1::4, -1] = 1
    grid[3::4, 0] = 1
    return grid


def test_action_large_takes_a_path_longer_than_the_lds_form_holds(S):
    """A serpentine corridor whose dense path has more than SIMQ_GRID_WAYPOINTS_MAX_PATH = 20 480 points, in the smallest odd window
    that gives one: a corridor of k rows of n cells joined by k - 1 cells, the corners cut by one diagonal step each."""
    n = next(n for n in range(3, 400, 2) if (n + 1) // 2 * n - ((n + 1) // 2 - 1) > 20480 + 2 * n)
    grid = serpentine(n)
    s, t = (0, 0), (n - 1, 0 if ((n - 1) // 2) % 2 == 0 else n - 1)
    assert grid[t] == 1
    dense = wo.dense_path(wo.spfa(grid, s)[1], s, t)
    assert 20480 < len(dense) < 20480 + 4 * n, (n, len(dense))
    want = so.waypoints(grid, dense)
    assert 100 < len(want) <= 4 * ((n + 1) // 2)                            # (a corner of the corridor keeps one or two waypoints)
    got = act_raw('simq_action_waypoints_large', [(grid, s, t)], [len(want) + 8])
    assert got['status'][0] == 0 and got['counts'][0] == len(want)
    assert np.array_equal(got['ways'][:len(want)], want) and (got['ways'][len(want):] == SENTINEL).all()


# ---- 3: the keywords of the public functions ----------------------------------------------------------------------------------------
def test_occupancy_maps_splits_a_mixed_list(S, golden_dir):
    rooms, _ = lr.load(golden_dir)
    small = occ_oracle.load_fixture(sorted(glob.glob(os.path.join(golden_dir, 'occupancy_maps_*.npz')))[0])[:3]
    big = [(room, m) for room in rooms for m in room['maps'][:2]]
    order = [('small', 0), ('big', 0), ('big', 2), ('small', 1), ('big', 1), ('small', 2), ('big', 3)]
    occupancy, masks, radii, thin_radii, want = [], [], [], [], []
    for kind, k in order:
        m, mask = (small[k], small[k]['room_mask']) if kind == 'small' else (big[k][1], big[k][0]['room_mask'])
        occupancy.append(m['occupancy'])
        masks.append(mask)
        radii.append(m['radius'])
        thin_radii.append(m['thin_radius'])
        want.append((m['configuration_space'], m['cspace_thin'], m['closest']))
    reset_counts()
    with pytest.raises(S.occupancy.SimqError, match=r'occupancy_maps: problem 1 is 184 x 262 \(rows, cols in 1 .. 256\)'):
        S.occupancy_maps(occupancy, masks, radii, thin_radii)
    assert counts_of('occupancy_maps', 'occupancy_maps_large') == [0, 0]
    got = S.occupancy_maps(occupancy, masks, radii, thin_radii, large_maps=True)
    assert counts_of('occupancy_maps', 'occupancy_maps_large') == [1, 1]
    for p in range(len(order)):
        for mine, theirs in zip((got.configuration_space[p], got.cspace_thin[p], got.closest_cspace_indices[p]), want[p]):
            assert np.array_equal(mine.cpu().numpy(), theirs), (p, order[p])
    # all under the cap, or all over it: the one entry point alone
    reset_counts()
    S.occupancy_maps(occupancy[0::3], masks[0::3], radii[0::3], thin_radii[0::3], large_maps=True)
    assert [order[p][0] for p in (0, 3, 6)] == ['small', 'small', 'big']
    S.occupancy_maps([occupancy[0], occupancy[3]], [masks[0], masks[3]], [radii[0], radii[3]], thin_radii[0], large_maps=True)
    assert counts_of('occupancy_maps', 'occupancy_maps_large') == [2, 1]
    one = S.configuration_space(occupancy[2], masks[2], radii[2], thin_radii[2], large_maps=True)
    assert counts_of('occupancy_maps', 'occupancy_maps_large') == [2, 2]
    for mine, theirs in zip(one, want[2]):
        assert mine.dtype == theirs.dtype and np.array_equal(mine, theirs)


def test_store_new_actions_splits_by_window(S, golden_dir):
    """Every case of the fixture in one call: the robots of the 0.5 m x 1.3 m room through simq_action_waypoints, those of the
    1.6 m x 1.6 m room through simq_action_waypoints_large, the reference's four attributes in problem order."""
    rooms, cases = lr.load(golden_dir)
    cases = [c for c in cases if c['use_shortest_path_movement']]
    maps = [m for room in rooms for m in room['maps']]
    first = [0, len(rooms[0]['maps'])]
    args = dict(cspace=[m['configuration_space'] for m in maps], cspace_thin=[m['cspace_thin'] for m in maps],
                closest=[m['closest'] for m in maps], positions=[c['position'] for c in cases],
                headings=np.asarray([c['heading'] for c in cases]), actions=[c['a'] for c in cases],
                robot_types=[c['robot_type'] for c in cases], map_index=[first[c['room']] + c['map'] for c in cases],
                window=[wo.free_box(room['room_mask']) for room in rooms for _ in room['maps']])      # the room masks' boxes, as BatchedMapper
    assert [(w[2] + 2) * (w[3] + 2) > 20000 for w in (args['window'][0], args['window'][-1])] == [False, True]
    assert len({c['room'] for c in cases}) == 2
    reset_counts()
    with pytest.raises(S.occupancy.SimqError, match='SIMQ_GRID_PATH_MAX_BOX_CELLS'):
        S.store_new_actions(**args)
    assert counts_of('action_waypoints', 'action_waypoints_large') == [0, 0]
    got = S.store_new_actions(large_windows=True, **args)
    assert counts_of('action_waypoints', 'action_waypoints_large') == [1, 1]
    for c, mine in zip(cases, got.as_lists()):
        assert act_oracle.same_bits(list(mine), [c['action'], c['target'], c['waypoints'], c['headings']]), c
    # a waypoint buffer of two pairs: the second round works over both parts
    from simq import actions
    lists = got.as_lists()
    assert max(len(w[2]) for w in lists) > 2
    assert all(max(len(w[2]) for w, c in zip(lists, cases) if c['room'] == r) > 2 for r in (0, 1))
    run = actions.run_problems
    try:
        actions.run_problems = lambda *a, **k: run(*a, **dict(k, capacity=2))
        reset_counts()
        short = S.store_new_actions(large_windows=True, **args)
        assert counts_of('action_waypoints', 'action_waypoints_large') == [2, 2]
    finally:
        actions.run_problems = run
    assert act_oracle.same_bits(short.as_lists(), lists)
    # the robots of one room alone: one entry point
    reset_counts()
    only = [k for k, c in enumerate(cases) if c['room'] == 1]
    sub = dict(args, positions=[args['positions'][k] for k in only], headings=args['headings'][only], actions=[args['actions'][k] for k in only],
               robot_types=[args['robot_types'][k] for k in only], map_index=[args['map_index'][k] for k in only])
    S.store_new_actions(large_windows=True, **sub)
    assert counts_of('action_waypoints', 'action_waypoints_large') == [0, 1]


# ---- 4: one BatchedMapper over rooms on both sides of both caps -----------------------------------------------------------------------
ENV_ROOMS = ((1.0, 1.0), (0.5, 1.3), (1.6, 1.6))                     # (room_width, room_length): under both caps, over one, over both
ENV_TYPES = (('pushing_robot', 'lifting_robot'), ('pushing_robot', 'lifting_robot'), ('lifting_robot', 'throwing_robot'))
RECEPTACLE = (0.2, -0.1, 0.0)
CFG = mapper_oracle.config(use_robot_map=True, use_distance_to_receptacle_map=True, use_shortest_path_map=True)


def overhead_frame(rng, blocks, empty=False):
    """A frame of the overhead camera over the middle of a room: a floor with raised blocks of obstacle ids (tools/
    observation_maps_rate.py); `empty`: the floor alone, which leaves an occupancy map as it is."""
    near, far = 0.1, 10
    heading = rng.uniform(-np.pi, np.pi)
    x, y = rng.uniform(-0.1, 0.1, size=2)
    g = obs_oracle.camera_geometry((x, y, 1), (x, y, 0), (np.cos(heading), np.sin(heading), 0), near, far, 1, 156)
    height, ids = np.zeros((156, 156)), np.zeros((156, 156), np.int32)
    for k in range(0 if empty else blocks):
        i, j, h = rng.randint(10, 130), rng.randint(10, 130), (0.044, 0.1, 0.2)[k % 3]
        height[i:i + 6, j:j + 6] = h
        ids[i:i + 6, j:j + 6] = 3 + k % 7
    buffer = ((far - far * near / (1.0 - height)) / (far - near)).astype(np.float32)
    return buffer, np.ascontiguousarray(ids), g


def masks_of(golden_dir):
    """({name: mask}, the bank, its names): a disk per robot type, each of its own radius (Mapper._create_robot_mask draws the robot's
    outline; the chain only needs masks that differ)."""
    names = ['pushing_robot', 'lifting_robot', 'throwing_robot', 'lifting_robot_with_cube']
    i, j = np.mgrid[0:96, 0:96]
    bank = np.stack([((i - 47.5) ** 2 + (j - 47.5) ** 2 <= (5 + k) ** 2).astype(np.float32) for k in range(len(names))])
    return {name: bank[k] for k, name in enumerate(names)}, bank, names


def robots_on_free_cells(bm_maps, envs, rng):
    """Per environment its robots as mapper_oracle dicts, each on a free cell of its own configuration space."""
    out, m = [], 0
    for e in envs:
        env = []
        for t in ENV_TYPES[e]:
            cs = bm_maps[m].configuration_space
            i, j = np.argwhere(cs != 0)[rng.randint(int((cs != 0).sum()))]
            x, y = wo.pixel_indices_to_position(i + float(rng.uniform(-0.4, 0.4)), j + float(rng.uniform(-0.4, 0.4)), cs.shape)
            env.append({'type': t, 'group': 0, 'position': (float(x), float(y)), 'heading': float(rng.uniform(-np.pi, np.pi)), 'lift_state': None,
                        'idle': True, 'target': None, 'intention_path': None, 'history_path': None})
            m += 1
        out.append(env)
    return out


def chain(S, golden_dir, envs, large_rooms):
    """A BatchedMapper over the named environments after one update from synthetic frames, the oracle's maps of every mapper, the
    robots, the states of get_states and the launch counts of update and get_states."""
    from simq.observation import CameraGeometry, IdRanges
    masks, bank, names = masks_of(golden_dir)
    flags = {f: CFG[f] for f in mapper_oracle.FLAGS}
    bm = S.BatchedMapper([ENV_ROOMS[e][0] for e in envs], [ENV_ROOMS[e][1] for e in envs], [list(ENV_TYPES[e]) for e in envs], masks,
                         receptacle_position=RECEPTACLE, large_rooms=large_rooms, **flags)
    rng = np.random.RandomState(17)
    frames, maps = [], []
    for e in envs:
        for t in ENV_TYPES[e]:
            frames.append(overhead_frame(rng, 5))
            maps.append(mapper_oracle.Maps(ENV_ROOMS[e][0], ENV_ROOMS[e][1], t))
            assert maps[-1].update(frames[-1][0], frames[-1][1], frames[-1][2], RANGES) == 0 and maps[-1].occupancy.any()
    reset_counts()
    bm.update([f[0] for f in frames], [f[1] for f in frames], [CameraGeometry(*f[2]) for f in frames], IdRanges(*RANGES))
    launched = counts_of('occupancy_maps', 'occupancy_maps_large')
    robots = robots_on_free_cells(maps, envs, rng)
    states = [[S.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle']) for r in env] for env in robots]
    got = bm.get_states(states)
    return bm, maps, robots, states, got.cpu().numpy(), launched, (bank, names)


def test_one_mapper_set_over_rooms_on_both_sides_of_both_caps(S, golden_dir):
    envs = (0, 1, 2)
    bm, maps, robots, states, got, launched, (bank, names) = chain(S, golden_dir, envs, True)
    assert bm.shapes == [(232, 232)] * 2 + [(184, 262)] * 2 + [(290, 290)] * 2
    assert bm.occupancy_entry == ['simq_occupancy_maps'] * 2 + ['simq_occupancy_maps_large'] * 4
    assert bm.action_entry == ['simq_action_waypoints'] * 4 + ['simq_action_waypoints_large'] * 2
    assert launched == [1, 1]                                                 # at most two launches for the stage, the LDS part first
    assert bm.occupancy_status.cpu().tolist() == [0] * 6
    m = 0
    for e, env in enumerate(robots):
        for r in range(len(env)):
            for name, mine, theirs in (('occupancy', bm.occupancy[m], maps[m].occupancy), ('cspace', bm.configuration_space[m], maps[m].configuration_space),
                                       ('thin', bm.cspace_thin[m], maps[m].cspace_thin), ('closest', bm.closest_cspace_indices[m], maps[m].closest)):
                assert np.array_equal(mine.cpu().numpy(), theirs), (m, name)
            want = mapper_oracle.get_state(CFG, maps[m], env, r, bank, names, RECEPTACLE)
            assert got[m].shape == want.shape and np.array_equal(got[m].view(np.int32), want.view(np.int32)), m
            m += 1

    # the fixture's maps as an update leaves them: their occupancy maps written into the object, then an update from frames of the
    # floor alone, which sets no cell, recomputes the three results
    from simq.observation import CameraGeometry, IdRanges
    rooms, cases = lr.load(golden_dir)
    rng = np.random.RandomState(23)
    done = 0
    for round_ in range(2):
        loaded = {}
        bm.reset([1, 2])
        for e in (1, 2):
            for r, t in enumerate(ENV_TYPES[e]):
                k = [k for k, fm in enumerate(rooms[e - 1]['maps']) if fm['robot_type'] == t][round_]
                loaded[bm.mapper_index(e, r)] = (e - 1, k)
                bm.occupancy[bm.mapper_index(e, r)].copy_(torch.from_numpy(rooms[e - 1]['maps'][k]['occupancy']))
        floor = [overhead_frame(rng, 0, empty=True) for _ in loaded]
        reset_counts()
        bm.update([f[0] for f in floor], [f[1] for f in floor], [CameraGeometry(*f[2]) for f in floor], IdRanges(*RANGES), mappers=sorted(loaded))
        assert counts_of('occupancy_maps', 'occupancy_maps_large') == [0, 1]
        for mapper, (room, k) in loaded.items():
            fm = rooms[room]['maps'][k]
            assert np.array_equal(bm.configuration_space[mapper].cpu().numpy(), fm['configuration_space']), (mapper, fm['name'])
            assert np.array_equal(bm.closest_cspace_indices[mapper].cpu().numpy(), fm['closest']), (mapper, fm['name'])
        where = {v: mapper for mapper, v in loaded.items()}
        mine = [c for c in cases if (c['room'], c['map']) in where and c['use_shortest_path_movement']]
        left = list(range(len(mine)))
        while left:                                                           # a call names a mapper once
            taken, now = set(), []
            for k in left:
                mapper = where[(mine[k]['room'], mine[k]['map'])]
                if mapper not in taken:
                    taken.add(mapper)
                    now.append((k, mapper))
            left = [k for k in left if k not in [n for n, _ in now]]
            # the mappers of the first environment ride along on the maps of their own update: the call mixes both sides of the cap
            seeded_rng = np.random.RandomState(100 + len(left))
            extra = robots_on_free_cells(maps[:2], (0,), seeded_rng)[0]
            extra_actions = [int(seeded_rng.randint(act_oracle.NUM_OUTPUT_CHANNELS[t] * 96 * 96)) for t in ENV_TYPES[0]]
            call_states = [[S.RobotState(r['position'] + (0,), r['heading'], r['type']) for r in extra]] + \
                [[S.RobotState((9.0, 9.0, 0), 0.0, t) for t in ENV_TYPES[e]] for e in (1, 2)]
            for k, mapper in now:
                e = bm.env_of[mapper]
                call_states[e][mapper - bm.env_begin[e]] = S.RobotState(mine[k]['position'], mine[k]['heading'], mine[k]['robot_type'])
            named = [0, 1] + [mapper for _, mapper in now]
            reset_counts()
            new = bm.store_new_actions(extra_actions + [mine[k]['a'] for k, _ in now], call_states, mappers=named)
            a, b = counts_of('action_waypoints', 'action_waypoints_large')
            assert a == 1 and b == (1 if any(mapper >= 4 for _, mapper in now) else 0)
            arrays = bm.store_new_actions(extra_actions + [mine[k]['a'] for k, _ in now], S.RobotArrays.from_states(bm, call_states), mappers=named)
            lists = new.as_lists()
            assert act_oracle.same_bits(lists, arrays.as_lists())
            for (k, mapper), out in zip(now, lists[2:]):
                c = mine[k]
                assert act_oracle.same_bits(list(out), [c['action'], c['target'], c['waypoints'], c['headings']]), (round_, k, mapper)
                done += 1
            for r in range(2):
                sp = lambda p, q, r=r: wo.occupancy_shortest_path(maps[r].configuration_space, maps[r].cspace_thin, maps[r].closest, p, q,
                                                                  so.exact)        # noqa: E731
                want = act_oracle.store_new_action(extra_actions[r], extra[r]['position'] + (0,), extra[r]['heading'], extra[r]['type'], sp)
                assert act_oracle.same_bits(list(lists[r]), list(want[:4])), (round_, r)
    assert done >= 10, done
    paths = bm.shortest_paths([(0.0, 0.0, 0)] * 2, [(0.3, 0.2, 0)] * 2, mappers=[3, 5], simplify='exact')
    assert len(paths) == 2 and all(len(p) >= 2 for p in paths)


def test_the_small_room_alone_is_as_it_was(S, golden_dir):
    """Only the 1.0 m x 1.0 m environment: with and without large_rooms the states of the oracle, one simq_occupancy_maps launch and
    no launch of a large entry."""
    results = [chain(S, golden_dir, (0,), large_rooms) for large_rooms in (False, True)]
    for bm, maps, robots, states, got, launched, (bank, names) in results:
        assert launched == [1, 0] and bm.occupancy_entry == ['simq_occupancy_maps'] * 2 and bm.action_entry == ['simq_action_waypoints'] * 2
        for r in range(2):
            want = mapper_oracle.get_state(CFG, maps[r], robots[0], r, bank, names, RECEPTACLE)
            assert np.array_equal(got[r].view(np.int32), want.view(np.int32)), r
        reset_counts()
        bm.store_new_actions([5000, 7000], states)
        assert counts_of('action_waypoints', 'action_waypoints_large') == [1, 0]
    assert np.array_equal(results[0][4].view(np.int32), results[1][4].view(np.int32))
    # without the keyword a room over the cap is refused where it was: by the library, at the update
    from simq.observation import CameraGeometry, IdRanges
    masks, _, _ = masks_of(golden_dir)
    bm = S.BatchedMapper(1.6, 1.6, [['pushing_robot']], masks)
    frame = overhead_frame(np.random.RandomState(1), 3)
    reset_counts()
    with pytest.raises(S.occupancy.SimqError, match=r'occupancy_maps: problem 0 is 290 x 290 \(rows, cols in 1 .. 256\)'):
        bm.update([frame[0]], [frame[1]], [CameraGeometry(*frame[2])], IdRanges(*RANGES))
    assert counts_of('occupancy_maps', 'occupancy_maps_large') == [0, 0]
