"""GPU: simq_action_waypoints (csrc/action_waypoints.hip) against today's pair simq_grid_paths + simq_grid_waypoints and the CPU
oracle, problem by problem; its edges (a long dense path, the window at the cap, an empty window, a short capacity, upstream words, a
free cell outside the window); BatchedMapper.store_new_actions against the reference's fixture and the scalar oracle in both argument
forms; the interplay with get_states."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import grid_simplify_oracle as so
import grid_waypoints_oracle as wo
import mapper_oracle
import store_new_action_oracle as oracle

pytestmark = pytest.mark.gpu
SENTINEL = -7


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    import simq.actions  # noqa: F401
    import simq.waypoints  # noqa: F401
    return simq


def run(cspaces, problems, thins=None, closests=None, upstream=None, expect_rc=0):
    """One simq_action_waypoints call.  cspaces (thins, closests): one array per map; problems: dicts with map, src, tgt and optionally
    box (default: the free box), capacity (pairs, default 64), line (test the thin map), snap, upstream (index).  Every problem's
    waypoint range is followed by one sentinel pair, every output is sentinel-filled.  Returns (waypoints as written up to min(count,
    capacity), counts, status, end pixels), having checked that nothing lies beyond."""
    from simq._lib import lib, ptr, stream_ptr
    from simq.actions import ActionWaypointProblem
    dev = torch.device('cuda', torch.cuda.current_device())
    at = np.concatenate([[0], np.cumsum([g.size for g in cspaces])])
    P = len(problems)
    probs = (ActionWaypointProblem * P)()
    wo_, caps = 0, []
    for p, q in enumerate(problems):
        m = q['map']
        rows, cols = cspaces[m].shape
        caps.append(int(q.get('capacity', 64)))
        probs[p] = ActionWaypointProblem(int(at[m]), int(at[m]) if q.get('line') else -1, 2 * int(at[m]) if q.get('snap') else -1, wo_, caps[-1],
                                         rows, cols, *q['src'], *q['tgt'], *q.get('box', wo.free_box(cspaces[m])), q.get('upstream', -1))
        wo_ += caps[-1] + 1
    flat = lambda maps, dt: None if maps is None else torch.from_numpy(np.concatenate([np.asarray(g, dt).reshape(-1) for g in maps])).to(dev)
    d_cspace, d_thin, d_closest = flat(cspaces, np.uint8), flat(thins, np.uint8), flat(closests, np.int32)
    d_up = None if upstream is None else torch.tensor(upstream, dtype=torch.int32, device=dev)
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    d_ways = torch.full((wo_, 2), SENTINEL, dtype=torch.int32, device=dev)
    d_counts, d_status = (torch.full((P,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2))
    d_ends = torch.full((P, 4), SENTINEL, dtype=torch.int32, device=dev)
    rc = lib.c.simq_action_waypoints(ptr(d_cspace), d_cspace.numel(), ptr(d_thin), 0 if d_thin is None else d_thin.numel(), ptr(d_closest),
                                     0 if d_closest is None else d_closest.numel(), probs, P, ptr(d_probs), ptr(d_ways), wo_, ptr(d_counts),
                                     ptr(d_ends), ptr(d_up), 0 if d_up is None else d_up.numel(), ptr(d_status), stream_ptr(dev))
    assert rc == expect_rc, (rc, lib.c.simq_last_error())
    ways, counts, status, ends = d_ways.cpu().numpy(), d_counts.cpu().numpy(), d_status.cpu().numpy(), d_ends.cpu().numpy()
    out, o = [], 0
    for p in range(P):
        n = max(0, min(int(counts[p]), caps[p])) if status[p] in (0, 3) else 0
        out.append(ways[o:o + n])
        assert (ways[o + n:o + caps[p] + 1] == SENTINEL).all(), p
        o += caps[p] + 1
    return out, counts, status, ends


def grid_oracle(grid, s, t):
    """The waypoints of the exact rule on a plain grid (no line test, no snap)."""
    return so.waypoints(grid, wo.dense_path(wo.spfa(grid, s)[1], s, t))


# ---- 1: the C entry against today's pair and the oracle ----------------------------------------------------------------------------
def test_random_grids_equal_todays_pair_and_the_oracle(S):
    cases = wo.random_grids()
    grids = [c[0] for c in cases]
    got, counts, status, ends = run(grids, [dict(map=p, src=s, tgt=t) for p, (_, s, t) in enumerate(cases)])
    pair = S.grid_waypoints(grids, [c[1] for c in cases], [c[2] for c in cases])
    assert (status == 0).all() and np.array_equal(status, pair.status) and np.array_equal(ends, pair.endpoints)
    bent = 0
    for p, (grid, s, t) in enumerate(cases):
        want = grid_oracle(grid, s, t)
        assert counts[p] == len(want) == len(pair.waypoints[p]), p
        assert np.array_equal(got[p], pair.waypoints[p]) and np.array_equal(got[p], want), p
        bent += len(want) > 2
    assert bent >= 20


@pytest.mark.parametrize('room', oracle.ROOMS)
def test_occupancy_problems_equal_todays_pair_and_the_oracle(S, golden_dir, room):
    cspace, thin, closest, problems = wo.occupancy_problems(golden_dir, room)
    shape = cspace.shape[1:]
    src = [wo.position_to_pixel_indices(a[0], a[1], shape) for _, a, _ in problems]
    tgt = [wo.position_to_pixel_indices(b[0], b[1], shape) for _, _, b in problems]
    index = [m for m, _, _ in problems]
    got, counts, status, ends = run(list(cspace), [dict(map=m, src=s, tgt=t, line=True, snap=True) for m, s, t in zip(index, src, tgt)],
                                    list(thin), list(closest))
    pair = S.grid_waypoints(cspace, src, tgt, grid_index=index, thin=thin, closest=closest)
    assert np.array_equal(status, pair.status) and np.array_equal(ends, pair.endpoints)
    cache = {}
    for p, m in enumerate(index):
        st, want, e = oracle.pixel_waypoints(cspace[m], thin[m], closest[m], src[p], tgt[p], cache.setdefault(m, {}))
        assert (status[p], counts[p], tuple(ends[p])) == (st, len(want), e), p
        assert np.array_equal(got[p], want) and np.array_equal(got[p], pair.waypoints[p]), p
    assert (status == 1).sum() >= 8 and (counts > 2).sum() >= 8


def test_cells_that_are_free_but_not_one(S):
    """A cell of 2 is free for the search and blocks the pruning's line, as in simq_grid_waypoints: the flag bytes keep both."""
    rng = np.random.RandomState(4)
    grid = (rng.rand(40, 50) < 0.9).astype(np.uint8)
    grid[rng.rand(40, 50) < 0.08] = 2
    free = np.argwhere(grid != 0)
    picks = [(tuple(int(x) for x in free[a]), tuple(int(x) for x in free[b])) for a, b in rng.randint(len(free), size=(24, 2))]
    got, counts, status, _ = run([grid], [dict(map=0, src=s, tgt=t) for s, t in picks])
    pair = S.grid_waypoints([grid], [s for s, _ in picks], [t for _, t in picks], grid_index=[0] * len(picks))
    differs = 0
    for p, (s, t) in enumerate(picks):
        want = grid_oracle(grid, s, t)
        assert status[p] == 0 and np.array_equal(got[p], want) and np.array_equal(got[p], pair.waypoints[p]), p
        differs += len(want) != len(grid_oracle((grid != 0).astype(np.uint8), s, t))
    assert differs >= 1


# ---- 2: the dense path stays in LDS --------------------------------------------------------------------------------------------------
def serpentine(n=41):
    grid = np.ones((n, n), np.uint8)
    grid[1::2, :] = 0
    grid[1::4, -1] = 1
    grid[3::4, 0] = 1
    return grid


def test_long_dense_path_in_one_library_call(S, monkeypatch):
    from simq import actions
    from simq._lib import Lib
    grid = serpentine()
    s, t = (0, 0), (40, 0)
    dense = wo.dense_path(wo.spfa(grid, s)[1], s, t)
    want = so.waypoints(grid, dense)
    assert len(dense) > 2 * (41 + 41) + 8 and 2 < len(want) <= actions.WAY_CAPACITY
    calls = []
    call = Lib.call
    monkeypatch.setattr(Lib, 'call', staticmethod(lambda name, *a, **k: calls.append(name) or call(name, *a, **k)))
    dev = torch.device('cuda', torch.cuda.current_device())
    probs = np.zeros(1, actions.ACTION_PROBLEM)
    probs['thin_offset'] = probs['closest_offset'] = probs['upstream'] = -1
    probs['rows'] = probs['cols'] = probs['box_rows'] = probs['box_cols'] = 41
    probs['tgt_i'] = 40
    status, counts, ends, pixels, words = actions.run_problems(probs, (torch.from_numpy(grid).to(dev).view(-1), None, None))
    assert calls == ['simq_action_waypoints'] and status.tolist() == [0] and ends.tolist() == [[0, 0, 40, 0]] and words.tolist() == [0]
    assert np.array_equal(pixels, want)
    del calls[:]
    pair = S.grid_waypoints([grid], [s], [t])                               # today's route: two rounds of two entries
    assert calls == ['simq_grid_paths', 'simq_grid_waypoints'] * 2 and np.array_equal(pair.waypoints[0], want)


def test_dense_path_past_one_ballot_of_the_kept_mask(S):
    """next_kept searches 64 mask words (2 048 points) a ballot and the reversed output carries the ranks from one chunk of 64 words to
    the next: a dense path longer than that takes the second trip of both loops of csrc/waypoint_rule.h, in both routes."""
    grid = serpentine(73)
    s, t = (0, 0), (72, 0)
    dense = wo.dense_path(wo.spfa(grid, s)[1], s, t)
    want = so.waypoints(grid, dense)
    assert len(dense) > 2048 + 64 and 2 < len(want) <= 64
    got, counts, status, ends = run([grid], [dict(map=0, src=s, tgt=t, capacity=64)])
    assert status.tolist() == [0] and counts.tolist() == [len(want)] and ends.tolist() == [[0, 0, 72, 0]]
    assert np.array_equal(got[0], want)
    pair = S.grid_waypoints([grid], [s], [t])                               # a second round gives the dense path its room
    assert pair.status.tolist() == [0] and np.array_equal(pair.waypoints[0], want)


def test_window_at_the_cap(S):
    grid = np.zeros((100, 200), np.uint8)
    grid[1:99, 1:199] = 1                                                   # 98 x 198 free cells: 20 000 with the halo
    grid[10:90, 60] = grid[20:99, 120] = 0
    grid[1:80, 160] = 0
    s, t = (50, 3), (97, 197)
    got, counts, status, ends = run([grid], [dict(map=0, src=s, tgt=t, box=(1, 1, 98, 198))])
    want = grid_oracle(grid, s, t)
    assert status[0] == 0 and len(want) > 3 and np.array_equal(got[0], want) and ends[0].tolist() == [50, 3, 97, 197]
    # one cell more is refused on the host and nothing is written
    _, counts, status, ends = run([grid], [dict(map=0, src=s, tgt=t, box=(1, 1, 98, 199))], expect_rc=-1)
    assert counts[0] == status[0] == SENTINEL and (ends == SENTINEL).all()


def test_empty_window_blocked_source_and_short_paths(S):
    closed = np.zeros((12, 14), np.uint8)
    pocket = closed.copy()
    pocket[1:5, 1:13] = 1
    pocket[7:11, 3:9] = 1
    problems = [(closed, (2, 2), (5, 5)),                                  # a window without a free cell
                (pocket, (5, 5), (2, 2)),                                  # a blocked source
                (pocket, (2, 2), (5, 5)),                                  # a blocked target
                (pocket, (2, 2), (8, 5)),                                  # an unreachable target
                (pocket, (8, 5), (8, 5)),                                  # target == source
                (pocket, (0, 0), (2, 2)),                                  # a blocked source outside the window
                (pocket, (1, 1), (11, 13)),                                # a target outside the window
                (pocket, (1, 1), (4, 12)), (pocket, (2, 2), (2, 3))]       # a clear diagonal, two neighbours
    grids = [closed, pocket]
    got, counts, status, ends = run(grids, [dict(map=int(g is pocket), src=s, tgt=t) for g, s, t in problems])
    pair = S.grid_waypoints([g for g, _, _ in problems], [s for _, s, _ in problems], [t for _, _, t in problems])
    for p, (g, s, t) in enumerate(problems):
        want = grid_oracle(g, s, t)
        assert status[p] == 0 and counts[p] == len(want) and np.array_equal(got[p], want) and np.array_equal(got[p], pair.waypoints[p]), p
        assert ends[p].tolist() == list(s) + list(t)
    assert counts[:7].tolist() == [1] * 7 and counts[7:].tolist() == [2, 2]


def test_short_capacity_and_the_second_round(S, monkeypatch):
    from simq import actions
    from simq._lib import Lib
    grid = serpentine(21)
    s, t = (0, 0), (20, 0)
    want = grid_oracle(grid, s, t)
    assert len(want) >= 10
    other = np.ones((9, 9), np.uint8)
    problems = [dict(map=1, src=(0, 0), tgt=(8, 8), capacity=2), dict(map=0, src=s, tgt=t, capacity=len(want) - 1), dict(map=1, src=(8, 0), tgt=(0, 8))]
    got, counts, status, _ = run([grid, other], problems)
    assert status.tolist() == [0, 3, 0] and counts.tolist() == [2, len(want), 2]
    assert np.array_equal(got[1], want[:len(want) - 1])                    # source first, cut at the capacity, nothing past it
    assert got[0].tolist() == [[0, 0], [8, 8]] and got[2].tolist() == [[8, 0], [0, 8]]
    # the Python layer recovers with one more call
    calls = []
    call = Lib.call
    monkeypatch.setattr(Lib, 'call', staticmethod(lambda name, *a, **k: calls.append(name) or call(name, *a, **k)))
    dev = torch.device('cuda', torch.cuda.current_device())
    flat = torch.from_numpy(np.concatenate([grid.reshape(-1), other.reshape(-1)])).to(dev)
    probs = np.zeros(3, actions.ACTION_PROBLEM)
    probs['thin_offset'] = probs['closest_offset'] = probs['upstream'] = -1
    probs['cspace_offset'] = [grid.size, 0, grid.size]
    probs['rows'] = probs['cols'] = probs['box_rows'] = probs['box_cols'] = [9, 21, 9]
    probs['src_i'], probs['src_j'], probs['tgt_i'], probs['tgt_j'] = [0, 0, 8], [0, 0, 0], [8, 20, 0], [8, 0, 8]
    status, counts, ends, pixels, _ = actions.run_problems(probs, (flat, None, None), capacity=4)
    assert calls == ['simq_action_waypoints'] * 2 and status.tolist() == [0, 0, 0] and counts.tolist() == [2, len(want), 2]
    assert np.array_equal(pixels, np.concatenate([[[0, 0], [8, 8]], want, [[8, 0], [0, 8]]]))


def test_upstream_words_pass_through(S, golden_dir):
    cspace, thin, closest, problems = wo.occupancy_problems(golden_dir, '184x232', per_kind=4)
    shape = cspace.shape[1:]
    index = [m for m, _, _ in problems]
    src = [wo.position_to_pixel_indices(a[0], a[1], shape) for _, a, _ in problems]
    tgt = [wo.position_to_pixel_indices(b[0], b[1], shape) for _, _, b in problems]
    words = [0, 4, 0, 1, 77, 0, 0, 0]
    ups = [0, 1, -1, 3, 4, 5, 2, -1]
    got, counts, status, ends = run(list(cspace), [dict(map=m, src=s, tgt=t, line=True, snap=True, upstream=u)
                                                   for m, s, t, u in zip(index, src, tgt, ups)], list(thin), list(closest), upstream=words)
    for p, m in enumerate(index):
        if ups[p] >= 0 and words[ups[p]] != 0:                             # the word, count 0, nothing else written
            assert (status[p], counts[p]) == (words[ups[p]], 0) and (ends[p] == SENTINEL).all() and len(got[p]) == 0, p
            continue
        st, want, e = oracle.pixel_waypoints(cspace[m], thin[m], closest[m], src[p], tgt[p])
        assert (status[p], counts[p], tuple(ends[p])) == (st, len(want), e) and np.array_equal(got[p], want), p


def test_a_free_cell_outside_the_window_is_status_2(S):
    grid = np.ones((20, 30), np.uint8)
    grid[3:17, 15] = 0
    ok = dict(map=0, src=(10, 2), tgt=(10, 28))
    got, counts, status, ends = run([grid], [ok, dict(ok, box=(0, 0, 20, 29)), dict(ok, box=(1, 0, 19, 30)), ok])
    want = grid_oracle(grid, (10, 2), (10, 28))
    assert status.tolist() == [0, 2, 2, 0] and counts.tolist() == [len(want), SENTINEL, SENTINEL, len(want)]
    assert (ends[1:3] == SENTINEL).all() and np.array_equal(got[0], want) and np.array_equal(got[3], want)


# ---- 3: BatchedMapper.store_new_actions ----------------------------------------------------------------------------------------------
ROOM_SIZES = {'184x232': (0.5, 1.0), '232x232': (1.0, 1.0)}


@pytest.fixture(scope='module')
def cases(golden_dir):
    return oracle.load_cases(golden_dir)


def loaded_mapper(S, golden_dir, room):
    """An object whose mapper 4 * k + r is a robot of type ROBOT_TYPES[r] on map k of the room's occupancy fixture: the maps the
    reference's fixture was computed on, written into the object's tensors as an update leaves them."""
    cspace, thin, closest = oracle.maps(golden_dir, room)
    masks = {name: np.zeros((96, 96), np.float32) for name in oracle.ROBOT_TYPES + ('lifting_robot_with_cube',)}
    bm = S.BatchedMapper(*ROOM_SIZES[room], [list(oracle.ROBOT_TYPES)] * len(cspace), masks)
    assert bm.shapes[0] == cspace.shape[1:]
    for name, maps in (('configuration_space', cspace), ('cspace_thin', thin), ('closest_cspace_indices', closest)):
        getattr(bm, name).copy_(torch.from_numpy(np.repeat(maps, 4, axis=0)))
    bm.occupancy_status.copy_(torch.from_numpy(np.repeat([0 if c.any() else 1 for c in cspace], 4).astype(np.int32)))
    return bm


@pytest.mark.parametrize('room', oracle.ROOMS)
def test_batched_mapper_equals_the_fixture_in_both_forms(S, golden_dir, cases, room):
    bm = loaded_mapper(S, golden_dir, room)
    mine = [c for c in cases if c['room'] == room]
    rng = np.random.RandomState(3)
    left, rounds = list(rng.permutation(len(mine))), 0
    while left:                                                             # a call names a mapper once: the cases in shuffled rounds
        taken, now = set(), []
        for k in list(left):
            m = 4 * mine[k]['map'] + oracle.ROBOT_TYPES.index(mine[k]['robot_type'])
            if m not in taken and mine[k]['use_shortest_path_movement'] == mine[left[0]]['use_shortest_path_movement']:
                taken.add(m)
                now.append((k, m))
        left = [k for k in left if k not in [n for n, _ in now]]
        ms = [m for _, m in now]
        sp = mine[now[0][0]]['use_shortest_path_movement']
        states = [[S.RobotState((9.0, 9.0, 0), 0.0, t) for t in oracle.ROBOT_TYPES] for _ in range(bm.num_envs)]
        for k, m in now:
            states[m // 4][m % 4] = S.RobotState(mine[k]['position'], mine[k]['heading'], mine[k]['robot_type'])
        a = [mine[k]['a'] for k, _ in now]
        lists = bm.store_new_actions(a, states, mappers=ms, use_shortest_path_movement=sp)
        arrays = bm.store_new_actions(a, S.RobotArrays.from_states(bm, states), mappers=ms, use_shortest_path_movement=sp)
        assert oracle.same_bits(lists.as_lists(), arrays.as_lists()) and np.array_equal(lists.status, arrays.status)
        for (k, m), got in zip(now, lists.as_lists()):
            c = mine[k]
            assert oracle.same_bits(list(got), [c['action'], c['target'], c['waypoints'], c['headings']]), (room, k)
            assert got[2][0] is c['position']
        rounds += 1
    assert rounds >= 2


@pytest.fixture(scope='module')
def updated(S, golden_dir):
    """An object over both mapper fixtures after the update of round 0, and its episodes; only read by the tests that share it."""
    from test_gpu_mapper import CONFIGS, build, frames_of
    episodes = [mapper_oracle.load_fixture(f) for f in sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))]
    bm = build(S, episodes, CONFIGS['full_spatial'])
    bm.update(*frames_of(S, [ep['rounds'][0] for ep in episodes]))
    return bm, episodes


def seeded_robots(S, bm, seed):
    """Robots on free cells of their mappers' configuration spaces, seeded; (states, actions)."""
    rng = np.random.RandomState(seed)
    states, actions = [], []
    for e in range(bm.num_envs):
        env = []
        for r, t in enumerate(bm.robot_types[e]):
            m = bm.mapper_index(e, r)
            cs = bm.configuration_space[m].cpu().numpy()
            i, j = np.argwhere(cs != 0)[rng.randint(int((cs != 0).sum()))]
            x, y = wo.pixel_indices_to_position(i + float(rng.uniform(-0.4, 0.4)), j + float(rng.uniform(-0.4, 0.4)), cs.shape)
            env.append(S.RobotState((float(x), float(y), 0), float(rng.uniform(-np.pi, np.pi)), t))
            actions.append(int(rng.randint(oracle.NUM_OUTPUT_CHANNELS[t] * 96 * 96)))
        states.append(env)
    return states, actions


def test_batched_mapper_after_the_golden_update_equals_the_oracle(S, updated, monkeypatch):
    from simq._lib import Lib
    bm, _ = updated
    maps = [[x[m].cpu().numpy() for x in (bm.configuration_space, bm.cspace_thin, bm.closest_cspace_indices)] for m in range(bm.num_mappers)]
    for seed, ms in ((1, None), (2, [4, 1, 5, 0]), (3, [2, 3]), (4, [5, 0])):   # all; shuffled subsets; two robots sharing nothing
        states, actions = seeded_robots(S, bm, seed)
        named = list(range(bm.num_mappers)) if ms is None else ms
        got = bm.store_new_actions([actions[m] for m in named], states, mappers=ms)
        arrays = bm.store_new_actions([actions[m] for m in named], S.RobotArrays.from_states(bm, states), mappers=ms)
        assert oracle.same_bits(got.as_lists(), arrays.as_lists())
        for m, g in zip(named, got.as_lists()):
            r = states[bm.env_of[m]][m - bm.env_begin[bm.env_of[m]]]
            sp = lambda a, b, m=m: wo.occupancy_shortest_path(*maps[m], a, b, so.exact)      # noqa: E731
            want = oracle.store_new_action(actions[m], r.position, r.heading, r.robot_type, sp)
            assert oracle.same_bits(list(g), list(want[:4])), (seed, m)
    # without shortest paths the library is not called
    calls = []
    monkeypatch.setattr(Lib, 'call', staticmethod(lambda name, *a, **k: calls.append(name)))
    plain = bm.store_new_actions(actions, states, use_shortest_path_movement=False)
    assert calls == [] and plain.offsets.tolist() == list(range(0, 2 * bm.num_mappers + 1, 2))
    for m, g in enumerate(plain.as_lists()):
        r = states[bm.env_of[m]][m - bm.env_begin[bm.env_of[m]]]
        assert oracle.same_bits(list(g), list(oracle.store_new_action(actions[m], r.position, r.heading, r.robot_type)[:4]))


def test_batched_mapper_reports_mappers_and_refuses_pending_frames(S, golden_dir):
    from test_gpu_mapper import CONFIGS, build, frames_of, pick
    episodes = [mapper_oracle.load_fixture(f) for f in sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))]
    bm = build(S, episodes, CONFIGS['overhead_only'])
    frames = frames_of(S, [ep['rounds'][0] for ep in episodes])
    bm.update(*pick(frames, [0, 1, 3, 4, 5]), mappers=[0, 1, 3, 4, 5])      # mapper 2 never had an update
    states, actions = [[S.RobotState((0.0, 0.0, 0), 0.3, t) for t in env] for env in bm.robot_types], [100] * 6
    with pytest.raises(S.actions.SimqError, match=r'mapper\(s\) 2 \(environment 0, robot 2\)') as e:
        bm.store_new_actions(actions, states)
    assert str(e.value).split('mapper(s) ')[1].split(' (simq_action')[0] == '2 (environment 0, robot 2)' and 'status [4]' in str(e.value)
    assert len(bm.store_new_actions([100] * 5, states, mappers=[5, 4, 3, 1, 0])) == 5
    bm.defer(*pick(frames, [4]), mappers=[4])
    with pytest.raises(S.actions.SimqError, match='deferred frames'):
        bm.store_new_actions(actions, states)
    assert len(bm.store_new_actions([100, 100], states, mappers=[0, 1])) == 2


# ---- 4: the interplay with get_states ----------------------------------------------------------------------------------------------
def test_waypoints_go_into_get_states_as_they_are(S, updated):
    from test_gpu_mapper import states_of
    bm, episodes = updated
    robots = states_of(S, [ep['rounds'][0] for ep in episodes])
    before = bm.get_states(robots).cpu().numpy()
    ra = S.RobotArrays.from_states(bm, robots)
    new = bm.store_new_actions([3000 + 17 * m for m in range(bm.num_mappers)], ra)
    assert np.array_equal(bm.get_states(robots).cpu().numpy().view(np.int32), before.view(np.int32))          # nothing of the maps changed
    lists = new.as_lists()
    moved = [[r._replace(target=lists[bm.mapper_index(e, k)][1], intention_path=lists[bm.mapper_index(e, k)][2])
              for k, r in enumerate(env)] for e, env in enumerate(robots)]
    want = bm.get_states(moved).cpu().numpy()
    packed = S.RobotArrays(ra.position, ra.heading, ra.lifting, ra.idle, new.target_end_effector_position,
                           (new.waypoint_positions, new.offsets), ra.history_path)
    got = bm.get_states(packed).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and not np.array_equal(want, before)
