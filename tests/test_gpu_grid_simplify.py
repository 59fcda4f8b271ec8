"""GPU: simq_grid_waypoints (csrc/grid_simplify.hip) against the exact rule and the pruning in Python integers
(tests/grid_simplify_oracle.py), bit for bit: the dense paths of the fixtures uploaded as they are, random lattice walks on two
grids at two tolerances, the degenerate and refused cases, and simplify='exact' end to end with its read-backs counted."""
import ctypes
import os

import numpy as np
import pytest
import torch

import grid_simplify_oracle as so
import grid_waypoints_oracle as oracle
from test_grid_simplify_cpu import fixture_paths

pytestmark = pytest.mark.gpu
SENTINEL = -7


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    import simq.waypoints  # noqa: F401
    return simq


def run(grids, problems):
    """One simq_grid_waypoints call.  grids: uint8 arrays; problems: dicts with grid (index), path (int [n, 2]) and optionally
    tolerance, capacity (pairs, default n), path_status, length (default n).  Every problem's waypoint range is followed by one
    sentinel pair.  Returns (waypoints as written, up to min(count, capacity) pairs each; counts; status; the sentinel pairs)."""
    from simq._lib import lib, ptr, stream_ptr
    from simq.waypoints import GridWaypointProblem
    dev = torch.device('cuda', torch.cuda.current_device())
    goff = np.concatenate([[0], np.cumsum([g.size for g in grids])])
    P = len(problems)
    probs = (GridWaypointProblem * P)()
    po = wo = 0
    caps = []
    for p, q in enumerate(problems):
        n = len(q['path'])
        caps.append(int(q.get('capacity', n)))
        rows, cols = grids[q['grid']].shape
        probs[p] = GridWaypointProblem(int(goff[q['grid']]), po, wo, rows, cols, caps[-1], int(q.get('tolerance', 1)))
        po += n
        wo += caps[-1] + 1
    d_grids = torch.from_numpy(np.concatenate([g.reshape(-1) for g in grids])).to(dev)
    d_paths = torch.from_numpy(np.concatenate([np.asarray(q['path'], np.int32).reshape(-1, 2) for q in problems])).to(dev)
    d_lengths = torch.tensor([q.get('length', len(q['path'])) for q in problems], dtype=torch.int32, device=dev)
    d_pstatus = torch.tensor([q.get('path_status', 0) for q in problems], dtype=torch.int32, device=dev)
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    d_ways = torch.full((wo, 2), SENTINEL, dtype=torch.int32, device=dev)
    d_counts = torch.full((P,), SENTINEL, dtype=torch.int32, device=dev)
    d_status = torch.full((P,), SENTINEL, dtype=torch.int32, device=dev)
    lib.call('simq_grid_waypoints', ptr(d_grids), ctypes.c_int64(d_grids.numel()), ptr(d_paths), ctypes.c_int64(po), ptr(d_lengths),
             ptr(d_pstatus), probs, P, ptr(d_probs), ptr(d_ways), ctypes.c_int64(wo), ptr(d_counts), ptr(d_status), stream_ptr(dev))
    ways, counts, status = d_ways.cpu().numpy(), d_counts.cpu().numpy(), d_status.cpu().numpy()
    out, behind, o = [], [], 0
    for p in range(P):
        out.append(ways[o:o + max(0, min(int(counts[p]), caps[p]))])
        behind.append(ways[o + caps[p]])
        assert (ways[o + max(0, min(int(counts[p]), caps[p])):o + caps[p] + 1] == SENTINEL).all(), p
        o += caps[p] + 1
    return out, counts, status, behind


def test_fixture_dense_paths_in_one_launch(simq_mod, golden_dir):
    """Every dense path of the fixtures (lengths 1 to 1 451) against the rule and the pruning on its own grid."""
    cases = fixture_paths(golden_dir)
    keys = []
    for key, _, _ in cases:
        if key not in keys:
            keys.append(key)
    grids = [next(g for k, g, _ in cases if k == key) for key in keys]
    problems = [dict(grid=keys.index(key), path=d) for key, _, d in cases]
    lengths = [len(d) for _, _, d in cases]
    assert len(problems) >= 900 and min(lengths) == 1 and max(lengths) >= 1400
    out, counts, status, _ = run(grids, problems)
    assert (status == 0).all(), np.flatnonzero(status != 0)[:8]
    kept = 0
    for p, (key, grid, d) in enumerate(cases):
        want = so.waypoints(grid, d)
        assert counts[p] == len(want) and np.array_equal(out[p], want), (key, p)
        kept += len(want) > 2
    assert kept >= 100                                                          # pruning kept an interior waypoint


def test_random_walks_on_two_grids_at_two_tolerances(simq_mod):
    walks, grids = so.random_walks(), so.walk_grids()
    problems = [dict(grid=k, path=w, tolerance=t) for t in (1, 2) for k in (0, 1) for w in walks]
    out, counts, status, _ = run(list(grids), problems)
    assert (status == 0).all(), np.flatnonzero(status != 0)[:8]
    dropped = kept = 0
    for p, q in enumerate(problems):
        want = so.waypoints(grids[q['grid']], q['path'], q['tolerance'])
        assert counts[p] == len(want) and np.array_equal(out[p], want), p
        sparse = len(so.exact(q['path'], q['tolerance']))
        dropped += len(want) < sparse
        kept += len(want) > 2
    assert dropped >= 1000 and kept >= 1000


def test_degenerate_and_refused_problems(simq_mod):
    grid = np.ones((40, 50), np.uint8)
    grid[10:30, 25] = 0
    corner = np.asarray([(35, 5)] * 1 + [(35 - i, 5) for i in range(1, 31)] + [(5, 5 + j) for j in range(1, 41)], np.int32)
    zigzag = np.asarray([(20 + 3 * (k % 2), 2 + 2 * k) for k in range(20)], np.int32)      # on a grid without a 1 nothing is pruned
    closed, wide = np.zeros((40, 50), np.uint8), np.ones((2, 32768), np.uint8)
    grids = [grid, wide, closed]
    paths = [np.asarray(pts, np.int32) for pts in ([(3, 3)], [(3, 3), (4, 4)], [(3, 3), (3, 3)], [(3, 3), (5, 4), (3, 5)],
                                                    [(3, 3), (4, 4), (5, 5)], [(3, 3), (3, 4), (3, 3)])]
    problems = [dict(grid=0, path=d) for d in paths]                                        # 0-5: n = 1, 2, 3
    problems += [dict(grid=2, path=zigzag),                                                 # 6
                 dict(grid=0, path=corner, path_status=1, length=0),                        # 7: the search said straight line
                 dict(grid=0, path=corner),                                                 # 8
                 dict(grid=0, path=corner, path_status=3, length=500),                      # 9: cut short by its capacity
                 dict(grid=2, path=zigzag, tolerance=2),                                    # 10
                 dict(grid=2, path=zigzag, capacity=len(so.waypoints(closed, zigzag)) - 1), # 11: one pair short
                 dict(grid=2, path=zigzag),                                                 # 12
                 dict(grid=1, path=np.asarray([(0, 5), (1, 32768), (0, 90)], np.int32)),    # 13: a coordinate of 2^15
                 dict(grid=1, path=np.asarray([(0, 5), (1, 32767), (0, 90)], np.int32)),    # 14: ... and the largest legal one
                 dict(grid=0, path=np.asarray([(3, 3), (-1, 4), (3, 5)], np.int32)),        # 15
                 dict(grid=0, path=np.asarray([(3, 3), (4, 50), (3, 5)], np.int32)),        # 16
                 dict(grid=0, path=corner, path_status=2),                                  # 17: a failed search
                 dict(grid=0, path=corner, length=0),                                       # 18
                 dict(grid=0, path=corner, length=10 ** 6),                                 # 19: beyond d_paths and the flag mask
                 dict(grid=0, path=corner)]                                                 # 20
    out, counts, status, behind = run(grids, problems)
    expect = {7: (1, 0), 9: (1, -1), 11: (3, len(so.waypoints(closed, zigzag))), 13: (2, SENTINEL), 15: (2, SENTINEL), 16: (2, SENTINEL),
              17: (2, SENTINEL), 18: (2, SENTINEL), 19: (2, SENTINEL)}
    for p, q in enumerate(problems):
        assert all((b == SENTINEL).all() for b in behind), p
        if p in expect:
            assert (status[p], counts[p]) == expect[p], (p, status[p], counts[p])
            if status[p] != 3:
                assert len(out[p]) == 0, p
            continue
        want = so.waypoints(grids[q['grid']], q['path'], q.get('tolerance', 1))
        assert status[p] == 0 and counts[p] == len(want) and np.array_equal(out[p], want), p
    want = so.waypoints(closed, zigzag)
    assert len(want) >= 10 and np.array_equal(out[11], want[:len(want) - 1])               # source first, cut at the capacity
    assert len(so.waypoints(grid, corner)) == 3 and 2 < len(so.waypoints(closed, zigzag, 2)) < len(want)


@pytest.mark.parametrize('room', ['184x232', '232x232'])
def test_shortest_paths_exact_end_to_end(simq_mod, golden_dir, room):
    """simq.shortest_paths(simplify='exact') on the occupancy fixture against OccupancyMap.shortest_path with the rule as its
    simplifier -- straight lines and paths of fewer than two waypoints included -- and against the same call with the host form."""
    cspace, thin, closest, problems = oracle.occupancy_problems(golden_dir, room)
    args = (cspace, thin, closest, [a for _, a, _ in problems], [b for _, _, b in problems])
    got = simq_mod.shortest_paths(*args, map_index=[m for m, _, _ in problems], simplify='exact')
    host = simq_mod.shortest_paths(*args, map_index=[m for m, _, _ in problems], simplify=simq_mod.approximate_polygon_exact)
    assert got == host
    straight, cache = 0, {}
    for (m, a, b), path in zip(problems, got):
        want = oracle.occupancy_shortest_path(cspace[m], thin[m], closest[m], a, b, so.exact, cache.setdefault(m, {}))
        assert path == want, (m, a, b)
        assert path[0] is a and path[-1] is b
        straight += len(want) == 2
    assert straight >= len(problems) // 4 and len(problems) - straight >= len(problems) // 4
    # a source on its target: a dense path of one point, fewer than two waypoints
    m, a, _ = problems[1]
    assert simq_mod.shortest_paths(cspace, thin, closest, [a], [a], map_index=[m], simplify='exact') == [[a, a]]


def test_batched_mapper_shortest_paths_exact(simq_mod, golden_dir):
    """BatchedMapper.shortest_paths(simplify='exact') on the maps of mapper_184x232.npz against the oracle on the same maps."""
    import mapper_oracle
    from test_gpu_mapper import CONFIGS, build, frames_of
    episode = mapper_oracle.load_fixture(os.path.join(golden_dir, 'mapper_184x232.npz'))
    mapper = build(simq_mod, [episode], CONFIGS['full_spatial'], (0, 0))
    mapper.update(*frames_of(simq_mod, [episode['rounds'][0]] * 2))
    cspace, thin = mapper.configuration_space.cpu().numpy(), mapper.cspace_thin.cpu().numpy()
    closest = mapper.closest_cspace_indices.cpu().numpy()
    M, shape = cspace.shape[0], cspace.shape[1:]
    rng = np.random.RandomState(11)
    half_x, half_y = shape[1] / 2 / oracle.PIXELS_PER_METER, shape[0] / 2 / oracle.PIXELS_PER_METER
    mappers = [m for m in range(M) if cspace[m].any()]
    bent = 0
    for _ in range(4):                                                            # (a call names each mapper once)
        sources = [(float(rng.uniform(-half_x, half_x)), float(rng.uniform(-half_y, half_y)), 0.0) for _ in mappers]
        targets = [(float(rng.uniform(-half_x, half_x)), float(rng.uniform(-half_y, half_y)), 0.0) for _ in mappers]
        got = mapper.shortest_paths(sources, targets, mappers=mappers, simplify='exact')
        for m, a, b, path in zip(mappers, sources, targets, got):
            want = oracle.occupancy_shortest_path(cspace[m], thin[m], closest[m], a, b, so.exact)
            assert path == want, (m, a, b)
            bent += len(want) > 2
    assert bent >= 1


def test_exact_reads_back_once(simq_mod, golden_dir, monkeypatch):
    """simplify='exact' makes one device-to-host copy for the whole call: status words, counts, end pixels and waypoints in one
    array, and no dense path or map.  A second one follows only when a dense path overflowed its first buffer.  (Maps that are device
    tensors cost the download of their free-cell boxes, four integers a map, before the search is queued -- grid_dense_paths' own.)"""
    from simq import waypoints
    from simq._lib import lib
    cspace, thin, closest, problems = oracle.occupancy_problems(golden_dir, '184x232')
    args = ([a for _, a, _ in problems], [b for _, _, b in problems])
    copies = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda t, *a, **k: copies.append(t.numel()) or cpu(t, *a, **k))
    lib.call('simq_launch_counts_reset')
    got = simq_mod.shortest_paths(cspace, thin, closest, *args, map_index=[m for m, _, _ in problems], simplify='exact')
    assert len(copies) == 1 and copies[0] <= len(problems) * (8 + 2 * waypoints.WAY_CAPACITY) + 1, copies
    assert lib.c.simq_launch_count(b'grid_waypoints') == 1 and lib.c.simq_launch_count(b'grid_simplify') == 1
    # device-resident maps: the boxes first, then the one array
    dev = torch.device('cuda', torch.cuda.current_device())
    on_device = [torch.from_numpy(x).to(dev) for x in (cspace, thin, closest)]
    del copies[:]
    inside_boxes = []
    boxes = waypoints._boxes

    def counted_boxes(*a):
        before = len(copies)
        found = boxes(*a)
        inside_boxes.append(len(copies) - before)
        return found
    monkeypatch.setattr(waypoints, '_boxes', counted_boxes)
    assert simq_mod.shortest_paths(*on_device, *args, map_index=[m for m, _, _ in problems], simplify='exact') == got
    assert inside_boxes == [1] and len(copies) == 2, (inside_boxes, copies)
    # a serpentine whose dense path overflows the first buffer: one more search, one more simplification, one more copy
    grid = np.ones((30, 31), np.uint8)
    grid[1::2, :] = 0
    grid[1::4, -1] = 1
    grid[3::4, 0] = 1
    del copies[:]
    lib.call('simq_launch_counts_reset')
    ways = simq_mod.grid_waypoints([grid], [(0, 0)], [(28, 0)])
    assert len(copies) == 2 and lib.c.simq_launch_count(b'grid_waypoints') == 2 and lib.c.simq_launch_count(b'grid_simplify') == 2
    dense = oracle.dense_path(oracle.spfa(grid, (0, 0))[1], (0, 0), (28, 0))
    assert ways.status[0] == 0 and np.array_equal(ways.waypoints[0], so.waypoints(grid, dense)) and len(ways.waypoints[0]) > 20
    assert ways.endpoints[0].tolist() == [0, 0, 28, 0]
    # more waypoints than the first read-back holds: the same second round
    comb = np.ones((6, 4 * waypoints.WAY_CAPACITY + 8), np.uint8)
    comb[:, 2::4] = 0
    comb[5, 2::8] = 1
    comb[0, 6::8] = 1                                                             # walls with their gaps at alternate ends
    s, t = (3, 0), (3, comb.shape[1] - 1)
    dense = oracle.dense_path(oracle.spfa(comb, s)[1], s, t)
    want = so.waypoints(comb, dense)
    assert len(want) > waypoints.WAY_CAPACITY and len(dense) <= 2 * sum(comb.shape) + 8     # the dense path fits, the waypoints do not
    del copies[:]
    ways = simq_mod.grid_waypoints([comb], [s], [t])
    assert len(copies) == 2 and np.array_equal(ways.waypoints[0], want)
