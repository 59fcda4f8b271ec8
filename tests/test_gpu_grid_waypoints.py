"""GPU: simq_grid_paths (csrc/grid_waypoints.hip) against the reference's own parents and dense paths (tests/golden/grid_waypoints_*.npz)
and against the numpy restatement of its search (tests/grid_waypoints_oracle.py), bit for bit; the distance output against
simq.grid_distance_images; the chain from simq.occupancy_maps; capacity, cap and caching."""
import ctypes
import os

import numpy as np
import pytest
import torch

import grid_waypoints_oracle as oracle
from test_grid_waypoints_cpu import oracle_search, waypoint_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    import simq.waypoints  # noqa: F401
    return simq


def fits(grid):
    from simq.waypoints import MAX_BOX_CELLS
    box = oracle.free_box(grid)
    return (box[2] + 2) * (box[3] + 2) <= MAX_BOX_CELLS


def test_fixtures_through_grid_dense_paths(simq_mod, golden_dir):
    """Every fixture whose free box fits the LDS cap, all of its targets in one launch per (grid, source); the others are refused."""
    n = refused = 0
    for key, grid, source, dist, parents, targets, dense, _ in waypoint_cases(golden_dir):
        if not fits(grid):
            with pytest.raises(simq_mod.waypoints.SimqError, match='SIMQ_GRID_PATH_MAX_BOX_CELLS'):
                simq_mod.grid_dense_paths([grid], [source], [source])
            refused += 1
            continue
        got = simq_mod.grid_dense_paths([grid], [source] * len(targets), targets, grid_index=[0] * len(targets), parents=True,
                                        distances=True)
        assert (got.status == 0).all(), key
        assert np.array_equal(got.parents[0].cpu().numpy(), parents), key
        assert np.array_equal(got.distances[0].cpu().numpy().view(np.int32), dist.view(np.int32)), key
        for t, want, path in zip(targets, dense, got.paths):
            assert np.array_equal(path, want), (key, t)
        n += 1
    assert n >= 20 and refused >= 2


def test_fixtures_through_the_raw_c_abi(simq_mod, golden_dir):
    from simq._lib import lib, ptr, stream_ptr
    from simq.waypoints import GridPathProblem
    dev = torch.device('cuda', torch.cuda.current_device())
    for want_key in ('clutter_large_0', 'values_7_255_0', 'row_300_1'):
        key, grid, source, dist, parents, targets, dense, _ = next(c for c in waypoint_cases(golden_dir) if c[0] == want_key)
        rows, cols = grid.shape
        P, cap = len(targets), 1024
        d_grid = torch.from_numpy(grid).to(dev)
        probs = (GridPathProblem * P)(*[GridPathProblem(0, -1, -1, p * cap, p * rows * cols if p == 0 else -1, -1, cap, rows, cols,
                                                        source[0], source[1], t[0], t[1], *oracle.free_box(grid), 0)
                                        for p, t in enumerate(targets)])
        d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
        paths = torch.full((P * cap, 2), -7, dtype=torch.int32, device=dev)
        lengths, status = torch.full((P,), -7, dtype=torch.int32, device=dev), torch.full((P,), -7, dtype=torch.int32, device=dev)
        ends = torch.full((P, 4), -7, dtype=torch.int32, device=dev)
        par = torch.full((rows, cols), -7, dtype=torch.int32, device=dev)
        lib.call('simq_grid_paths', ptr(d_grid), ctypes.c_int64(grid.size), None, ctypes.c_int64(0), probs, P, ptr(d_probs), ptr(paths),
                 ctypes.c_int64(P * cap), ptr(lengths), ptr(ends), ptr(par), ctypes.c_int64(par.numel()), None, ctypes.c_int64(0),
                 ptr(status), stream_ptr(dev))
        assert (status.cpu().numpy() == 0).all(), key
        assert np.array_equal(par.cpu().numpy(), parents), key
        host, ln = paths.cpu().numpy().reshape(P, cap, 2), lengths.cpu().numpy()
        for p, (t, want) in enumerate(zip(targets, dense)):
            assert ln[p] == len(want) and np.array_equal(host[p, :ln[p]], want), (key, t)
            assert (host[p, ln[p]:] == -7).all()
            assert ends.cpu().numpy()[p].tolist() == list(source) + list(t)


def test_random_grids_in_one_mixed_launch(simq_mod):
    cases = oracle.random_grids()
    grids, sources, targets = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    got = simq_mod.grid_dense_paths(grids, sources, targets, parents=True, distances=True)
    dist = simq_mod.grid_distance_images(grids, sources)
    for p, (grid, s, t) in enumerate(cases):
        o_dist, o_parents, _ = oracle.spfa(grid, s)
        assert np.array_equal(got.parents[p].cpu().numpy(), o_parents), p
        assert np.array_equal(got.paths[p], oracle.dense_path(o_parents, s, t)), p
        assert np.array_equal(got.distances[p].cpu().numpy().view(np.int32), dist[p].cpu().numpy().view(np.int32)), p
        assert np.array_equal(got.distances[p].cpu().numpy().view(np.int32), o_dist.view(np.int32)), p


def test_degenerate_shapes(simq_mod):
    one, blocked = np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8)
    row, col = np.ones((1, 37), np.uint8), np.ones((41, 1), np.uint8)
    row[0, 20] = 0
    full = np.ones((9, 11), np.uint8)                                   # the free box touches the border on every side
    full[4, 2:9] = 0
    pocket = np.zeros((12, 14), np.uint8)
    pocket[1:5, 1:13] = 1
    pocket[7:11, 3:9] = 1                                               # two free regions that do not meet
    problems = [(one, (0, 0), (0, 0)), (blocked, (0, 0), (0, 0)), (row, (0, 3), (0, 19)), (row, (0, 3), (0, 30)), (col, (40, 0), (0, 0)),
                (full, (0, 0), (8, 10)), (full, (8, 10), (0, 0)), (full, (0, 5), (8, 5)), (full, (4, 0), (4, 10)),
                (full, (4, 3), (8, 8)),                                 # a blocked source
                (full, (0, 0), (4, 5)),                                 # a blocked target
                (pocket, (2, 2), (8, 5)),                               # an unreachable target
                (pocket, (8, 5), (8, 5)),                               # target == source
                (pocket, (0, 0), (2, 2)),                               # a blocked source outside the free box
                (pocket, (1, 1), (11, 13))]                             # a target outside the free box
    grids = [p[0] for p in problems]
    got = simq_mod.grid_dense_paths(grids, [p[1] for p in problems], [p[2] for p in problems], parents=True, distances=True)
    dist = simq_mod.grid_distance_images(grids, [p[1] for p in problems])
    for p, (grid, s, t) in enumerate(problems):
        o_dist, o_parents, _ = oracle.spfa(grid, s)
        assert np.array_equal(got.parents[p].cpu().numpy(), o_parents), p
        assert np.array_equal(got.paths[p], oracle.dense_path(o_parents, s, t)), p
        assert np.array_equal(got.distances[p].cpu().numpy().view(np.int32), o_dist.view(np.int32)), p
        assert np.array_equal(got.distances[p].cpu().numpy().view(np.int32), dist[p].cpu().numpy().view(np.int32)), p
    for p in (1, 9, 10, 11, 12, 13, 14):
        assert len(got.paths[p]) == 1 and tuple(got.paths[p][0]) == problems[p][2]


def test_capacity_and_cap(simq_mod):
    from simq._lib import last_error, lib, ptr, stream_ptr
    from simq.waypoints import MAX_BOX_CELLS, GridPathProblem
    dev = torch.device('cuda', torch.cuda.current_device())
    grid = np.ones((20, 30), np.uint8)
    grid[3:17, 15] = 0
    s, t = (10, 2), (10, 28)
    want = oracle.dense_path(oracle.spfa(grid, s)[1], s, t)
    d_grid = torch.from_numpy(grid).to(dev)

    def run(cap, box):
        probs = (GridPathProblem * 1)(GridPathProblem(0, -1, -1, 0, 0, 0, cap, 20, 30, s[0], s[1], t[0], t[1], *box, 0))
        d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
        out = [torch.full(shape, -7, dtype=dt, device=dev) for shape, dt in (((len(want) + 8, 2), torch.int32), ((1,), torch.int32),
                                                                             ((4,), torch.int32), ((600,), torch.int32),
                                                                             ((600,), torch.float32), ((1,), torch.int32))]
        rc = lib.c.simq_grid_paths(ptr(d_grid), grid.size, None, 0, probs, 1, ptr(d_probs), ptr(out[0]), len(want) + 8, ptr(out[1]), ptr(out[2]),
                                   ptr(out[3]), 600, ptr(out[4]), 600, ptr(out[5]), stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, [o.cpu().numpy() for o in out]

    rc, (paths, length, _, par, dist, status) = run(len(want) - 1, (0, 0, 20, 30))
    assert rc == 0 and status[0] == 3 and length[0] == len(want)
    assert np.array_equal(paths[:len(want) - 1], want[:-1]) and (paths[len(want) - 1:] == -7).all()
    assert np.array_equal(par.reshape(20, 30), oracle.spfa(grid, s)[1])
    # the Python layer fetches the longer path with one more launch
    long_grid = np.ones((30, 31), np.uint8)
    long_grid[1::2, :] = 0
    long_grid[1::4, -1] = 1
    long_grid[3::4, 0] = 1                                              # a serpentine: the path is far longer than the first buffer
    lib.call('simq_launch_counts_reset')
    got = simq_mod.grid_dense_paths([long_grid], [(0, 0)], [(28, 0)])
    assert lib.c.simq_launch_count(b'grid_waypoints') == 2 and got.status[0] == 0
    assert np.array_equal(got.paths[0], oracle.dense_path(oracle.spfa(long_grid, (0, 0))[1], (0, 0), (28, 0)))
    # a declared box that misses a free cell: status 2, nothing else written
    rc, outs = run(len(want), (0, 0, 20, 29))
    assert rc == 0 and outs[5][0] == 2 and all((o == -7).all() for o in outs[:5])
    # a box over the cap: refused on the host, nothing launched or written
    big = torch.ones((150, 150), dtype=torch.uint8, device=dev)
    assert 152 * 152 > MAX_BOX_CELLS
    lib.call('simq_launch_counts_reset')
    with pytest.raises(simq_mod.waypoints.SimqError, match='SIMQ_GRID_PATH_MAX_BOX_CELLS'):
        simq_mod.grid_dense_paths([big], [(0, 0)], [(5, 5)])
    assert lib.c.simq_launch_count(b'grid_waypoints') == 0 and 'SIMQ_GRID_PATH_MAX_BOX_CELLS' in last_error()


def test_large_batch_over_both_rooms(simq_mod, golden_dir):
    cases = {c[0]: c for c in waypoint_cases(golden_dir) if c[0] in ('clutter_small_0', 'clutter_large_0')}
    grids = [cases['clutter_small_0'][1], cases['clutter_large_0'][1]]
    rng = np.random.RandomState(3)
    free = [np.argwhere(g != 0) for g in grids]
    index = [p % 2 for p in range(1024)]
    sources = [tuple(int(x) for x in free[k][rng.randint(len(free[k]))]) for k in index]
    targets = [tuple(int(x) for x in free[k][rng.randint(len(free[k]))]) for k in index]
    got = simq_mod.grid_dense_paths(grids, sources, targets, grid_index=index, parents=True)
    assert (got.status == 0).all()
    for p in range(0, 1024, 16):
        o_parents = oracle.spfa(grids[index[p]], sources[p])[1]
        assert np.array_equal(got.parents[p].cpu().numpy(), o_parents), p
        assert np.array_equal(got.paths[p], oracle.dense_path(o_parents, sources[p], targets[p])), p


@pytest.mark.parametrize('room', ['184x232', '232x232'])
def test_chain_from_occupancy_maps(simq_mod, golden_dir, room, monkeypatch):
    """simq.occupancy_maps feeds simq.shortest_paths on the device; the result equals the oracle's OccupancyMap.shortest_path on the
    fixture's reference maps.  No configuration space goes from the host to the device."""
    from simq import waypoints
    z = np.load(os.path.join(golden_dir, 'occupancy_maps_%s.npz' % room))
    cspace, thin, closest, problems = oracle.occupancy_problems(golden_dir, room)
    assert len(problems) >= 32
    maps = simq_mod.occupancy_maps(z['occupancy'], z['room_mask'], z['radius'].tolist(), z['thin_radius'].tolist())

    def no_upload(a):
        raise AssertionError('a host array of %s went to the device' % (a.shape,))
    monkeypatch.setattr(waypoints.torch, 'from_numpy', no_upload)
    got = simq_mod.shortest_paths(maps.configuration_space, maps.cspace_thin, maps.closest_cspace_indices, [a for _, a, _ in problems],
                                  [b for _, _, b in problems], map_index=[m for m, _, _ in problems], simplify=oracle.identity)
    monkeypatch.undo()
    straight, cache = 0, {}
    for (m, a, b), path in zip(problems, got):
        want = oracle.occupancy_shortest_path(cspace[m], thin[m], closest[m], a, b, oracle.identity, cache.setdefault(m, {}))
        assert path == want, (m, a, b)
        straight += len(want) == 2
    assert straight >= len(problems) // 4 and len(problems) - straight >= len(problems) // 4


def test_waypoint_graph_caches_per_source(simq_mod, golden_dir):
    from simq._lib import lib
    key, grid, source, dist, parents, targets, dense, ways = next(c for c in waypoint_cases(golden_dir) if c[0] == 'clutter_small_0')
    graph = simq_mod.WaypointGraph(grid)
    lib.call('simq_launch_counts_reset')
    assert np.array_equal(graph.dense_path(source, targets[1]), dense[1])
    assert lib.c.simq_launch_count(b'grid_waypoints') == 1
    for t, want_dense, want in zip(targets, dense, ways['every_third']):
        assert np.array_equal(graph.dense_path(source, t), want_dense)
        assert np.array_equal(np.asarray(graph.shortest_path(source, t, simplify=oracle.every_third), np.int32).reshape(-1, 2), want)
    assert np.array_equal(graph.shortest_path_image(source).view(np.int32), dist.view(np.int32))
    assert lib.c.simq_launch_count(b'grid_waypoints') == 1 and lib.c.simq_launch_count(b'grid_distance') == 0
