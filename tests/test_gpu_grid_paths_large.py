"""GPU: simq_grid_paths_large (csrc/grid_waypoints.hip: the search of simq_grid_paths with its state in a workspace in global memory)
and large_windows=True.  The fixtures simq_grid_paths refuses against the reference's own parents, paths and waypoints; both entry
points against each other byte for byte wherever both accept; windows just over the LDS cap and over 2^16 cells against the numpy
restatement of the search (tests/grid_waypoints_oracle.py); a path longer than simq_grid_waypoints takes; the front stages; one call
split between both entry points.  Everything is compared bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import grid_simplify_oracle as so
import grid_waypoints_oracle as oracle
import occupancy_maps_oracle
from test_grid_waypoints_cpu import oracle_search, waypoint_cases

pytestmark = pytest.mark.gpu

OVER_THE_CAP = ('open_232_0', 'open_232_1', 'wide_600_0', 'wide_600_1')
SENTINEL = -7


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    import simq.waypoints  # noqa: F401
    return simq


def window_cells(grid):
    box = oracle.free_box(grid)
    return (box[2] + 2) * (box[3] + 2)


@functools.lru_cache(maxsize=None)
def seeded(n):
    """(grid, source, oracle distances, oracle parents, counters): an n x n grid with 30 % of its cells blocked, searched from its last
    cell."""
    grid = (np.random.RandomState(1).rand(n, n) > 0.3).astype(np.uint8)
    source = (n - 1, n - 1)
    assert grid[source] == 1 and oracle.free_box(grid) == (0, 0, n, n)
    return (grid, source) + oracle.spfa(grid, source)


def reachable_near(dist, corner):
    """The reachable cell nearest to `corner` (the first in row-major order among equals)."""
    ii, jj = np.nonzero(dist >= 0)
    k = int(np.argmin((ii - corner[0]) ** 2 + (jj - corner[1]) ** 2))
    return int(ii[k]), int(jj[k])


def test_the_refused_fixtures(simq_mod, golden_dir):
    """The four (grid, source) fixtures whose windows are over the LDS cap (232 x 232 and 40 x 600): all targets of a case in one
    call.  Without large_windows=True every one of them is refused."""
    from simq.waypoints import MAX_BOX_CELLS
    cases = [c for c in waypoint_cases(golden_dir) if c[0] in OVER_THE_CAP]
    assert sorted(c[0] for c in cases) == sorted(OVER_THE_CAP)
    for key, grid, source, dist, parents, targets, dense, ways in cases:
        assert window_cells(grid) > MAX_BOX_CELLS, key
        got = simq_mod.grid_dense_paths([grid], [source] * len(targets), targets, grid_index=[0] * len(targets), parents=True,
                                        distances=True, large_windows=True)
        assert (got.status == 0).all(), key
        assert np.array_equal(got.parents[0].cpu().numpy(), parents), key
        for t, want, path in zip(targets, dense, got.paths):
            assert np.array_equal(path, want), (key, t)
        bits = got.distances[0].cpu().numpy().view(np.int32)
        assert np.array_equal(bits, dist.view(np.int32)), key
        assert np.array_equal(bits, simq_mod.grid_distance_images([grid], [source])[0].cpu().numpy().view(np.int32)), key
        graph = simq_mod.WaypointGraph(grid, large_windows=True)
        for t, want in zip(targets, ways['identity']):
            got_way = graph.shortest_path(source, t, simplify=oracle.identity)
            assert np.array_equal(np.asarray(got_way, np.int32).reshape(-1, 2), want), (key, t)


def degenerate_problems():
    """The fifteen problems of test_gpu_grid_waypoints.py::test_degenerate_shapes."""
    one, blocked = np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8)
    row, col = np.ones((1, 37), np.uint8), np.ones((41, 1), np.uint8)
    row[0, 20] = 0
    full = np.ones((9, 11), np.uint8)                                   # the free box touches the border on every side
    full[4, 2:9] = 0
    pocket = np.zeros((12, 14), np.uint8)
    pocket[1:5, 1:13] = 1
    pocket[7:11, 3:9] = 1                                               # two free regions that do not meet
    return [(one, (0, 0), (0, 0)), (blocked, (0, 0), (0, 0)), (row, (0, 3), (0, 19)), (row, (0, 3), (0, 30)), (col, (40, 0), (0, 0)),
            (full, (0, 0), (8, 10)), (full, (8, 10), (0, 0)), (full, (0, 5), (8, 5)), (full, (4, 0), (4, 10)),
            (full, (4, 3), (8, 8)),                                     # a blocked source
            (full, (0, 0), (4, 5)),                                     # a blocked target
            (pocket, (2, 2), (8, 5)),                                   # an unreachable target
            (pocket, (8, 5), (8, 5)),                                   # target == source
            (pocket, (0, 0), (2, 2)),                                   # a blocked source outside the free box
            (pocket, (1, 1), (11, 13))]                                 # a target outside the free box


def raw(entry, problems, capacities, boxes=None):
    """One call of `entry` ('simq_grid_paths' or 'simq_grid_paths_large') over (grid, source, target) problems through the C ABI, every
    output prefilled with SENTINEL: {name: host array}.  The large entry gets its workspaces end to end, filled with 0xA5."""
    from simq._lib import lib, ptr, stream_ptr
    from simq.waypoints import GridPathLargeProblem, GridPathProblem
    dev = torch.device('cuda', torch.cuda.current_device())
    P = len(problems)
    boxes = boxes or [oracle.free_box(g) for g, _, _ in problems]
    goff = np.concatenate([[0], np.cumsum([(g.size + 15) // 16 * 16 for g, _, _ in problems])]).tolist()
    ioff = np.concatenate([[0], np.cumsum([g.size for g, _, _ in problems])]).tolist()
    poff = np.concatenate([[0], np.cumsum(capacities)]).tolist()
    packed = np.zeros(goff[-1], np.uint8)
    for p, (g, _, _) in enumerate(problems):
        packed[goff[p]:goff[p] + g.size] = g.reshape(-1)
    d_grids = torch.from_numpy(packed).to(dev)
    large = entry == 'simq_grid_paths_large'
    need = [lib.c.simq_grid_paths_large_work_bytes(b[2], b[3]) for b in boxes]
    woff = np.concatenate([[0], np.cumsum(need)]).tolist()
    descs = []
    for p, (g, s, t) in enumerate(problems):
        offsets = [goff[p], -1, -1, poff[p], ioff[p], ioff[p]] + ([woff[p]] if large else [])
        descs.append((GridPathLargeProblem if large else GridPathProblem)(*offsets, capacities[p], g.shape[0], g.shape[1], s[0], s[1],
                                                                          t[0], t[1], *boxes[p], 0))
    probs = ((GridPathLargeProblem if large else GridPathProblem) * P)(*descs)
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    out = dict(paths=torch.full((poff[-1], 2), SENTINEL, dtype=torch.int32, device=dev),
               lengths=torch.full((P,), SENTINEL, dtype=torch.int32, device=dev),
               ends=torch.full((P, 4), SENTINEL, dtype=torch.int32, device=dev),
               parents=torch.full((ioff[-1],), SENTINEL, dtype=torch.int32, device=dev),
               dist=torch.full((ioff[-1],), float(SENTINEL), dtype=torch.float32, device=dev),
               status=torch.full((P,), SENTINEL, dtype=torch.int32, device=dev))
    extra = ()
    if large:
        work = torch.full((woff[-1],), 0xA5, dtype=torch.uint8, device=dev)
        extra = (ptr(work), ctypes.c_int64(woff[-1]))
    lib.call(entry, ptr(d_grids), ctypes.c_int64(packed.size), None, ctypes.c_int64(0), probs, P, ptr(d_probs), ptr(out['paths']),
             ctypes.c_int64(poff[-1]), ptr(out['lengths']), ptr(out['ends']), ptr(out['parents']), ctypes.c_int64(ioff[-1]),
             ptr(out['dist']), ctypes.c_int64(ioff[-1]), ptr(out['status']), *extra, stream_ptr(dev))
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host['dist'] = host['dist'].view(np.int32)
    host['path_starts'], host['image_starts'] = poff, ioff
    return host


def same_bytes(a, b):
    for k in ('paths', 'lengths', 'ends', 'parents', 'dist', 'status'):
        assert np.array_equal(a[k], b[k]), k


def test_both_entries_write_the_same_bytes(simq_mod):
    """The 60 random grids and the fifteen degenerate problems, each set through both entry points: every output byte equal, the
    sentinels past each path's length included; then against the oracle; a short path buffer; a window that misses a free cell."""
    for problems in (oracle.random_grids(), degenerate_problems()):
        capacities = [max(1, g.size) for g, _, _ in problems]
        lds, hbm = raw('simq_grid_paths', problems, capacities), raw('simq_grid_paths_large', problems, capacities)
        same_bytes(lds, hbm)
        assert (hbm['status'] == 0).all()
        for p, (grid, s, t) in enumerate(problems):
            o_dist, o_parents, _ = oracle.spfa(grid, s)
            want = oracle.dense_path(o_parents, s, t)
            a, i = hbm['path_starts'][p], hbm['image_starts'][p]
            assert hbm['lengths'][p] == len(want) and np.array_equal(hbm['paths'][a:a + len(want)], want), p
            assert (hbm['paths'][a + len(want):hbm['path_starts'][p + 1]] == SENTINEL).all(), p
            assert np.array_equal(hbm['parents'][i:i + grid.size].reshape(grid.shape), o_parents), p
            assert np.array_equal(hbm['dist'][i:i + grid.size].reshape(grid.shape), o_dist.view(np.int32)), p
            assert hbm['ends'][p].tolist() == list(s) + list(t), p
    # a path buffer one pair short wherever the path has more than one point: status 3 with the same need from both
    problems = oracle.random_grids()[:12]
    need = raw('simq_grid_paths_large', problems, [g.size for g, _, _ in problems])['lengths']
    capacities = [max(1, int(n) - 1) for n in need]
    lds, hbm = raw('simq_grid_paths', problems, capacities), raw('simq_grid_paths_large', problems, capacities)
    same_bytes(lds, hbm)
    assert np.array_equal(hbm['lengths'], need) and (need > 1).sum() >= 8
    assert np.array_equal(hbm['status'], np.where(need > 1, 3, 0))
    # a declared window that misses a free cell: status 2 from both, nothing else written
    boxes = [oracle.free_box(g) for g, _, _ in problems]
    boxes[3] = boxes[3][:3] + (boxes[3][3] - 1,)
    boxes[7] = (boxes[7][0] + 1, boxes[7][1], boxes[7][2] - 1, boxes[7][3])
    lds, hbm = raw('simq_grid_paths', problems, capacities, boxes), raw('simq_grid_paths_large', problems, capacities, boxes)
    same_bytes(lds, hbm)
    for p in (3, 7):
        a, b, i, g = hbm['path_starts'][p], hbm['path_starts'][p + 1], hbm['image_starts'][p], problems[p][0]
        assert hbm['status'][p] == 2 and hbm['lengths'][p] == SENTINEL and (hbm['ends'][p] == SENTINEL).all()
        assert (hbm['paths'][a:b] == SENTINEL).all() and (hbm['parents'][i:i + g.size] == SENTINEL).all()
        assert (hbm['dist'][i:i + g.size] == np.float32(SENTINEL).view(np.int32)).all()
    assert (np.delete(hbm['status'], [3, 7]) != 2).all()


def check_against_oracle(simq_mod, n, targets):
    grid, source, o_dist, o_parents, _ = seeded(n)
    got = simq_mod.grid_dense_paths([grid], [source] * len(targets), targets, grid_index=[0] * len(targets), parents=True,
                                    distances=True, large_windows=True)
    assert (got.status == 0).all()
    assert np.array_equal(got.parents[0].cpu().numpy(), o_parents)
    assert np.array_equal(got.distances[0].cpu().numpy().view(np.int32), o_dist.view(np.int32))
    for t, path in zip(targets, got.paths):
        assert np.array_equal(path, oracle.dense_path(o_parents, source, t)), t
    return got


def test_just_over_the_cap(simq_mod):
    """142 x 142 with 30 % blocked: 20 736 cells with the halo, 15 147 pushes for 14 115 free cells (the ring wraps), 431 exchanges
    with the front, 15 pushes whose exchange depends on the order of the relaxations inside a pop."""
    from simq.waypoints import MAX_BOX_CELLS
    grid, source, o_dist, _, count = seeded(142)
    assert MAX_BOX_CELLS < window_cells(grid) == 20736
    assert count['pushes'] > int(grid.sum()) and count['swaps'] > 0 and count['order_sensitive'] > 0, count
    ii, jj = np.nonzero(o_dist >= 0)
    pick = np.random.RandomState(2).choice(ii.size, 6, replace=False)
    targets = [(int(ii[k]), int(jj[k])) for k in pick] + [reachable_near(o_dist, (0, 0)), source]
    got = check_against_oracle(simq_mod, 142, targets)
    assert max(len(p) for p in got.paths) >= 142 and len(got.paths[-1]) == 1


def test_indices_past_16_bits(simq_mod):
    """258 x 258 built the same way: 67 600 cells with the halo, so window indices pass 2^16 and a 16-bit ring entry loses them
    (here: 50 516 pushes for 46 483 free cells)."""
    grid, source, o_dist, _, count = seeded(258)
    assert window_cells(grid) == 67600 > 1 << 16
    assert count['pushes'] > int(grid.sum()) and count['swaps'] > 0 and count['order_sensitive'] > 0, count
    targets = [reachable_near(o_dist, c) for c in ((0, 0), (0, 257), (257, 0), (257, 257))]
    assert len(set(targets)) == 4 and targets[0][0] * 260 + targets[0][1] < 1 << 16 < source[0] * 260 + source[1]
    check_against_oracle(simq_mod, 258, targets)


def test_a_path_longer_than_the_simplifier_takes(simq_mod):
    """A free row of 22 000 cells end to end: the dense path comes back whole; simq_grid_waypoints keeps its bound of
    SIMQ_GRID_WAYPOINTS_MAX_PATH = 20 480 points and the call raises its error; 20 000 cells give the two end points."""
    from simq.waypoints import MAX_BOX_CELLS
    row = np.ones((1, 22000), np.uint8)
    assert window_cells(row) == 66006 > MAX_BOX_CELLS
    got = simq_mod.grid_dense_paths([row], [(0, 21999)], [(0, 0)], large_windows=True)
    assert got.status[0] == 0
    assert np.array_equal(got.paths[0], np.stack([np.zeros(22000, np.int32), np.arange(22000, dtype=np.int32)], 1))
    with pytest.raises(simq_mod.waypoints.SimqError, match='simq_grid_waypoints'):
        simq_mod.grid_waypoints([row], [(0, 21999)], [(0, 0)], large_windows=True)
    ways = simq_mod.grid_waypoints([row[:, :20000]], [(0, 19999)], [(0, 0)], large_windows=True)
    assert ways.status[0] == 0 and ways.waypoints[0].tolist() == [[0, 19999], [0, 0]]


def test_front_stages_over_the_cap(simq_mod):
    """simq.occupancy_maps -> simq.shortest_paths(simplify='exact', large_windows=True) on a 160 x 160 map whose free cells span the
    whole map, against OccupancyMap.shortest_path with the exact rule as its simplifier, straight and traced problems both."""
    from simq.waypoints import MAX_BOX_CELLS
    rng = np.random.RandomState(6)
    occupancy = np.zeros((160, 160), np.uint8)
    for _ in range(14):
        i, j = rng.randint(8, 140, size=2)
        occupancy[i:i + rng.randint(3, 14), j:j + rng.randint(3, 14)] = 1
    mask = np.ones((160, 160), np.uint8)
    cspace, thin, closest = occupancy_maps_oracle.update(occupancy, mask, 6, 3)
    assert window_cells(cspace) > MAX_BOX_CELLS
    maps = simq_mod.occupancy_maps([occupancy], [mask], 6, 3)
    assert np.array_equal(maps.configuration_space[0].cpu().numpy(), cspace)
    rng = np.random.RandomState(61)
    half = 160 / 2 / oracle.PIXELS_PER_METER
    sources = [tuple(float(x) for x in rng.uniform(-half, half, size=2)) + (0.0,) for _ in range(16)]
    targets = [tuple(float(x) for x in rng.uniform(-half, half, size=2)) + (0.0,) for _ in range(16)]
    with pytest.raises(simq_mod.waypoints.SimqError, match='SIMQ_GRID_PATH_MAX_BOX_CELLS'):
        simq_mod.shortest_paths(maps.configuration_space, maps.cspace_thin, maps.closest_cspace_indices, sources, targets,
                                map_index=[0] * 16, simplify='exact')
    got = simq_mod.shortest_paths(maps.configuration_space, maps.cspace_thin, maps.closest_cspace_indices, sources, targets,
                                  map_index=[0] * 16, simplify='exact', large_windows=True)
    host = simq_mod.shortest_paths(maps.configuration_space, maps.cspace_thin, maps.closest_cspace_indices, sources, targets,
                                   map_index=[0] * 16, simplify=simq_mod.approximate_polygon_exact, large_windows=True)
    assert got == host
    straight, cache = 0, {}
    for a, b, path in zip(sources, targets, got):
        want = oracle.occupancy_shortest_path(cspace, thin, closest, a, b, so.exact, cache)
        assert path == want, (a, b)
        straight += len(want) == 2
    assert 4 <= straight <= 12, straight


def test_one_call_split_between_both_entries(simq_mod):
    """Problems over the cap interleaved with problems under it: one launch of each entry point, results in problem order; the same
    call without large_windows raises and launches nothing."""
    from simq._lib import lib
    small = oracle.random_grids()[:6]
    problems = []
    for k, (grid, s, t) in enumerate(small):
        problems.append((grid, s, t))
        n = (142, 258)[k % 2]
        big, source, o_dist, _, _ = seeded(n)
        problems.append((big, source, reachable_near(o_dist, ((0, 0), (0, n - 1), (n - 1, 0))[k % 3])))
    grids, sources, targets = [p[0] for p in problems], [p[1] for p in problems], [p[2] for p in problems]
    lib.call('simq_launch_counts_reset')
    with pytest.raises(simq_mod.waypoints.SimqError, match='SIMQ_GRID_PATH_MAX_BOX_CELLS'):
        simq_mod.grid_dense_paths(grids, sources, targets, parents=True, distances=True)
    assert lib.c.simq_launch_count(b'grid_waypoints') == 0 and lib.c.simq_launch_count(b'grid_paths_large') == 0
    got = simq_mod.grid_dense_paths(grids, sources, targets, parents=True, distances=True, large_windows=True)
    assert lib.c.simq_launch_count(b'grid_waypoints') == 1 and lib.c.simq_launch_count(b'grid_paths_large') == 1
    assert (got.status == 0).all()
    for p, (grid, s, t) in enumerate(problems):
        o_dist, o_parents = seeded(grid.shape[0])[2:4] if p % 2 else oracle.spfa(grid, s)[:2]
        assert got.endpoints[p].tolist() == list(s) + list(t), p
        assert np.array_equal(got.parents[p].cpu().numpy(), o_parents), p
        assert np.array_equal(got.distances[p].cpu().numpy().view(np.int32), o_dist.view(np.int32)), p
        assert np.array_equal(got.paths[p], oracle.dense_path(o_parents, s, t)), p
    # all under the cap, or all over it: the one entry point alone
    lib.call('simq_launch_counts_reset')
    simq_mod.grid_dense_paths(grids[::2], sources[::2], targets[::2], large_windows=True)
    assert lib.c.simq_launch_count(b'grid_waypoints') == 1 and lib.c.simq_launch_count(b'grid_paths_large') == 0
    simq_mod.grid_dense_paths(grids[1:4:2], sources[1:4:2], targets[1:4:2], large_windows=True)
    assert lib.c.simq_launch_count(b'grid_waypoints') == 1 and lib.c.simq_launch_count(b'grid_paths_large') == 1
