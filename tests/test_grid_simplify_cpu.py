"""CPU: the exact simplification rule (tests/grid_simplify_oracle.py) against a float64 restatement of the published
approximate_polygon, simq.approximate_polygon_exact against the rule, simplify='exact' through WaypointGraph and simq.shortest_paths
with the device stage replaced, and every host refusal of simq_grid_waypoints (no kernel is launched here)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import grid_simplify_oracle as so
import grid_waypoints_oracle as oracle
from test_grid_waypoints_cpu import oracle_search, waypoint_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def fixture_paths(golden_dir):
    """Every dense path of grid_waypoints_{rooms,clutter,edges}.npz with its grid: [(key, grid, dense)]."""
    return tuple((key, grid, d) for key, grid, _, _, _, _, dense, _ in waypoint_cases(golden_dir) for d in dense)


def test_rule_equals_the_float_algorithm_wherever_that_is_free_of_ties(golden_dir):
    """The rule equals the float64 algorithm with values within 1e-9 counted as equal on every fixture dense path of 3 or more points
    and on every random walk, at tolerance 1; the algorithm as published (eps = 0) differs on some of them, and only where the rule
    recorded a tie.  Both kinds of path exist: with a tie and without."""
    long_enough = [d for _, _, d in fixture_paths(golden_dir) if len(d) >= 3]
    assert len(long_enough) >= 800 and max(len(d) for d in long_enough) >= 1400
    for name, paths in (('fixtures', long_enough), ('walks', so.random_walks())):
        tied = raw_differs = 0
        for p, d in enumerate(paths):
            ties = dict(tolerance=0, argmax=0)
            got = so.simplify_exact(d, 1, ties)
            assert np.array_equal(got, so.approximate_polygon_float(d, 1, eps=1e-9)), (name, p)
            has_tie = ties['tolerance'] + ties['argmax'] > 0
            tied += has_tie
            if not np.array_equal(got, so.approximate_polygon_float(d, 1)):
                raw_differs += 1
                assert has_tie, (name, p)
        print('%s: %d paths, %d with a tie, %d on which the float algorithm as published differs' % (name, len(paths), tied, raw_differs))
        assert 0 < tied < len(paths), (name, tied)


def test_walks_are_what_the_tests_say():
    walks = so.random_walks()
    assert len(walks) == 2000 and {len(w) for w in walks} >= set(range(3, 121))
    assert all(np.abs(np.diff(w, axis=0)).max() == 1 for w in walks)
    assert all(w.min() >= 1 and w.max() < so.WALK_EXTENT - 1 for w in walks)
    assert sum(len(np.unique(w, axis=0)) < len(w) for w in walks) >= 500                    # walks that come back to a pixel
    ones, mixed = so.walk_grids()
    kept = [len(so.waypoints(mixed, w)) for w in walks[:200]]
    assert all(len(so.waypoints(ones, w)) == 2 for w in walks[:50]) and min(kept) == 2 and max(kept) > 4


def test_host_function_equals_the_rule(golden_dir):
    import simq
    n = 0
    for tolerance in (1, 2):
        for d in [d for _, _, d in fixture_paths(golden_dir)] + list(so.random_walks()):
            assert np.array_equal(simq.approximate_polygon_exact(d, tolerance), so.exact(d, tolerance)), (tolerance, n)
            n += 1
    special = [[(5, 5)], [(5, 5), (5, 6)], [(5, 5), (5, 5)], [(5, 5), (6, 6), (7, 5)], [(5, 5), (9, 9), (5, 5)], [(3, 3)] * 6,
               [(0, j) for j in range(40)], [(i, 7) for i in range(40, 0, -1)], [(i, i) for i in range(30)], [(i, 30 - i) for i in range(30)],
               [(0, j) for j in range(20)] + [(i, 19) for i in range(1, 20)],                # an L: the corner is kept
               [(0, 0), (1, 1), (0, 2), (1, 3), (0, 4)], [(0, 0), (2, 1), (0, 2)],           # distances of exactly 1 and below
               [(0, 0), (40000, 1), (0, 70000), (3, 3)]]                                     # beyond 2^15: Python integers
    for pts in special:
        for tolerance in (1, 2, 255):
            d = np.asarray(pts, np.int64)
            assert np.array_equal(simq.approximate_polygon_exact(d, tolerance), so.simplify_exact(d, tolerance)), (pts[:4], tolerance)
    assert len(simq.approximate_polygon_exact(np.asarray(special[10]), 1)) == 3
    assert len(simq.approximate_polygon_exact(np.asarray(special[11]), 1)) == 2             # 1 is not above the tolerance of 1
    for bad_tolerance in (0, 256, 1.5, True):
        with pytest.raises(ValueError, match='tolerance'):
            simq.approximate_polygon_exact(np.zeros((3, 2), np.int32), bad_tolerance)
    for bad in (np.zeros((3, 2), np.float64), np.zeros((0, 2), np.int32), np.zeros(4, np.int32)):
        with pytest.raises(ValueError, match='integer'):
            simq.approximate_polygon_exact(bad, 1)


def test_waypoint_graph_with_the_exact_simplifier(golden_dir, L):
    """WaypointGraph.shortest_path(simplify='exact') and (simplify=simq.approximate_polygon_exact), parents from the oracle's search,
    against the oracle's pruning behind the rule."""
    import simq
    n = 0
    for key, grid, source, _, _, targets, dense, _ in waypoint_cases(golden_dir):
        graph = simq.WaypointGraph(grid)
        graph.search = lambda g, s, key=key: oracle_search(key, golden_dir)[:2]
        for t, d in list(zip(targets, dense))[::3]:
            want = [tuple(int(x) for x in q) for q in oracle.prune(grid, d, so.exact)]
            assert graph.shortest_path(source, t, simplify='exact') == want, (key, t)
            assert graph.shortest_path(source, t, simplify=simq.approximate_polygon_exact) == want, (key, t)
            assert np.array_equal(np.asarray(want, np.int32).reshape(-1, 2), so.waypoints(grid, d)), (key, t)
            n += 1
    assert n >= 250
    with pytest.raises(ValueError, match="'exact'"):
        simq.WaypointGraph(np.ones((4, 5), np.uint8)).shortest_path((0, 0), (3, 4), simplify='douglas')


@pytest.mark.parametrize('room', ['184x232', '232x232'])
def test_shortest_paths_exact_with_the_device_stage_replaced(golden_dir, L, monkeypatch, room):
    """simq.shortest_paths(simplify='exact') with grid_waypoints -- search, simplification and pruning on the device -- replaced by
    the oracle: pixel conversion, the straight verdict, the len < 2 rule and the end points.  No dense path is asked for."""
    from simq import waypoints
    cspace, thin, closest, problems = oracle.occupancy_problems(golden_dir, room)
    cache = {}

    def fake(grids, sources, targets, grid_index=None, thin=None, closest=None, tolerance=1):
        ways, status, ends = [], [], []
        for k, s, t in zip(grid_index, sources, targets):
            if oracle.is_straight(thin[k], s, t):
                ways.append(np.zeros((0, 2), np.int32)), status.append(1), ends.append(s + t)
                continue
            s2, t2 = tuple(int(closest[k][h][s]) for h in (0, 1)), tuple(int(closest[k][h][t]) for h in (0, 1))
            if (k, s2) not in cache:
                cache[(k, s2)] = oracle.spfa(grids[k], s2)[1]
            ways.append(so.waypoints(grids[k], oracle.dense_path(cache[(k, s2)], s2, t2), tolerance))
            status.append(0), ends.append(s2 + t2)
        return waypoints.Waypoints(ways, np.asarray(status, np.int32), np.asarray(ends, np.int32))

    def no_dense_paths(*a, **k):
        raise AssertionError("simplify='exact' asked for dense paths")

    monkeypatch.setattr(waypoints, 'grid_waypoints', fake)
    monkeypatch.setattr(waypoints, 'grid_dense_paths', no_dense_paths)
    got = waypoints.shortest_paths(cspace, thin, closest, [a for _, a, _ in problems], [b for _, _, b in problems],
                                   map_index=[m for m, _, _ in problems], simplify='exact')
    straight = 0
    for (m, a, b), path in zip(problems, got):
        want = oracle.occupancy_shortest_path(cspace[m], thin[m], closest[m], a, b, so.exact)
        assert path == want, (m, a, b)
        assert path[0] is a and path[-1] is b
        straight += len(want) == 2
    assert straight >= len(problems) // 4 and len(problems) - straight >= len(problems) // 4, straight


def test_simplify_names(L, monkeypatch):
    """An unknown name is a ValueError before anything is queued; None is still scikit-image or the error that names it."""
    import simq
    from simq import waypoints

    def nothing_queued(*a, **k):
        raise AssertionError('a device stage ran')
    monkeypatch.setattr(waypoints, 'grid_waypoints', nothing_queued)
    monkeypatch.setattr(waypoints, 'grid_dense_paths', nothing_queued)
    one = np.ones((1, 8, 8), np.uint8)
    with pytest.raises(ValueError, match="'exact'"):
        simq.shortest_paths(one, one, np.zeros((1, 2, 8, 8), np.int32), [(0.0, 0.0)], [(0.01, 0.01)], simplify='Exact')
    try:
        import skimage.measure  # noqa: F401
    except ImportError:
        with pytest.raises(L.SimqError, match='scikit-image') as e:
            waypoints._simplifier(None)
        assert "simplify='exact'" in str(e.value)
    assert waypoints._simplifier('exact') is simq.approximate_polygon_exact and waypoints._simplifier(oracle.identity) is oracle.identity


def test_export_is_declared_bound_and_laid_out(L):
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    assert 'int simq_grid_waypoints(' in text and 'simq_grid_waypoints' in L.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), 'simq_grid_waypoints')
    from simq.waypoints import MAX_BOX_CELLS, GridWaypointProblem
    assert ctypes.sizeof(GridWaypointProblem) == 40 and GridWaypointProblem.rows.offset == 24 and GridWaypointProblem.tolerance.offset == 36
    cap = int(text.split('#define SIMQ_GRID_WAYPOINTS_MAX_PATH')[1].split()[0])
    assert cap > MAX_BOX_CELLS and cap % 32 == 0                                   # every path simq_grid_paths can write has its flag


def test_c_abi_rejects_bad_descriptors_before_any_device_call(L):
    """Every check of simq_grid_waypoints runs on the host before the descriptor copy / launch (the fake device pointers below are
    never dereferenced)."""
    from simq.waypoints import GridWaypointProblem
    c = L.lib.c
    base = 1 << 32
    bufs = dict(grids=base, paths=base + (1 << 24), lengths=base + (2 << 24), pstatus=base + (3 << 24), probs=base + (4 << 24),
                ways=base + (5 << 24), counts=base + (6 << 24), status=base + (7 << 24))

    def call(descs, n=None, grids_bytes=1 << 20, path_pairs=1 << 16, way_pairs=1 << 16, **ptrs):
        a = {k: ctypes.c_void_p(v) if v else None for k, v in dict(bufs, **ptrs).items()}
        arr = (GridWaypointProblem * len(descs))(*descs)
        return c.simq_grid_waypoints(a['grids'], grids_bytes, a['paths'], path_pairs, a['lengths'], a['pstatus'], arr,
                                     len(descs) if n is None else n, a['probs'], a['ways'], way_pairs, a['counts'], a['status'], None)

    def prob(**kw):
        f = dict(grid_offset=0, path_offset=0, way_offset=0, rows=10, cols=12, way_capacity=16, tolerance=1)
        f.update(kw)
        return GridWaypointProblem(*[f[n] for n, _ in GridWaypointProblem._fields_])

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1, word
        assert word in L.last_error(), (word, L.last_error())

    for name in bufs:
        refused('NULL', [prob()], **{name: 0})
    refused('n = 0', [prob()], n=0)
    refused('extents', [prob()], way_pairs=0)
    refused('extents', [prob()], path_pairs=0)
    refused('2^22', [prob(rows=2048, cols=2048)])
    refused('2^15', [prob(rows=1, cols=32769)])
    refused('2^15', [prob(rows=0)])
    refused('tolerance = 0', [prob(tolerance=0)])
    refused('tolerance = 256', [prob(tolerance=256)])
    refused('grid_offset', [prob()], grids_bytes=119)
    refused('grid_offset', [prob(grid_offset=-1)])
    refused('path_offset', [prob(path_offset=16)], path_pairs=16)
    refused('path_offset', [prob(path_offset=-1)])
    refused('way_capacity', [prob(way_capacity=0)])
    refused('way_offset', [prob(way_offset=1)], way_pairs=16)
    refused('way_offset', [prob(way_offset=-1)])
    refused('overlap in d_ways', [prob(), prob(way_offset=15)])
    refused('d_paths and d_ways overlap', [prob()], ways=bufs['paths'] + 64)
    refused('d_grids and d_status overlap', [prob()], status=bufs['grids'] + 16)
    refused('d_lengths and d_counts overlap', [prob()], counts=bufs['lengths'])
    refused('d_path_status and d_status overlap', [prob()], status=bufs['pstatus'])
    refused('d_problems and d_ways overlap', [prob()], probs=bufs['ways'] + 8)
    refused('d_paths is not 8-byte aligned', [prob()], paths=bufs['paths'] + 4)
    refused('d_ways is not 8-byte aligned', [prob()], ways=bufs['ways'] + 4)
    refused('d_problems is not 8-byte aligned', [prob()], probs=bufs['probs'] + 4)
    refused('d_counts is not 4-byte aligned', [prob()], counts=bufs['counts'] + 2)
    # the largest legal sides pass every host check of the descriptor: what refuses this call is the next rule
    refused('d_status is not 4-byte aligned', [prob(rows=32768, cols=127, tolerance=255)], status=bufs['status'] + 1, grids_bytes=1 << 23)


def test_without_a_gpu_the_device_form_raises_and_the_host_form_works(L, monkeypatch):
    import torch
    import simq
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.grid_waypoints([np.ones((4, 5), np.uint8)], [(0, 0)], [(3, 4)])
    with pytest.raises(ValueError, match='tolerance'):
        simq.grid_waypoints([np.ones((4, 5), np.uint8)], [(0, 0)], [(3, 4)], tolerance=0)
    graph = simq.WaypointGraph(np.ones((4, 5), np.uint8))
    graph.search = lambda g, s: oracle.spfa(g, s)[:2]
    assert graph.shortest_path((0, 0), (3, 4), simplify='exact') == [(0, 0), (3, 4)]
