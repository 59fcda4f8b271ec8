"""CPU: the waypoint oracle against the reference's own parents, dense paths and waypoints (tests/golden/grid_waypoints_*.npz, written
by tools/gen_grid_waypoints_golden.py from shortest_paths.pyx), the host half of simq.WaypointGraph and simq.shortest_paths, the C-ABI
entry simq_grid_paths and its refusals (no kernel is launched here), and guards on the random grids the GPU test uses."""
import ctypes
import functools
import os

import numpy as np
import pytest

import grid_waypoints_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('rooms', 'clutter', 'edges')


def split(flat, lengths):
    out, o = [], 0
    for n in lengths:
        out.append(np.asarray(flat[o:o + n], np.int32).reshape(-1, 2))
        o += n
    return out


def parents_from_codes(codes):
    rows, cols = codes.shape
    parents = np.full((rows, cols), -1, np.int32)
    for k, (di, dj) in enumerate(oracle.DIRS):
        ii, jj = np.nonzero(codes == k)
        parents[ii, jj] = (ii - di) * cols + (jj - dj)
    return parents


def waypoint_cases(golden_dir):
    """(key, grid, source, reference distances, reference parents, targets, dense paths, {simplifier: waypoints})."""
    for kind in KINDS:
        g = np.load(os.path.join(golden_dir, 'grid_paths_%s.npz' % kind))
        z = np.load(os.path.join(golden_dir, 'grid_waypoints_%s.npz' % kind))
        for key in z['names']:
            key = str(key)
            name, si = key.rsplit('_', 1)
            ways = {label: split(z['way_%s_%s' % (label, key)], z['way_%s_len_%s' % (label, key)]) for label in ('identity', 'every_third')}
            yield (key, g['grid_' + name], tuple(int(x) for x in g['src_' + name][int(si)]), g['dist_' + name][int(si)],
                   parents_from_codes(z['parents_' + key]), [tuple(int(x) for x in t) for t in z['targets_' + key]],
                   split(z['dense_' + key], z['dense_len_' + key]), ways)


@functools.lru_cache(maxsize=None)
def oracle_search(key, golden_dir):
    for k, grid, source, *_ in waypoint_cases(golden_dir):
        if k == key:
            return oracle.spfa(grid, source)
    raise KeyError(key)


def test_oracle_equals_the_reference_bit_for_bit(golden_dir):
    n = 0
    for key, grid, source, dist, parents, targets, dense, _ in waypoint_cases(golden_dir):
        o_dist, o_parents, _ = oracle_search(key, golden_dir)
        assert np.array_equal(o_parents, parents), key
        assert np.array_equal(o_dist.view(np.int32), dist.view(np.int32)), key
        assert len(targets) == len(dense) >= 1
        for t, want in zip(targets, dense):
            assert np.array_equal(oracle.dense_path(o_parents, source, t), want), (key, t)
        n += 1
    assert n >= 25


def test_waypoint_graph_host_half_equals_the_reference(golden_dir, L):
    """WaypointGraph.shortest_path with its parents from the oracle (WaypointGraph.search): walk, pruning and reversal against the
    reference's final output under both stand-in simplifiers."""
    import simq
    n = 0
    for key, grid, source, dist, parents, targets, dense, ways in waypoint_cases(golden_dir):
        graph = simq.WaypointGraph(grid)
        graph.search = lambda g, s, key=key: oracle_search(key, golden_dir)[:2]
        for label, simplify in (('identity', oracle.identity), ('every_third', oracle.every_third)):
            for t, want_dense, want in zip(targets, dense, ways[label]):
                assert np.array_equal(graph.dense_path(source, t), want_dense), (key, t)
                got = graph.shortest_path(source, t, simplify=simplify)
                assert np.array_equal(np.asarray(got, np.int32).reshape(-1, 2), want), (key, t, label)
                n += 1
        assert graph.shortest_path_image(source) is graph.cache[source]          # the search's own distance image, no launch
        assert np.array_equal(graph.cache[source].view(np.int32), dist.view(np.int32))
    assert n >= 1000


def test_default_simplifier_is_skimage_or_a_clear_error(L):
    import simq
    graph = simq.WaypointGraph(np.ones((4, 5), np.uint8))
    graph.search = lambda g, s: oracle.spfa(g, s)[:2]
    try:
        import skimage.measure  # noqa: F401
    except ImportError:
        with pytest.raises(L.SimqError, match='scikit-image'):
            graph.shortest_path((0, 0), (3, 4))
    else:
        assert graph.shortest_path((0, 0), (3, 4))[0] == (0, 0)
    with pytest.raises(NotImplementedError, match='order'):
        simq.GridGraph(np.ones((4, 5), np.uint8)).shortest_path((0, 0), (3, 4))


@pytest.mark.parametrize('room', ['184x232', '232x232'])
def test_shortest_paths_host_half_equals_the_oracle(golden_dir, L, monkeypatch, room):
    """simq.shortest_paths with the device stage replaced by the oracle: pixel conversion, the straight verdict, the len < 2 rule and the
    end points."""
    from simq import waypoints
    cspace, thin, closest, problems = oracle.occupancy_problems(golden_dir, room)
    cache = {}

    def fake(grids, sources, targets, grid_index=None, thin=None, closest=None, **_):
        paths, status, ends = [], [], []
        for k, s, t in zip(grid_index, sources, targets):
            if oracle.is_straight(thin[k], s, t):
                paths.append(np.zeros((0, 2), np.int32)), status.append(1), ends.append(s + t)
                continue
            s2, t2 = tuple(int(closest[k][h][s]) for h in (0, 1)), tuple(int(closest[k][h][t]) for h in (0, 1))
            if (k, s2) not in cache:
                cache[(k, s2)] = oracle.spfa(grids[k], s2)[1]
            paths.append(oracle.dense_path(cache[(k, s2)], s2, t2)), status.append(0), ends.append(s2 + t2)
        return waypoints.DensePaths(paths, np.asarray(status, np.int32), np.asarray(ends, np.int32), None, None)

    monkeypatch.setattr(waypoints, 'grid_dense_paths', fake)
    got = waypoints.shortest_paths(cspace, thin, closest, [a for _, a, _ in problems], [b for _, _, b in problems],
                                   map_index=[m for m, _, _ in problems], simplify=oracle.identity)
    straight = 0
    for (m, a, b), path in zip(problems, got):
        want = oracle.occupancy_shortest_path(cspace[m], thin[m], closest[m], a, b, oracle.identity)
        assert path == want, (m, a, b)
        assert path[0] is a and path[-1] is b
        straight += len(want) == 2
    assert straight >= len(problems) // 4 and len(problems) - straight >= len(problems) // 4, straight


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_export_is_declared_bound_and_laid_out(L):
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    assert 'int simq_grid_paths(' in text and 'simq_grid_paths' in L.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), 'simq_grid_paths')
    from simq.waypoints import MAX_BOX_CELLS, GridPathProblem
    assert ctypes.sizeof(GridPathProblem) == 96
    assert GridPathProblem.path_capacity.offset == 48 and GridPathProblem.box_cols.offset == 88
    assert '#define SIMQ_GRID_PATH_MAX_BOX_CELLS %d' % MAX_BOX_CELLS in text and MAX_BOX_CELLS >= 16384
    assert 8 * MAX_BOX_CELLS + 16 <= 160 * 1024                                   # 8 bytes of LDS per cell


def test_c_abi_rejects_bad_descriptors_before_any_device_call(L):
    """Every check of simq_grid_paths runs on the host before the descriptor copy / launch (the fake device pointers below are never
    dereferenced)."""
    from simq.waypoints import GridPathProblem
    c = L.lib.c
    base = 1 << 32
    bufs = dict(grids=base, closest=base + (1 << 24), probs=base + (2 << 24), paths=base + (3 << 24), lengths=base + (4 << 24),
                ends=base + (5 << 24), parents=base + (6 << 24), dist=base + (7 << 24), status=base + (8 << 24))

    def call(descs, n=None, grids_bytes=1 << 20, closest_ints=1 << 20, path_pairs=1 << 16, parents_ints=1 << 20, dist_floats=1 << 20, **ptrs):
        a = {k: ctypes.c_void_p(v) if v else None for k, v in dict(bufs, **ptrs).items()}
        arr = (GridPathProblem * len(descs))(*descs)
        return c.simq_grid_paths(a['grids'], grids_bytes, a['closest'], closest_ints, arr, len(descs) if n is None else n, a['probs'],
                                 a['paths'], path_pairs, a['lengths'], a['ends'], a['parents'], parents_ints, a['dist'], dist_floats,
                                 a['status'], None)

    def prob(**kw):
        f = dict(grid_offset=0, thin_offset=-1, closest_offset=-1, path_offset=0, parents_offset=-1, dist_offset=-1, path_capacity=16,
                 rows=10, cols=12, src_i=3, src_j=4, tgt_i=5, tgt_j=6, box_i0=1, box_j0=1, box_rows=8, box_cols=10, reserved_=0)
        f.update(kw)
        return GridPathProblem(*[f[n] for n, _ in GridPathProblem._fields_])

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1, word
        assert word in L.last_error(), (word, L.last_error())

    refused('NULL', [prob()], paths=0)
    refused('n = 0', [prob()], n=0)
    refused('source (10, 4) outside', [prob(src_i=10)])
    refused('target (5, -1) outside', [prob(tgt_j=-1)])
    refused('2^22', [prob(rows=2048, cols=2048)])
    refused('grid_offset', [prob()], grids_bytes=119)
    refused('grid_offset', [prob(grid_offset=-1)])
    refused('thin_offset', [prob(thin_offset=200)], grids_bytes=300)
    refused('closest_offset', [prob(closest_offset=1)], closest_ints=240)
    refused('closest_offset', [prob(closest_offset=0)], closest=0)
    refused('path_capacity', [prob(path_capacity=0)])
    refused('path_offset', [prob(path_offset=1)], path_pairs=16)
    refused('parents_offset', [prob(parents_offset=1)], parents_ints=120)
    refused('dist_offset', [prob(dist_offset=0)], dist_floats=119)
    refused('box', [prob(box_i0=3, box_rows=8)])
    refused('box', [prob(box_cols=-1)])
    refused('SIMQ_GRID_PATH_MAX_BOX_CELLS', [prob(rows=200, cols=200, box_i0=0, box_j0=0, box_rows=140, box_cols=140)])
    refused('overlap in d_paths', [prob(), prob(path_offset=15)])
    refused('overlap in d_parents', [prob(parents_offset=0), prob(path_offset=16, parents_offset=119)])
    refused('overlap in d_dist', [prob(dist_offset=0), prob(path_offset=16, dist_offset=100)])
    refused('d_paths and d_dist overlap', [prob(dist_offset=0)], dist=bufs['paths'] + 64)
    refused('d_grids overlap', [prob()], status=bufs['grids'] + 16)
    refused('d_paths is not 4-byte aligned', [prob()], paths=bufs['paths'] + 2)
    refused('d_problems is not 8-byte aligned', [prob()], probs=bufs['probs'] + 4)


def test_without_a_gpu_the_dense_paths_raise(L, monkeypatch):
    import torch
    import simq
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.WaypointGraph(np.ones((4, 5), np.uint8)).dense_path((0, 0), (3, 4))
    with pytest.raises(ValueError):
        simq.grid_dense_paths([np.ones((4, 5), np.uint8)], [(0, 0)], [(1, 1), (2, 2)])


def test_random_grids_can_tell_a_wrong_emulation():
    """Caps on the input of the GPU test, not measurements.  The ring the kernel uses has one slot per vertex (free cell) plus one --
    the bound on the live queue -- so a grid wraps it when its pushes exceed its free cells + 1; no grid with 10 % of its cells
    blocked can push more often than its box has cells."""
    cases = oracle.random_grids()
    assert len(cases) == 60
    again = oracle.random_grids()
    assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(cases, again))
    total = dict(swaps=0, order_sensitive=0, queued_relaxations=0)
    wraps = 0
    for grid, source, _ in cases:
        assert 8 <= grid.shape[0] <= 60 and 8 <= grid.shape[1] <= 70
        count = oracle.spfa(grid, source)[2]
        for k in total:
            total[k] += count[k]
        wraps += count['pushes'] + 1 > int((grid != 0).sum()) + 1             # slots used (the source's included) > ring slots
    assert total['swaps'] >= 100 and total['order_sensitive'] >= 5 and total['queued_relaxations'] >= 1000, total
    assert wraps >= 10, wraps
