"""CPU: simq_grid_paths_large (csrc/grid_waypoints.hip), the search of simq_grid_paths with its state in a caller's workspace in global
memory -- the binding and the workspace size, every refusal of the entry point with fake device pointers (no kernel is launched
here), what it accepts that simq_grid_paths refuses, the host function that splits a call's problems between the two entry points,
and the large_windows keyword."""
import ctypes
import os

import numpy as np
import pytest

import grid_waypoints_oracle as oracle
from test_grid_waypoints_cpu import oracle_search, waypoint_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARENA = []


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_exports_are_declared_bound_and_laid_out(L):
    from simq.waypoints import GridPathLargeProblem, GridPathProblem, large_work_bytes
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, declared in (('simq_grid_paths_large', 'int simq_grid_paths_large('),
                           ('simq_grid_paths_large_work_bytes', 'int64_t simq_grid_paths_large_work_bytes(')):
        assert declared in text and name in L.EXPORTS and hasattr(raw, name), name
    assert ctypes.sizeof(GridPathLargeProblem) == ctypes.sizeof(GridPathProblem) + 8 == 104
    assert GridPathLargeProblem.work_offset.offset == 48 and GridPathLargeProblem.work_offset.size == 8
    assert [n for n, _ in GridPathLargeProblem._fields_ if n != 'work_offset'] == [n for n, _ in GridPathProblem._fields_]
    assert GridPathLargeProblem.path_capacity.offset == 56 and GridPathLargeProblem.box_cols.offset == 96
    fn = L.lib.c.simq_grid_paths_large_work_bytes
    for rows, cols in ((0, 0), (1, 1), (98, 198), (232, 232), (1, 32768), (2047, 2047)):
        cells, ring = (rows + 2) * (cols + 2), rows * cols + 1
        want = -(-(4 * cells + 4 * ring + cells + cells) // 16) * 16           # distances, ring, parents, flags
        assert fn(rows, cols) == large_work_bytes(rows, cols) == want, (rows, cols)
        assert want % 16 == 0 and 10 * rows * cols < want
    assert fn(232, 232) == 543840
    for rows in (0, 1, 7, 141, 232):                                              # monotone in both arguments
        for cols in (0, 1, 7, 141, 232):
            assert fn(rows + 1, cols) >= fn(rows, cols) <= fn(rows, cols + 1) and fn(rows, cols) % 16 == 0
    assert fn(-1, 4) == -1 and fn(4, -1) == -1 and fn(2048, 2048) == -1


def harness(L):
    """(call, prob, bufs) over fake device pointers, as test_grid_waypoints_cpu does for simq_grid_paths; every buffer 16 MiB apart.
    Where there is a device the pointers lie in one real allocation instead: a call that passes the checks launches, and what it
    then reads and writes is inside the extents it declared."""
    import torch
    from simq.waypoints import GridPathLargeProblem
    c = L.lib.c
    base = 1 << 32
    if torch.cuda.is_available():
        ARENA.append(torch.zeros((11 << 24) + 4096, dtype=torch.uint8, device='cuda'))
        base = (ARENA[-1].data_ptr() + (1 << 20) + 4095) // 4096 * 4096
    bufs = dict(grids=base, closest=base + (1 << 24), probs=base + (2 << 24), paths=base + (3 << 24), lengths=base + (4 << 24),
                ends=base + (5 << 24), parents=base + (6 << 24), dist=base + (7 << 24), status=base + (8 << 24), work=base + (9 << 24))

    def call(descs, n=None, grids_bytes=1 << 20, closest_ints=1 << 20, path_pairs=1 << 16, parents_ints=1 << 20, dist_floats=1 << 20,
             work_bytes=1 << 20, **ptrs):
        a = {k: ctypes.c_void_p(v) if v else None for k, v in dict(bufs, **ptrs).items()}
        arr = (GridPathLargeProblem * len(descs))(*descs)
        return c.simq_grid_paths_large(a['grids'], grids_bytes, a['closest'], closest_ints, arr, len(descs) if n is None else n, a['probs'],
                                       a['paths'], path_pairs, a['lengths'], a['ends'], a['parents'], parents_ints, a['dist'], dist_floats,
                                       a['status'], a['work'], work_bytes, None)

    def prob(**kw):
        f = dict(grid_offset=0, thin_offset=-1, closest_offset=-1, path_offset=0, parents_offset=-1, dist_offset=-1, work_offset=0,
                 path_capacity=16, rows=10, cols=12, src_i=3, src_j=4, tgt_i=5, tgt_j=6, box_i0=1, box_j0=1, box_rows=8, box_cols=10,
                 reserved_=0)
        f.update(kw)
        return GridPathLargeProblem(*[f[n] for n, _ in GridPathLargeProblem._fields_])

    return call, prob, bufs


def test_c_abi_rejects_bad_descriptors_before_any_device_call(L):
    """Every check of simq_grid_paths_large runs on the host before the descriptor copy / launch: the rules it shares with
    simq_grid_paths (all but the cap) and those of the workspace."""
    call, prob, bufs = harness(L)
    need = L.lib.c.simq_grid_paths_large_work_bytes(8, 10)
    assert need == 1056

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1, word
        err = L.last_error()
        assert err.startswith('grid_paths_large:') and word in err, (word, err)

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
    refused('overlap in d_paths', [prob(), prob(path_offset=15, work_offset=need)])
    refused('overlap in d_parents', [prob(parents_offset=0), prob(path_offset=16, parents_offset=119, work_offset=need)])
    refused('overlap in d_dist', [prob(dist_offset=0), prob(path_offset=16, dist_offset=100, work_offset=need)])
    refused('d_paths and d_dist overlap', [prob(dist_offset=0)], dist=bufs['paths'] + 64)
    refused('d_grids overlap', [prob()], status=bufs['grids'] + 16)
    refused('d_paths is not 4-byte aligned', [prob()], paths=bufs['paths'] + 2)
    refused('d_problems is not 8-byte aligned', [prob()], probs=bufs['probs'] + 4)
    # the workspace
    refused('NULL', [prob()], work=0)
    refused('d_work is not 16-byte aligned', [prob()], work=bufs['work'] + 8)
    refused('work_offset', [prob()], work_bytes=need - 1)
    refused('work_offset', [prob(work_offset=-16)])
    refused('work_offset', [prob(work_offset=8)])
    refused('work_offset', [prob(work_offset=(1 << 20) - need + 16)])
    refused('work_offset', [prob(work_offset=1 << 20)])
    refused('overlap in d_work', [prob(), prob(path_offset=16, work_offset=need - 16)])
    refused('overlap in d_work', [prob(work_offset=need - 16), prob(path_offset=16)])
    refused('d_paths and d_work overlap', [prob()], work=bufs['paths'] + 64)
    refused('d_status and d_work overlap', [prob()], work=bufs['status'])
    refused('d_status and d_work overlap', [prob()], status=bufs['work'] + need - 4, work_bytes=need)
    refused('d_work and d_grids overlap', [prob()], work=bufs['grids'] + 4096)
    refused('d_work and d_grids overlap', [prob()], work=bufs['grids'] - (1 << 20) + 16)


def test_c_abi_accepts_what_the_capped_entry_refuses(L):
    """A call passes every host check exactly when it reaches the descriptor upload, its first HIP call: without a device that one
    fails (-2, naming the upload), with one the call launches and returns 0.  Either way the answer is not the refusal -1."""
    import torch
    call, prob, bufs = harness(L)
    fn = L.lib.c.simq_grid_paths_large_work_bytes

    def accepted(*args, **kw):
        rc = call(*args, **kw)
        if torch.cuda.is_available():
            assert rc == 0, L.last_error()
            torch.cuda.synchronize()
        else:
            assert rc == -2 and 'upload_descriptors' in L.last_error(), (rc, L.last_error())

    big = dict(rows=200, cols=200, box_i0=0, box_j0=0, box_rows=140, box_cols=140)          # test_grid_waypoints_cpu.py:196
    assert 142 * 142 > 20000
    accepted([prob(**big)])
    accepted([prob(**big), prob(**dict(big, path_offset=16, work_offset=fn(140, 140)))], work_bytes=2 * fn(140, 140))     # end to end
    accepted([prob()], status=bufs['work'] + 1056, work_bytes=1056)                       # d_work ends where d_status begins
    accepted([prob(box_i0=0, box_j0=0, box_rows=0, box_cols=0)], work_bytes=32)           # the empty window


def test_split_by_window():
    from simq.waypoints import MAX_BOX_CELLS, entry_calls, restore_order, split_by_window, _window_order
    small, edge, over, wide = (3, 4, 50, 60), (0, 0, 98, 198), (0, 0, 140, 140), (1, 0, 1, 22000)
    assert 100 * 200 == MAX_BOX_CELLS and 142 * 142 > MAX_BOX_CELLS
    assert split_by_window([small, edge, (0, 0, 0, 0)]) == ([0, 1, 2], [])
    assert split_by_window([over, wide, (0, 0, 98, 199)]) == ([], [0, 1, 2])
    rng = np.random.RandomState(0)
    boxes = [(small, edge, over, wide)[k] for k in rng.randint(4, size=40)]
    fit, big = split_by_window(boxes)
    assert fit == [p for p, b in enumerate(boxes) if b in (small, edge)] and big == [p for p, b in enumerate(boxes) if b in (over, wide)]
    assert fit and big and sorted(fit + big) == list(range(40))
    descs = [dict(box=b, tag=p) for p, b in enumerate(boxes)]
    order, n_fit = _window_order(descs, True)
    assert order == fit + big and n_fit == len(fit)
    launched = [descs[p]['tag'] for p in order]                                     # what comes back in launch order ...
    assert restore_order(order, launched) == list(range(40))                        # ... is put back in problem order
    assert np.array_equal(np.asarray(launched)[np.argsort(order)], np.arange(40))
    assert _window_order(descs, False) == (list(range(40)), 40)                     # all to simq_grid_paths, which refuses
    # an empty part makes no call
    assert entry_calls(40, 40) == [('simq_grid_paths', 0, 40)]
    assert entry_calls(0, 40) == [('simq_grid_paths_large', 0, 40)]
    assert entry_calls(n_fit, 40) == [('simq_grid_paths', 0, n_fit), ('simq_grid_paths_large', n_fit, 40)]


def test_large_windows_argument(L, golden_dir):
    import simq
    grid = np.ones((4, 5), np.uint8)
    for bad in ('yes', 1, None):
        with pytest.raises(ValueError, match='large_windows'):
            simq.grid_dense_paths([grid], [(0, 0)], [(1, 1)], large_windows=bad)
        with pytest.raises(ValueError, match='large_windows'):
            simq.grid_waypoints([grid], [(0, 0)], [(1, 1)], large_windows=bad)
        with pytest.raises(ValueError, match='large_windows'):
            simq.shortest_paths([grid], [grid], [np.zeros((2, 4, 5), np.int32)], [(0., 0.)], [(0., 0.)], large_windows=bad)
        with pytest.raises(ValueError, match='large_windows'):
            simq.WaypointGraph(grid, large_windows=bad)
    # the host half of WaypointGraph does not depend on the keyword
    key, grid, source, dist, parents, targets, dense, ways = next(c for c in waypoint_cases(golden_dir) if c[0] == 'open_232_0')
    graphs = [simq.WaypointGraph(grid), simq.WaypointGraph(grid, large_windows=True)]
    assert [g.large_windows for g in graphs] == [False, True]
    for g in graphs:
        g.search = lambda grid_, s: oracle_search(key, golden_dir)[:2]
    for t, want_dense, want in list(zip(targets, dense, ways['every_third']))[:8]:
        got = [g.shortest_path(source, t, simplify=oracle.every_third) for g in graphs]
        assert got[0] == got[1]
        assert np.array_equal(np.asarray(got[1], np.int32).reshape(-1, 2), want)
        assert np.array_equal(graphs[1].dense_path(source, t), want_dense)
