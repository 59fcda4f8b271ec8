"""CPU: the point-query oracle against the reference's own OccupancyMap.shortest_path_distance (tests/golden/grid_queries.npz, written
by tools/gen_grid_queries_golden.py) and against the distance images of tests/grid_paths_oracle.py, the C-ABI entry
simq_grid_distance_queries and its refusals, and every argument error of the wrappers (no kernel is launched here)."""
import ctypes
import math
import os

import numpy as np
import pytest

import grid_paths_oracle
import grid_queries_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOMS = ('184x232', '232x232')


def query_cases(golden_dir, room):
    """(map index, configuration space, closest, [S, 2] source positions, [S, Q, 2] target positions, [S, 2] and [S, Q, 2] pixels,
    [S, Q] float64 reference results) per map of the room's occupancy fixture."""
    maps = np.load(os.path.join(golden_dir, 'occupancy_maps_%s.npz' % room))
    z = np.load(os.path.join(golden_dir, 'grid_queries.npz'))
    for m in range(len(maps['names'])):
        yield (m, maps['configuration_space'][m], maps['closest'][m]) + tuple(
            z['%s_%s' % (k, room)][m] for k in ('source_positions', 'target_positions', 'source_pixels', 'target_pixels', 'distances'))


def random_problem(rng, rows, cols, n_targets, blocked=0.25):
    """A random grid with a wall that cuts a corner off, a closest block (nearest free cell by brute force, any tie rule: it only has
    to name a free cell), a source and targets anywhere in the grid -- on blocked cells and across the wall included."""
    grid = (rng.rand(rows, cols) >= blocked).astype(np.uint8)
    k = min(rows, cols) // 3
    grid[k, :k + 1] = 0
    grid[:k + 1, k] = 0                                                             # the corner [0, k) x [0, k) is its own component
    grid[0, 0] = grid[rows - 1, cols - 1] = 1
    fi, fj = np.nonzero(grid)
    ii, jj = np.mgrid[0:rows, 0:cols]
    near = ((ii[..., None] - fi) ** 2 + (jj[..., None] - fj) ** 2).argmin(-1)
    closest = np.stack([fi[near], fj[near]]).astype(np.int32)
    source = (int(rng.randint(rows)), int(rng.randint(cols)))
    targets = [(int(rng.randint(rows)), int(rng.randint(cols))) for _ in range(n_targets)]
    return grid, closest, source, targets


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


@pytest.mark.parametrize('room', ROOMS)
def test_oracle_equals_the_reference_bit_for_bit(golden_dir, room):
    n = unreachable = 0
    for m, cspace, closest, src, tgt, src_px, tgt_px, want in query_cases(golden_dir, room):
        assert src.dtype == tgt.dtype == want.dtype == np.float64 and want.shape == tgt.shape[:2] and want.shape[1] >= 20
        cache = {}
        for s in range(len(src)):
            assert oracle.position_to_pixel_indices(src[s][0], src[s][1], cspace.shape) == tuple(src_px[s])
            for t in range(tgt.shape[1]):
                assert oracle.position_to_pixel_indices(tgt[s, t][0], tgt[s, t][1], cspace.shape) == tuple(tgt_px[s, t])
                got = oracle.shortest_path_distance(cspace, closest, src[s], tgt[s, t], cache)
                assert np.float64(got).view(np.int64) == want[s, t].view(np.int64), (room, m, s, t)
                assert got == oracle.distance_to_receptacle(cspace, closest, src[s], tgt[s, t], cache=cache)
                unreachable += got == -1 / 96
                n += 1
    assert n >= 13 * 40 and unreachable >= 4


def test_oracle_is_the_distance_image_at_the_snapped_pixels():
    rng = np.random.RandomState(5)
    snapped = cut = 0
    for k in range(12):
        rows, cols = int(rng.randint(20, 41)), int(rng.randint(30, 51))
        grid, closest, source, targets = random_problem(rng, rows, cols, 40)
        for cl in (closest, None):
            got = oracle.pixel_distances(grid, cl, source, targets)
            s = tuple(int(x) for x in closest[:, source[0], source[1]]) if cl is not None else source
            image = grid_paths_oracle.distance_image(grid, s)
            want = [image[tuple(closest[:, i, j])] if cl is not None else image[i, j] for i, j in targets]
            assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), np.asarray(want, np.float32).view(np.int32))
            if cl is not None:
                assert (grid[closest[0], closest[1]] != 0).all()
                snapped += sum(grid[t] == 0 for t in targets)
                cut += int((got < 0).sum())
    assert snapped >= 60 and cut >= 12                       # the random problems do meet blocked targets and other components


def test_euclidean_branch_is_the_reference_expression():
    rec, pos = (0.31, -0.42, 0.0), (-0.17, 0.05)
    want = math.sqrt((rec[0] - pos[0])**2 + (rec[1] - pos[1])**2)
    assert oracle.distance_to_receptacle(None, None, rec, pos, shortest_path=False) == want == oracle.distance(pos, rec)


def test_export_is_declared_bound_and_laid_out(L):
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    assert 'int simq_grid_distance_queries(' in text and 'envs.py:2506-2511' in text
    assert 'simq_grid_distance_queries' in L.EXPORTS and hasattr(ctypes.CDLL(L.LIB_PATH), 'simq_grid_distance_queries')
    from simq.grid_queries import GridQueryProblem
    struct = text[text.index('typedef struct simq_grid_query_problem {'):text.index('} simq_grid_query_problem;')]
    names = [n for line in struct.splitlines()[1:] for n in line.split(';')[0].split(None, 1)[1].replace(' ', '').split(',')]
    assert names == [n for n, _ in GridQueryProblem._fields_]
    offsets = [getattr(GridQueryProblem, n).offset for n in names]
    assert offsets == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52] and ctypes.sizeof(GridQueryProblem) == 56
    import simq
    assert callable(simq.grid_distance_queries) and callable(simq.shortest_path_distances) and callable(simq.distances_to_receptacle)


def test_c_abi_rejects_bad_calls_before_any_device_call(L):
    """Every check of simq_grid_distance_queries runs on the host before the descriptor copy and the launch (the fake device pointers
    below are never dereferenced), and a refused call leaves the launch log alone."""
    from simq.grid_queries import GridQueryProblem
    c = L.lib.c
    base = 1 << 32
    bufs = dict(grids=base, closest=base + (1 << 26), desc=base + (2 << 26), work=base + (3 << 26), out=base + (4 << 26),
                status=base + (5 << 26))

    def call(descs, targets=((1, 2), (3, 4), (5, 6), (7, 8)), n=None, grids_bytes=1 << 20, closest_ints=1 << 20, work_floats=1 << 20,
             out_floats=1 << 10, images=0, **ptrs):
        a = {k: ctypes.c_void_p(v) if v else None for k, v in dict(bufs, **ptrs).items()}
        arr = (GridQueryProblem * len(descs))(*descs)
        flat = np.asarray(targets, np.int32).reshape(-1, 2)
        return c.simq_grid_distance_queries(a['grids'], grids_bytes, a['closest'], closest_ints, arr, len(descs) if n is None else n,
                                            flat.ctypes.data_as(ctypes.c_void_p) if len(flat) else None, len(flat), a['desc'], a['work'],
                                            work_floats, images, a['out'], out_floats, a['status'], None)

    def prob(**kw):
        f = dict(grid_offset=0, closest_offset=-1, work_offset=0, target_offset=0, n_targets=2, rows=10, cols=12, src_i=3, src_j=4,
                 reserved_=0)
        f.update(kw)
        return GridQueryProblem(*[f[n] for n, _ in GridQueryProblem._fields_])

    L.lib.call('simq_launch_counts_reset')

    def refused(word, *args, **kw):
        assert call(*args, **kw) == -1, word
        assert word in L.last_error(), (word, L.last_error())

    refused('NULL', [prob()], work=0)
    refused('NULL targets or d_out', [prob()], out=0)
    refused('n = 0', [prob()], n=0)
    refused('images = 2', [prob()], images=2)
    refused('2^22', [prob(rows=2048, cols=2048)])
    refused('is 0 x 12', [prob(rows=0)])
    refused('source (10, 4) outside', [prob(src_i=10)])
    refused('source (3, -1) outside', [prob(src_j=-1)])
    refused('target 1 (3, 12) outside its 10 x 12 grid', [prob()], targets=((1, 2), (3, 12)))
    refused('target 0 (-1, 2) outside', [prob(target_offset=1, n_targets=1)], targets=((1, 2), (-1, 2)))
    refused('targets [3, 5) outside the 4', [prob(target_offset=3)])
    refused('targets [0, -1) outside', [prob(n_targets=-1)])
    refused('grid bytes', [prob()], grids_bytes=119)
    refused('grid bytes', [prob(grid_offset=-1)])
    refused('closest ints [1, 241) outside the 240', [prob(closest_offset=1)], closest_ints=240)
    refused('closest ints', [prob(closest_offset=0)], closest=0)
    refused('closest ints', [prob(closest_offset=-2)])
    refused('working image floats [1, 121) outside the 120', [prob(work_offset=1)], work_floats=120)
    refused('d_out holds 3 floats, the targets need 4', [prob()], out_floats=3)
    refused('problems 0 and 1 share working image', [prob(), prob(work_offset=119, target_offset=2)])
    refused('problems 0 and 1 share d_out', [prob(), prob(work_offset=120, target_offset=1)])
    refused('d_out overlaps d_grids', [prob()], out=bufs['grids'] + 64)
    refused('d_work overlaps d_closest', [prob(closest_offset=0)], work=bufs['closest'] + 4 * 100)
    refused('d_work overlaps d_out', [prob()], out=bufs['work'] + 4 * 119)
    refused('d_status overlaps d_descriptors', [prob()], status=bufs['desc'] + 56 + 28)          # inside the uploaded targets
    refused('aligned', [prob()], out=bufs['out'] + 2)
    refused('aligned', [prob()], desc=bufs['desc'] + 4)
    refused('aligned', [prob(closest_offset=0)], closest=bufs['closest'] + 1)
    assert c.simq_launch_count(b'grid_queries') == 0


def test_wrappers_raise_value_errors_before_asking_for_a_device(L, monkeypatch):
    import torch
    import simq
    from simq import _batch

    def no_device(what):
        raise AssertionError('the device was asked for (%s) before the arguments were checked' % what)
    monkeypatch.setattr(_batch, 'device', no_device)
    g = np.ones((4, 5), np.uint8)
    cl = np.zeros((2, 4, 5), np.int32)
    q = simq.grid_distance_queries
    for args, kw in ((([g.astype(np.float32)], [(0, 0)], [[(1, 1)]]), {}),                       # a grid that is not uint8
                     (([g], [(0, 0, 0)], [[(1, 1)]]), {}),                                      # a source that is no pair
                     (([g], [(0, 0)], [[(1, 1, 1)]]), {}),                                      # a target that is no pair
                     (([g], [(0, 0)], [3]), {}),                                                # targets[p] that is no sequence
                     (([g], [(0, 0)], [[(1, 1)], [(2, 2)]]), {}),                               # more target lists than sources
                     (([g], [], []), {}),                                                       # no problem
                     (([], [(0, 0)], [[]]), {}),                                                # no grid
                     (([g, g], [(0, 0)], [[]]), {}),                                            # two grids, one source, no index
                     (([g], [(0, 0)], [[]]), dict(grid_index=[1])),                             # an index outside the grids
                     (([g], [(0, 0)], [[]]), dict(closest=[cl.astype(np.int64)])),              # closest that is not int32
                     (([g], [(0, 0)], [[]]), dict(closest=[cl[:1]])),                           # ... not [2, rows, cols]
                     (([g], [(0, 0)], [[]]), dict(closest=[cl, cl])),                           # ... not one per grid
                     (([g], [(0, 0)], [[]]), dict(closest=[np.zeros((2, 5, 4), np.int32)]))):   # ... of another shape
        with pytest.raises(ValueError):
            q(*args, **kw)
    d = simq.shortest_path_distances
    for args, kw in ((([g], [cl], [(0.0, 0.0)], [[(0.1, 0.1)], []]), {}),                        # more target lists than sources
                     (([g], [cl], [(0.0,)], [[(0.1, 0.1)]]), {}),                               # a source that is no position
                     (([g], [cl], [(0.0, 0.0)], [[(0.1,)]]), {}),                               # a target that is no position
                     (([g], [cl], [(0.0, 0.0)], [0.1]), {}),                                    # target_positions[p] that is no sequence
                     (([g], [cl], [], []), {}),                                                 # no problem
                     (([g], [cl], 7, [[]]), {}),                                                # sources that are no sequence
                     (([g], None, [(0.0, 0.0)], [[]]), {}),                                     # no closest cells
                     (([g, g], [cl, cl], [(0.0, 0.0)], [[]]), {}),                              # two maps, one source, no index
                     (([g], [cl], [(0.0, 0.0)], [[]]), dict(map_index=[2])),
                     (([g], [cl], [(0.0, 0.0)], [[]]), dict(pixels_per_meter=0)),
                     (([g], [cl], [(0.0, 0.0)], [[]]), dict(pixels_per_meter=float('inf'))),
                     (([g.astype(np.int32)], [cl], [(0.0, 0.0)], [[]]), {})):
        with pytest.raises(ValueError):
            d(*args, **kw)
    r = simq.distances_to_receptacle
    with pytest.raises(ValueError):
        r([g], [cl], [(0.0, 0.0)], [[(0.1, 0.1)], []])
    for kw in (dict(receptacle_positions=[(0.0,)], positions=[[]]), dict(receptacle_positions=[(0.0, 0.0)], positions=[[], []]),
               dict(receptacle_positions=3, positions=[[]]), dict(receptacle_positions=[(0.0, 0.0)], positions=[[(1.0,)]])):
        with pytest.raises(ValueError):
            r(None, None, shortest_path=False, **kw)
    monkeypatch.undo()
    # with correct arguments and no GPU the wrappers say so; nothing falls back to the host
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(L.SimqError, match='MI355X'):
        q([g], [(0, 0)], [[(1, 1)]])
    with pytest.raises(L.SimqError, match='MI355X'):
        d([g], [cl], [(0.0, 0.0)], [[(0.01, 0.01)]])


def test_euclidean_distances_to_receptacle_need_no_device(L, monkeypatch):
    """shortest_path=False is the reference's distance(position, receptacle_position) in float64, in its operation order."""
    import simq
    from simq import _batch
    monkeypatch.setattr(_batch, 'device', lambda what: (_ for _ in ()).throw(AssertionError('no device is needed')))
    rng = np.random.RandomState(2)
    recs = [tuple(rng.uniform(-1, 1, 3)) for _ in range(3)]
    cubes = [[tuple(rng.uniform(-1, 1, 3)) for _ in range(q)] for q in (4, 0, 7)]
    got = simq.distances_to_receptacle(None, None, recs, cubes, shortest_path=False)
    assert [g.shape for g in got] == [(4,), (0,), (7,)] and all(g.dtype == np.float64 for g in got)
    for rec, ps, g in zip(recs, cubes, got):
        for p, x in zip(ps, g):
            assert float(x) == oracle.distance(p, rec) == math.sqrt((rec[0] - p[0])**2 + (rec[1] - p[1])**2)
