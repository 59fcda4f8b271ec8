"""GPU: simq_grid_distance_queries (csrc/grid_queries.hip) against the reference's own OccupancyMap.shortest_path_distance
(tests/golden/grid_queries.npz), the numpy oracle (tests/grid_queries_oracle.py) and simq.grid_distance_images, bit for bit; the chain
from simq.occupancy_maps; what the launch writes and what it leaves alone; the refusals."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import grid_queries_oracle as oracle
from test_grid_queries_cpu import ROOMS, query_cases, random_problem

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 63, 64, 65, 130)                             # targets per problem: none, one, around the wave width, two rounds and more


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    import simq.grid_queries  # noqa: F401
    return simq


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def mixed_problems():
    """64 problems on random 20 x 30 to 40 x 50 grids, every count of COUNTS at least ten times, every other problem snapped through a
    closest block, and the oracle's distances.  Computed once and shared."""
    rng = np.random.RandomState(11)
    out = []
    for p in range(64):
        rows, cols = int(rng.randint(20, 41)), int(rng.randint(30, 51))
        grid, closest, source, targets = random_problem(rng, rows, cols, COUNTS[p % len(COUNTS)])
        if p % 8 in (3, 4):                                  # a blocked source for certain, snapped (p even) and not
            bi, bj = np.nonzero(grid == 0)
            source = (int(bi[0]), int(bj[0]))
        closest = closest if p % 2 == 0 else None
        out.append((grid, closest, source, targets, oracle.pixel_distances(grid, closest, source, targets)))
    return out


def test_golden_fixtures_through_the_position_wrapper(simq_mod, golden_dir):
    """Every fixture query, one launch per room: 13 maps x 2 sources x 20 targets, equal as float64 bits to what the reference's own
    OccupancyMap.shortest_path_distance returned."""
    for room in ROOMS:
        cases = list(query_cases(golden_dir, room))
        cspace, closest = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
        index = [m for m, *_ in cases for _ in range(len(cases[0][3]))]
        sources = [tuple(s) for c in cases for s in c[3]]
        targets = [[tuple(t) for t in ts] for c in cases for ts in c[4]]
        want = [w for c in cases for w in c[7]]
        got = simq_mod.shortest_path_distances(cspace, closest, sources, targets, map_index=index)
        assert len(got) == len(want) == 26
        for p, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.float64 and np.array_equal(bits(g), bits(w)), (room, index[p], p)
        # Mapper.distance_to_receptacle is the same call with the receptacle as the source
        again = simq_mod.distances_to_receptacle(cspace, closest, sources[:4], targets[:4], map_index=index[:4])
        assert all(np.array_equal(bits(a), bits(w)) for a, w in zip(again, want))


def test_golden_fixtures_through_the_raw_c_abi(simq_mod, golden_dir):
    from simq._lib import lib, ptr, stream_ptr
    from simq.grid_queries import GridQueryProblem
    dev = torch.device('cuda', torch.cuda.current_device())
    for room in ROOMS:
        cases = [c for c in query_cases(golden_dir, room) if c[0] in (0, 3, 11)]
        rows, cols = cases[0][1].shape
        cells, S, Q = rows * cols, 2, cases[0][6].shape[1]
        d_grids = torch.from_numpy(np.stack([c[1] for c in cases])).to(dev)
        d_closest = torch.from_numpy(np.stack([c[2] for c in cases])).to(dev)
        P = len(cases) * S
        probs = (GridQueryProblem * P)(*[GridQueryProblem(k * cells, 2 * k * cells, (k * S + s) * cells, (k * S + s) * Q, Q, rows, cols,
                                                          int(c[5][s][0]), int(c[5][s][1]), 0)
                                         for k, c in enumerate(cases) for s in range(S)])
        targets = np.ascontiguousarray(np.concatenate([c[6].reshape(-1, 2) for c in cases]).astype(np.int32))
        desc = torch.empty(ctypes.sizeof(probs) + 8 * len(targets), dtype=torch.uint8, device=dev)
        work = torch.empty(P * cells, dtype=torch.float32, device=dev)
        out = torch.full((P * Q,), -7.0, dtype=torch.float32, device=dev)
        status = torch.full((P,), -7, dtype=torch.int32, device=dev)
        lib.call('simq_grid_distance_queries', ptr(d_grids), ctypes.c_int64(d_grids.numel()), ptr(d_closest), ctypes.c_int64(d_closest.numel()),
                 probs, P, targets.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(targets)), ptr(desc), ptr(work),
                 ctypes.c_int64(work.numel()), 0, ptr(out), ctypes.c_int64(out.numel()), ptr(status), stream_ptr(dev))
        assert (status.cpu().numpy() == 0).all(), room
        got = out.cpu().numpy().astype(np.float64) / 96.0
        want = np.concatenate([c[7].reshape(-1) for c in cases])
        assert np.array_equal(bits(got), bits(want)), room


def test_mixed_shapes_and_counts_in_one_launch(simq_mod):
    """Q crosses the wave width and includes empty problems; targets on blocked cells, blocked sources (snapped and not) and targets
    in components the source cannot reach are all met; every other problem goes without a closest block."""
    from simq._lib import lib
    probs = mixed_problems()
    lib.call('simq_launch_counts_reset')
    got = simq_mod.grid_distance_queries([q[0] for q in probs], [q[2] for q in probs], [q[3] for q in probs], closest=[q[1] for q in probs])
    assert lib.c.simq_launch_count(b'grid_queries') == 1 and len(got) == 64
    seen = dict(blocked_target=0, blocked_source=0, snapped_source=0, unreachable=0, empty=0)
    for p, (g, (grid, closest, source, targets, want)) in enumerate(zip(got, probs)):
        assert g.dtype == torch.float32 and g.is_cuda and tuple(g.shape) == (len(targets),)
        assert np.array_equal(bits(g), bits(want)), p
        seen['blocked_target'] += sum(grid[t] == 0 for t in targets)
        seen['blocked_source'] += grid[source] == 0
        seen['snapped_source'] += grid[source] == 0 and closest is not None
        seen['unreachable'] += int((want < 0).sum())
        seen['empty'] += len(targets) == 0
    assert seen['blocked_target'] >= 200 and seen['blocked_source'] >= 16 and seen['snapped_source'] >= 8, seen
    assert seen['unreachable'] >= 100 and seen['empty'] >= 10, seen
    assert {len(t) for _, _, _, t, _ in probs} == set(COUNTS)


def test_distances_and_images_equal_grid_distance_images(simq_mod):
    """The query kernel and the image kernel share their relaxation: with images=True the whole working image equals
    simq.grid_distance_images for the snapped source, and every distance is that image at the snapped target."""
    probs = [q for q in mixed_problems() if q[1] is not None][:16]
    grids, closest = [q[0] for q in probs], [q[1] for q in probs]
    dists, images = simq_mod.grid_distance_queries(grids, [q[2] for q in probs], [q[3] for q in probs], closest=closest, images=True)
    snapped = [oracle.snap(q[1], q[2]) for q in probs]
    want = simq_mod.grid_distance_images(grids, snapped)
    for p, (grid, cl, source, targets, _) in enumerate(probs):
        assert tuple(images[p].shape) == grid.shape and np.array_equal(bits(images[p]), bits(want[p])), p
        host = want[p].cpu().numpy()
        at = np.asarray([host[oracle.snap(cl, t)] for t in targets], np.float32)
        assert np.array_equal(bits(dists[p]), bits(at)), p
    # and without images the distances are the same
    plain = simq_mod.grid_distance_queries(grids, [q[2] for q in probs], [q[3] for q in probs], closest=closest)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain, dists))


def test_degenerate_shapes(simq_mod):
    """P = 1; a single row and a single column; one free cell closed in by blocked ones; no free cell at all."""
    row = np.ones((1, 70), np.uint8)
    row[0, 40] = 0
    col = np.ones((70, 1), np.uint8)
    col[10, 0] = 0
    one = np.zeros((9, 11), np.uint8)
    one[4, 6] = 1
    none = np.zeros((5, 6), np.uint8)
    to_one = np.zeros((2, 9, 11), np.int32)
    to_one[0], to_one[1] = 4, 6
    cases = [(row, None, (0, 3), [(0, j) for j in range(70)]),
             (col, None, (69, 0), [(i, 0) for i in range(70)]),
             (one, None, (4, 6), [(4, 6), (4, 5), (0, 0), (8, 10)]),
             (one, to_one, (0, 0), [(4, 6), (4, 5), (0, 0), (8, 10)]),
             (none, None, (2, 2), [(2, 2), (2, 3), (0, 0)])]
    for k, (grid, cl, source, targets) in enumerate(cases):                         # P = 1 each
        got = simq_mod.grid_distance_queries([grid], [source], [targets], closest=None if cl is None else [cl])
        want = oracle.pixel_distances(grid, cl, source, targets)
        assert len(got) == 1 and np.array_equal(bits(got[0]), bits(want)), k
    assert oracle.pixel_distances(row, None, (0, 3), [(0, 39), (0, 41)]).tolist() == [36.0, -1.0]
    assert oracle.pixel_distances(one, to_one, (0, 0), [(0, 0), (8, 10)]).tolist() == [0.0, 0.0]
    assert oracle.pixel_distances(one, None, (4, 6), [(4, 6), (4, 5)]).tolist() == [0.0, -1.0]


@pytest.mark.parametrize('room', ROOMS)
def test_full_size_fixture_map_with_20_targets(simq_mod, golden_dir, room):
    """One cluttered map of each room shape at the pixel level: 20 targets from each of its two sources, against the reference's
    results and against the distance image."""
    m, cspace, closest, _, _, src_px, tgt_px, want = next(c for c in query_cases(golden_dir, room) if c[0] == 4)
    sources = [tuple(int(x) for x in s) for s in src_px]
    targets = [[tuple(int(x) for x in t) for t in ts[:20]] for ts in tgt_px]
    dists, images = simq_mod.grid_distance_queries([cspace], sources, targets, grid_index=[0, 0], closest=[closest], images=True)
    ref = simq_mod.grid_distance_images([cspace], [oracle.snap(closest, s) for s in sources], grid_index=[0, 0])
    for s in range(2):
        assert tuple(dists[s].shape) == (20,)
        assert np.array_equal(bits(dists[s].cpu().numpy().astype(np.float64) / 96.0), bits(want[s][:20])), (room, s)
        assert np.array_equal(bits(images[s]), bits(ref[s])), (room, s)


@pytest.mark.parametrize('room', ROOMS)
def test_chain_from_occupancy_maps(simq_mod, golden_dir, room, monkeypatch):
    """simq.occupancy_maps feeds simq.shortest_path_distances on the device: one occupancy launch, one query launch, no distance-image
    launch, no host array uploaded through torch and one read-back; the result equals the reference's and the oracle's."""
    from simq._lib import lib
    z = np.load(os.path.join(golden_dir, 'occupancy_maps_%s.npz' % room))
    cases = list(query_cases(golden_dir, room))
    index = [m for m, *_ in cases for _ in range(2)]
    sources = [tuple(s) for c in cases for s in c[3]]
    targets = [[tuple(t) for t in ts] for c in cases for ts in c[4]]
    lib.call('simq_launch_counts_reset')
    maps = simq_mod.occupancy_maps(z['occupancy'], z['room_mask'], z['radius'].tolist(), z['thin_radius'].tolist())
    assert maps.configuration_space.is_cuda and maps.closest_cspace_indices.is_cuda

    reads = []
    real_cpu = torch.Tensor.cpu

    def no_upload(a):
        raise AssertionError('a host array of %s went to the device' % (a.shape,))

    def counted_cpu(self, *args, **kw):
        reads.append(tuple(self.shape))
        return real_cpu(self, *args, **kw)
    monkeypatch.setattr(torch, 'from_numpy', no_upload)
    monkeypatch.setattr(torch.Tensor, 'cpu', counted_cpu)
    got = simq_mod.shortest_path_distances(maps.configuration_space, maps.closest_cspace_indices, sources, targets, map_index=index)
    monkeypatch.undo()
    total = sum(len(t) for t in targets)
    assert reads == [(total + len(sources),)]                                       # the packed distances and the status words, once
    assert lib.c.simq_launch_count(b'occupancy_maps') == 1 and lib.c.simq_launch_count(b'grid_queries') == 1
    assert lib.c.simq_launch_count(b'grid_distance') == 0 and lib.c.simq_launch_count(b'grid_waypoints') == 0
    for p, c in enumerate(cases):
        for s in range(2):
            assert np.array_equal(bits(got[2 * p + s]), bits(c[7][s])), (room, p, s)
    for p in (0, 5):                                                                # and the oracle itself, on two of the maps
        m, cspace, closest, src, tgt = cases[p][:5]
        cache = {}
        want = [oracle.shortest_path_distance(cspace, closest, src[0], t, cache) for t in tgt[0]]
        assert np.array_equal(bits(got[2 * p]), bits(np.asarray(want, np.float64))), (room, p)


def raw_call(grid, closest, probs_fields, targets, images, fill, lead=37, gap=19, **sizes):
    """simq_grid_distance_queries on buffers filled with `fill`, every problem's spans placed by the caller inside larger buffers.
    Returns (rc, work, out, status) as host arrays."""
    from simq._lib import lib, ptr, stream_ptr
    from simq.grid_queries import GridQueryProblem
    dev = torch.device('cuda', torch.cuda.current_device())
    d_grid = torch.from_numpy(grid).to(dev)
    d_closest = None if closest is None else torch.from_numpy(closest).to(dev)
    P = len(probs_fields)
    probs = (GridQueryProblem * P)(*[GridQueryProblem(*f) for f in probs_fields])
    flat = np.ascontiguousarray(np.asarray(targets, np.int32).reshape(-1, 2))
    desc = torch.empty(ctypes.sizeof(probs) + 8 * len(flat), dtype=torch.uint8, device=dev)
    work = torch.full((sizes.get('work_floats', 0) + lead + gap,), fill, dtype=torch.float32, device=dev)
    out = torch.full((sizes.get('out_floats', len(flat)) + gap,), fill, dtype=torch.float32, device=dev)
    status = torch.full((P + 2,), -7, dtype=torch.int32, device=dev)
    rc = lib.c.simq_grid_distance_queries(ptr(d_grid), sizes.get('grids_bytes', grid.size), ptr(d_closest),
                                          sizes.get('closest_ints', 0 if closest is None else closest.size), probs, P,
                                          flat.ctypes.data_as(ctypes.c_void_p), len(flat), ptr(desc), ptr(work), work.numel(), images,
                                          ptr(out), sizes.get('out_floats', len(flat)), ptr(status), stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, work.cpu().numpy(), out.cpu().numpy(), status.cpu().numpy()


def test_dirty_memory_is_overwritten_and_nothing_else_is_touched(simq_mod):
    """Two problems on one grid whose working images and target ranges lie apart inside larger buffers: whatever the buffers held,
    the spans come out the same, and every float outside them keeps its fill."""
    grid, closest, source, targets, _ = next(q for q in mixed_problems() if q[1] is not None and len(q[3]) == 65)
    rows, cols = grid.shape
    cells = rows * cols
    other = (rows - 1, cols - 1)
    # targets: [0, 65) problem 1's, [65, 70) unused, [70, 135) problem 0's; working images at floats 37 and 37 + cells + 11
    flat = list(targets) + [(0, 0)] * 5 + list(targets)
    fields = [(0, 0, 37, 70, 65, rows, cols, source[0], source[1], 0), (0, 0, 37 + cells + 11, 0, 65, rows, cols, other[0], other[1], 0)]
    want = [oracle.pixel_distances(grid, closest, s, targets) for s in (source, other)]
    image = [simq_mod.grid_distance_images([grid], [oracle.snap(closest, s)])[0].cpu().numpy() for s in (source, other)]
    results = []
    for fill in (-7.0, float('nan'), 0.0):
        rc, work, out, status = raw_call(grid, closest, fields, flat, 1, fill, work_floats=2 * cells + 11, out_floats=135)
        assert rc == 0 and status.tolist() == [0, 0, -7, -7]
        assert np.array_equal(bits(out[70:135]), bits(want[0])) and np.array_equal(bits(out[0:65]), bits(want[1]))
        assert np.array_equal(bits(work[37:37 + cells]), bits(image[0].reshape(-1)))
        assert np.array_equal(bits(work[37 + cells + 11:37 + 2 * cells + 11]), bits(image[1].reshape(-1)))
        untouched = np.concatenate([out[65:70], out[135:], work[:37], work[37 + cells:37 + cells + 11], work[37 + 2 * cells + 11:]])
        assert len(untouched) == 5 + 19 + 37 + 11 + 19 and np.array_equal(bits(untouched), bits(np.full(len(untouched), fill, np.float32)))
        results.append(np.concatenate([out[0:65], out[70:135]]))
    assert all(np.array_equal(bits(r), bits(results[0])) for r in results)
    # scratch mode (images = 0) gives the same distances and stays inside the same spans
    rc, work, out, status = raw_call(grid, closest, fields, flat, 0, -7.0, work_floats=2 * cells + 11, out_floats=135)
    assert rc == 0 and np.array_equal(bits(out[70:135]), bits(want[0])) and np.array_equal(bits(out[0:65]), bits(want[1]))
    assert (np.concatenate([out[65:70], out[135:], work[:37], work[37 + cells:37 + cells + 11], work[37 + 2 * cells + 11:]]) == -7.0).all()


def test_a_closest_cell_outside_the_grid_is_status_2(simq_mod):
    """What the host cannot see: a closest block on the device that names a cell outside the grid.  The kernel re-checks: a bad
    source writes nothing, a bad target leaves only its own distance unwritten."""
    grid = np.ones((6, 7), np.uint8)
    closest = np.stack(np.mgrid[0:6, 0:7]).astype(np.int32)                         # every cell its own closest
    closest[0, 2, 3] = 6                                                            # row 6 of a 6-row grid
    fields = [(0, 0, 37, 0, 3, 6, 7, 2, 3, 0), (0, 0, 37 + 42, 3, 3, 6, 7, 0, 0, 0)]
    flat = [(0, 0), (1, 1), (2, 2), (0, 1), (2, 3), (0, 2)]
    rc, work, out, status = raw_call(grid, closest, fields, flat, 0, -7.0, work_floats=84, out_floats=6)
    assert rc == 0 and status[:2].tolist() == [2, 2]
    assert (out[:3] == -7.0).all() and (work[37:37 + 42] == -7.0).all()             # the bad source: nothing written
    assert out[3:6].tolist() == [1.0, -7.0, 2.0]                                    # the bad target alone is left out
    with pytest.raises(simq_mod.grid_queries.SimqError, match='status'):
        simq_mod.grid_distance_queries([grid], [(2, 3)], [[(0, 0)]], closest=[closest])


def test_refusals_launch_nothing(simq_mod):
    from simq._lib import last_error, lib
    grid = np.ones((6, 7), np.uint8)
    closest = np.stack(np.mgrid[0:6, 0:7]).astype(np.int32)
    dev = torch.device('cuda', torch.cuda.current_device())
    ok = (0, 0, 37, 0, 2, 6, 7, 1, 1, 0)
    two = [(0, 0), (5, 6), (1, 1), (2, 2)]
    lib.call('simq_launch_counts_reset')

    def refused(word, *args, **kw):
        rc, work, out, status = raw_call(*args, **kw)
        assert rc == -1 and word in last_error(), (word, last_error())
        assert (work == -7.0).all() and (out == -7.0).all() and (status == -7).all(), word
        assert lib.c.simq_launch_count(b'grid_queries') == 0, word

    refused('target 1 (6, 6) outside its 6 x 7 grid', grid, closest, [ok], [(0, 0), (6, 6)], 0, -7.0, work_floats=42)
    refused('closest ints [0, 84) outside the 83', grid, closest, [ok], two[:2], 0, -7.0, work_floats=42, closest_ints=83)
    refused('problems 0 and 1 share d_out', grid, closest, [ok, (0, 0, 37 + 42, 1, 2, 6, 7, 2, 2, 0)], two, 0, -7.0, work_floats=84)
    # d_out inside the grids: the last 8 of the 42 grid bytes
    from simq._lib import ptr, stream_ptr
    from simq.grid_queries import GridQueryProblem
    d_grid = torch.ones(64, dtype=torch.uint8, device=dev)
    probs = (GridQueryProblem * 1)(GridQueryProblem(0, -1, 37, 0, 2, 6, 7, 1, 1, 0))
    flat = np.asarray(two[:2], np.int32)
    desc = torch.empty(56 + 16, dtype=torch.uint8, device=dev)
    work = torch.full((42 + 37,), -7.0, dtype=torch.float32, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = lib.c.simq_grid_distance_queries(ptr(d_grid), 42, None, 0, probs, 1, flat.ctypes.data_as(ctypes.c_void_p), 2, ptr(desc), ptr(work),
                                          work.numel(), 0, ptr(d_grid[32:40].view(torch.float32)), 2, ptr(status), stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == -1 and 'd_out overlaps d_grids' in last_error(), last_error()
    assert lib.c.simq_launch_count(b'grid_queries') == 0
    assert (d_grid.cpu().numpy() == 1).all() and (work.cpu().numpy() == -7.0).all() and status.item() == -7
    # the wrapper turns a refusal into a SimqError that carries the library's message
    with pytest.raises(simq_mod.grid_queries.SimqError, match='target 0 .7, 0. outside its 6 x 7 grid'):
        simq_mod.grid_distance_queries([grid], [(0, 0)], [[(7, 0)]])
    assert lib.c.simq_launch_count(b'grid_queries') == 0
