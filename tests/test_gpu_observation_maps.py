"""GPU: simq_observation_update (csrc/observation_maps.hip) against the fixtures the reference's Mapper / OccupancyMap wrote and against
the numpy oracle, which defines the order of points of equal height (tests/observation_maps_oracle.py)."""
import ctypes
import os

import numpy as np
import pytest

import observation_maps_oracle as oracle
import occupancy_maps_oracle

pytestmark = pytest.mark.gpu
F = np.float32
FILES = ('observation_maps_184x232.npz', 'observation_maps_232x232.npz')
CAMERAS = {'overhead': (0.1, 10, 1), 'forward': (0.001, 1, 16.0 / 9)}
RANGES = oracle.IdRanges(3, 9, 10, 11, 20)
ID_PALETTE = np.asarray([-1, 0, 0, 0, 0, 1, 2, 3, 5, 9, 10, 10, 11, 20, 21], np.int32)


@pytest.fixture(scope='module')
def S():
    import torch
    import simq
    from simq import observation
    assert torch.cuda.is_available()
    return simq, observation, torch


def sim_geometry(ob, g):
    return ob.CameraGeometry(*g)


def sim_ranges(ob, r):
    return ob.IdRanges(*r)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == F else a.dtype)


def check_against_reference(name, rec, over, occ):
    """The tie condition of the fixtures: equal to the reference off the ambiguous pixels, equal to the oracle everywhere."""
    want_over, want_occ = rec['overhead_before'].copy(), rec['occupancy_before'].copy()
    assert oracle.update(want_over, want_occ, rec['depth'], rec['ids'], rec['geometry'], rec['ranges']) == 0
    _, ambiguous, _ = oracle.tied_pixels(over.shape, rec['depth'], rec['ids'], rec['geometry'], rec['ranges'])
    assert name.startswith('tie_') == bool(ambiguous.any())
    assert np.array_equal(bits(over)[~ambiguous], bits(rec['overhead_after'])[~ambiguous]), name
    assert np.array_equal(bits(over), bits(want_over)), name
    assert np.array_equal(occ, rec['occupancy_after']), name


def random_problem(rng, k, shape):
    """A random frame of either camera at a pose up to the border of a map of `shape`: depth values from a few levels, so that points
    of equal height and different seg share pixels."""
    kind = ('overhead', 'forward')[k % 2]
    near, far, aspect = CAMERAS[kind]
    heading = rng.uniform(-np.pi, np.pi)
    x, y = rng.uniform(-shape[1] / 192.0, shape[1] / 192.0), rng.uniform(-shape[0] / 192.0, shape[0] / 192.0)
    if kind == 'overhead':
        g = oracle.camera_geometry((x, y, 1), (x, y, 0), (np.cos(heading), np.sin(heading), 0), near, far, aspect, 156)
        levels = ((far - far * near / np.asarray([1.0, 0.956, 0.9, 0.8])) / (far - near)).astype(F)
        buffer = levels[rng.randint(0, 4, (156 // 4 + 1, 156 // 4 + 1))].repeat(4, 0).repeat(4, 1)[:156, :156]
        buffer = np.where(rng.rand(156, 156) < 0.7, levels[0], buffer).astype(F)
    else:
        c = np.cos(np.radians(60))
        g = oracle.camera_geometry((x, y, 0.08), (x + 0.14 * np.cos(heading), y + 0.14 * np.sin(heading), 0),
                                   (c * np.cos(heading), c * np.sin(heading), np.sin(np.radians(60))), near, far, aspect, 156)
        buffer = np.where(rng.rand(156, 277) < 0.2, 1.0, rng.uniform(0.99, 1.0, (156, 277))).astype(F)
    ids = ID_PALETTE[rng.randint(0, ID_PALETTE.size, (buffer.shape[0] // 3 + 1, buffer.shape[1] // 3 + 1))].repeat(3, 0).repeat(3, 1)
    ids = np.ascontiguousarray(ids[:buffer.shape[0], :buffer.shape[1]])
    r = oracle.IdRanges(3, 9, None if k % 5 == 0 else 10, 11, 20)
    return np.ascontiguousarray(buffer), ids, g, r


def prefilled(rng, shape):
    over = np.full(shape, -3.0, F)
    occ = np.where(rng.rand(*shape) < 0.3, 7, 0).astype(np.uint8)
    return over, occ


@pytest.mark.parametrize('fname', FILES)
def test_fixtures_through_observation_update_observe_and_the_c_abi(S, golden_dir, fname):
    simq, ob, torch = S
    from simq._lib import lib, ptr, stream_ptr
    top, cases = oracle.load_fixture(os.path.join(golden_dir, fname))
    # one launch over every frame of the file, each on its own pair of maps (mixed camera shapes)
    overs = [torch.from_numpy(rec['overhead_before'].copy()).cuda() for _, rec in cases]
    occs = [torch.from_numpy(rec['occupancy_before'].copy()).cuda() for _, rec in cases]
    geoms = []
    for _, rec in cases:
        c = rec['camera_constants'].tolist()
        g = simq.camera_geometry(tuple(rec['camera'][0].tolist()), tuple(rec['camera'][1].tolist()), tuple(rec['camera'][2].tolist()),
                                 c[0], c[1], c[2], int(c[3]), c[4])
        for a, b in zip(g, rec['geometry']):
            assert np.array_equal(bits(np.asarray(a, F).reshape(-1)), bits(np.asarray(b, F).reshape(-1)))
        geoms.append(g)
    simq.observation_update([rec['depth'] for _, rec in cases], [rec['ids'] for _, rec in cases], geoms,
                            [sim_ranges(ob, rec['ranges']) for _, rec in cases], overs, occs)
    for (name, rec), over, occ in zip(cases, overs, occs):
        check_against_reference(name, rec, over.cpu().numpy(), occ.cpu().numpy())
    for (name, rec), g in list(zip(cases, geoms))[::3]:
        before = rec['overhead_before'].copy()
        over, occ = simq.observe(rec['depth'], rec['ids'], g, sim_ranges(ob, rec['ranges']), rec['overhead_before'], rec['occupancy_before'])
        assert np.array_equal(before, rec['overhead_before'])
        check_against_reference(name, rec, over, occ)
    # the C-ABI with the stored vectors, two frames in one buffer
    for a, b in ((0, len(cases) - 1), (1, len(cases) - 2)):
        recs = [cases[a][1], cases[b][1]]
        words, offs = 0, []
        parts = []
        for rec in recs:
            o = []
            for arr in (rec['depth'], rec['ids'], rec['pixel_x'], rec['pixel_y']):
                o.append(words)
                parts.append(np.ascontiguousarray(arr).reshape(-1).view(np.int32))
                words += arr.size
            offs.append(o)
        frames = torch.from_numpy(np.concatenate(parts)).cuda()
        rows, cols = recs[0]['overhead_before'].shape
        over = torch.from_numpy(np.stack([r_['overhead_before'] for r_ in recs])).cuda()
        occ = torch.from_numpy(np.stack([r_['occupancy_before'] for r_ in recs])).cuda()
        probs = (ob.ObservationProblem * 2)()
        for k, (rec, o) in enumerate(zip(recs, offs)):
            q = probs[k]
            q.depth_offset, q.ids_offset, q.px_offset, q.py_offset = o
            q.overhead_offset = q.occupancy_offset = k * rows * cols
            v = rec['vectors']
            q.cam, q.principal, q.right, q.up = [(ctypes.c_float * 3)(*v[i].tolist()) for i in range(4)]
            q.far_near, q.far, q.far_minus_near = rec['depth_constants'].tolist()
            q.min_obstacle, q.max_obstacle, q.receptacle, q.has_receptacle, q.min_cube, q.max_cube = rec['id_ranges'].tolist()
            q.height, q.width = rec['depth'].shape
            q.rows, q.cols = rows, cols
        d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device='cuda')
        status = torch.full((2,), -1, dtype=torch.int32, device='cuda')
        lib.call('simq_observation_update', ptr(frames), ctypes.c_int64(words), probs, 2, ptr(d_probs), ptr(over), ctypes.c_int64(over.numel()),
                 ptr(occ), ctypes.c_int64(occ.numel()), ptr(status), stream_ptr(over.device))
        assert status.cpu().tolist() == [0, 0]
        for k, idx in enumerate((a, b)):
            check_against_reference(cases[idx][0], recs[k], over[k].cpu().numpy(), occ[k].cpu().numpy())


def test_mixed_launch_of_random_problems_equals_the_oracle(S):
    """160 problems in one launch: both cameras, both room shapes, poses up to the border of the map (points clip to border pixels),
    equal heights with different seg values (the oracle defines who wins), maps prefilled with a sentinel that every pixel no point
    reached must keep."""
    simq, ob, torch = S
    rng = np.random.RandomState(11)
    P = 160
    problems = [random_problem(rng, k, ((184, 232), (232, 232))[(k // 2) % 2]) for k in range(P)]
    shapes = [((184, 232), (232, 232))[(k // 2) % 2] for k in range(P)]
    host = [prefilled(rng, s) for s in shapes]
    overs = [torch.from_numpy(o.copy()).cuda() for o, _ in host]
    occs = [torch.from_numpy(c.copy()).cuda() for _, c in host]
    simq.observation_update([p[0] for p in problems], [p[1] for p in problems], [sim_geometry(ob, p[2]) for p in problems],
                            [sim_ranges(ob, p[3]) for p in problems], overs, occs)
    n_ambiguous = n_border = n_kept = 0
    for k, ((buffer, ids, g, r), (over, occ)) in enumerate(zip(problems, host)):
        assert oracle.update(over, occ, buffer, ids, g, r) == 0
        got_over, got_occ = overs[k].cpu().numpy(), occs[k].cpu().numpy()
        assert np.array_equal(bits(got_over), bits(over)), k
        assert np.array_equal(got_occ, occ), k
        written, ambiguous, _ = oracle.tied_pixels(over.shape, buffer, ids, g, r)
        assert np.all(got_over[~written] == F(-3.0))
        n_kept += int((~written).sum())
        n_ambiguous += int(ambiguous.sum())
        n_border += int(written[0].sum() + written[-1].sum() + written[:, 0].sum() + written[:, -1].sum())
        assert set(np.unique(got_occ).tolist()) <= {0, 1, 7}
    assert n_ambiguous > 1000 and n_border > 100 and n_kept > 100000


def test_uniform_launch_of_1024_problems_equals_the_oracle(S):
    simq, ob, torch = S
    rng = np.random.RandomState(12)
    P, shape = 1024, (232, 232)
    base = [random_problem(rng, 2 * k, shape) for k in range(16)]          # overhead frames; problem p takes frame p % 16 with its own ids
    depth = np.stack([base[p % 16][0] for p in range(P)])
    ids = np.stack([np.roll(base[p % 16][1], p // 16, axis=1) for p in range(P)])
    geoms = [sim_geometry(ob, b[2]) for b in base]
    over = torch.full((P,) + shape, -3.0, dtype=torch.float32, device='cuda')
    occ = torch.zeros((P,) + shape, dtype=torch.uint8, device='cuda')
    got = simq.observation_update(torch.from_numpy(depth).cuda(), ids, [geoms[p % 16] for p in range(P)], sim_ranges(ob, RANGES), over, occ)
    assert got[0] is over and got[1] is occ
    over, occ = over.cpu().numpy(), occ.cpu().numpy()
    for p in range(P):
        want_over, want_occ = np.full(shape, -3.0, F), np.zeros(shape, np.uint8)
        assert oracle.update(want_over, want_occ, depth[p], ids[p], base[p % 16][2], RANGES) == 0
        assert np.array_equal(bits(over[p]), bits(want_over)), p
        assert np.array_equal(occ[p], want_occ), p


def test_three_successive_launches_accumulate_as_the_reference_does(S, golden_dir):
    simq, ob, torch = S
    for fname in FILES:
        top, cases = oracle.load_fixture(os.path.join(golden_dir, fname))
        rec = dict(cases)
        steps = [rec['successive_step%d' % k] for k in range(3)]
        over = torch.from_numpy(steps[0]['overhead_before'].copy()).cuda()[None]
        occ = torch.from_numpy(steps[0]['occupancy_before'].copy()).cuda()[None]
        for s in steps:
            simq.observation_update(s['depth'][None], s['ids'][None], sim_geometry(ob, s['geometry']), sim_ranges(ob, s['ranges']), over, occ)
            assert np.array_equal(bits(over[0].cpu().numpy()), bits(s['overhead_after']))
            assert np.array_equal(occ[0].cpu().numpy(), s['occupancy_after'])
        assert (steps[2]['overhead_after'] != steps[0]['overhead_after']).any()


def test_two_problems_naming_one_map_are_refused_and_nothing_is_written(S):
    simq, ob, torch = S
    from simq._lib import SimqError
    rng = np.random.RandomState(13)
    a, b = random_problem(rng, 0, (184, 232)), random_problem(rng, 2, (184, 232))
    over = torch.full((2, 184, 232), -3.0, dtype=torch.float32, device='cuda')
    occ = torch.zeros((2, 184, 232), dtype=torch.uint8, device='cuda')
    for overs, occs in (([over[0], over[0]], [occ[0], occ[1]]), ([over[0], over[1]], [occ[1], occ[1]])):
        with pytest.raises(SimqError, match='share memory'):
            simq.observation_update([a[0], b[0]], [a[1], b[1]], [sim_geometry(ob, a[2]), sim_geometry(ob, b[2])], sim_ranges(ob, RANGES), overs, occs)
        torch.cuda.synchronize()
        assert bool((over == -3.0).all()) and not bool(occ.any())


def test_a_non_finite_frame_leaves_its_maps_and_its_neighbours_are_right(S):
    simq, ob, torch = S
    from simq._lib import SimqError
    rng = np.random.RandomState(14)
    shape = (232, 232)
    problems = [random_problem(rng, k, shape) for k in (0, 2, 1)]
    bad = problems[1][0].copy()
    bad[77, 5] = np.nan
    problems[1] = (bad,) + problems[1][1:]
    host = [prefilled(rng, shape) for _ in range(3)]
    over = torch.from_numpy(np.stack([h[0] for h in host])).cuda()
    occ = torch.from_numpy(np.stack([h[1] for h in host])).cuda()
    with pytest.raises(SimqError, match=r'not finite.*problems \[1\]'):
        simq.observation_update([p[0] for p in problems], [p[1] for p in problems], [sim_geometry(ob, p[2]) for p in problems],
                                sim_ranges(ob, RANGES), over, occ)
    for k, ((buffer, ids, g, _), (want_over, want_occ)) in enumerate(zip(problems, host)):
        assert oracle.update(want_over, want_occ, buffer, ids, g, RANGES) == (1 if k == 1 else 0)
        assert np.array_equal(bits(over[k].cpu().numpy()), bits(want_over)) and np.array_equal(occ[k].cpu().numpy(), want_occ)
    assert np.all(host[1][0] == F(-3.0))


def test_chain_into_occupancy_maps_on_the_device_resident_map(S, golden_dir):
    """observation_update -> simq.occupancy_maps on the occupancy map where it is: the configuration space, thin space and closest
    cells the oracle of the occupancy stage gives for the reference's own occupancy map."""
    simq, ob, torch = S
    for fname in FILES:
        top, cases = oracle.load_fixture(os.path.join(golden_dir, fname))
        picked = [(n, r) for n, r in cases if n in ('boxes_cubes', 'successive_step2', 'forward_wall', 'tie_receptacle_a')]
        assert len(picked) == 4
        occ = torch.from_numpy(np.stack([r['occupancy_before'] for _, r in picked])).cuda()
        over = torch.from_numpy(np.stack([r['overhead_before'] for _, r in picked])).cuda()
        simq.observation_update([r['depth'] for _, r in picked], [r['ids'] for _, r in picked], [sim_geometry(ob, r['geometry']) for _, r in picked],
                                [sim_ranges(ob, r['ranges']) for _, r in picked], over, occ)
        radius, thin = [int(x) for x in top['radius']]
        got = simq.occupancy_maps(occ, [top['room_mask']], radius, thin, room_index=[0] * 4)
        for k, (name, rec) in enumerate(picked):
            assert rec['occupancy_after'].any()
            cs, th, near = occupancy_maps_oracle.update(rec['occupancy_after'], top['room_mask'], radius, thin)
            assert np.array_equal(got.configuration_space[k].cpu().numpy(), cs), name
            assert np.array_equal(got.cspace_thin[k].cpu().numpy(), th), name
            assert np.array_equal(got.closest_cspace_indices[k].cpu().numpy(), near), name


def test_chain_into_local_state_images_with_the_updated_map_as_the_overhead_base(S, golden_dir):
    """observation_update -> simq.local_state_images('overhead') on the device tensor: channel 0 of the reference's get_state."""
    simq, ob, torch = S
    from simq.local_maps import RobotStamp
    n = 0
    for fname in FILES:
        top, cases = oracle.load_fixture(os.path.join(golden_dir, fname))
        picked = [(name, r) for name, r in cases if 'state0' in r and not name.startswith('tie_')]
        overs = [torch.from_numpy(r['overhead_before'].copy()).cuda() for _, r in picked]
        occs = [torch.from_numpy(r['occupancy_before'].copy()).cuda() for _, r in picked]
        simq.observation_update([r['depth'] for _, r in picked], [r['ids'] for _, r in picked], [sim_geometry(ob, r['geometry']) for _, r in picked],
                                [sim_ranges(ob, r['ranges']) for _, r in picked], overs, occs)
        poses = [((float(r['pose'][0]), float(r['pose'][1])), float(r['pose'][2])) for _, r in picked]
        robots = [[RobotStamp(pose[0], pose[1], 0, float(top['robot_seg_value']))] for pose in poses]
        states = simq.local_state_images(overs, [[('overhead', k)] for k in range(len(picked))], poses, robots=robots, masks=top['robot_mask'][None])
        for k, (name, r) in enumerate(picked):
            assert np.array_equal(bits(states[k, :, :, 0].cpu().numpy()), bits(r['state0'])), name
            n += 1
    assert n >= 20
