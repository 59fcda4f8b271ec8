"""GPU: simq.BatchedMapper (update + get_states of many Mapper / OccupancyMap pairs as one chain on the device) against the reference
Mapper's own rounds (tests/golden/mapper_*.npz), bit for bit; against the chain of the public functions written by hand
(tests/mapper_chain.py), stage by stage; and simq_grid_distance_images_snapped, the device-side snap that joins the occupancy maps to
the distance images, on its own."""
import glob
import os

import numpy as np
import pytest
import torch

import mapper_oracle as oracle
from grid_paths_oracle import distance_image, mapper_image
from mapper_chain import Chain

pytestmark = pytest.mark.gpu

CONFIGS = oracle.configurations()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(host(a) if isinstance(a, torch.Tensor) else a).view(np.int32)


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


@pytest.fixture(scope='module')
def episodes(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))
    assert len(files) == 2, files
    return [oracle.load_fixture(f) for f in files]


def build(simq_mod, episodes, cfg, envs=(0, 1)):
    """One object for the named episodes (one environment each)."""
    fx = [episodes[e] for e in envs]
    masks = {name: fx[0]['masks'][k] for k, name in enumerate(fx[0]['mask_names'])}
    flags = {f: cfg[f] for f in oracle.FLAGS}
    rest = {k: v for k, v in cfg.items() if k not in oracle.FLAGS}
    return simq_mod.BatchedMapper([f['room_width'] for f in fx], [f['room_length'] for f in fx], [f['types'] for f in fx], masks,
                                  [f['groups'] for f in fx], [f['receptacle_position'] for f in fx], **flags, **rest)


def frames_of(simq_mod, rnds):
    """(depth, ids, geometries, id_ranges) of the rounds' frames, one after the other, as simq.observation_update takes them."""
    from simq.observation import CameraGeometry, IdRanges
    depth, ids, geoms, ranges = [], [], [], []
    for rnd in rnds:
        for f in rnd['frames']:
            depth.append(f['depth'])
            ids.append(f['ids'])
            geoms.append(CameraGeometry(*f['geometry']))
            ranges.append(IdRanges(*f['ranges']))
    return depth, ids, geoms, ranges


def states_of(simq_mod, rnds):
    return [[simq_mod.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'], r['history_path'])
             for r in rnd['robots']] for rnd in rnds]


def pick(frames, mappers):
    return tuple([part[m] for m in mappers] for part in frames)


def expected(cfg, episodes, t, mappers):
    return np.stack([oracle.expected_state(cfg, episodes[m // 3]['rounds'][t]['images'], m % 3, 3) for m in mappers])


# ---- 1: both fixtures in one object, round by round, against the golden -------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_both_episodes_in_one_object_equal_the_reference_round_by_round(simq_mod, episodes, name):
    cfg = CONFIGS[name]
    bm = build(simq_mod, episodes, cfg)
    assert (bm.num_envs, bm.num_mappers) == (2, 6) and bm.shapes == [(184, 232)] * 3 + [(232, 232)] * 3 and not bm.uniform
    assert bm.channels == oracle.channel_names(cfg, 3)
    shuffled = [4, 1, 5, 0]
    for t in range(len(episodes[0]['rounds'])):
        rnds = [ep['rounds'][t] for ep in episodes]
        frames, robots = frames_of(simq_mod, rnds), states_of(simq_mod, rnds)
        if t == 1:                                                  # the same update in two calls over shuffled subsets
            bm.update(*pick(frames, shuffled), mappers=shuffled)
            bm.update(*pick(frames, [3, 2]), mappers=[3, 2])
        else:
            bm.update(*frames)
        got = bm.get_states(robots)
        assert got.dtype == torch.float32 and tuple(got.shape) == (6, 96, 96, len(bm.channels)) and got.is_contiguous()
        want = expected(cfg, episodes, t, range(6))
        for m in range(6):
            for c, channel in enumerate(bm.channels):
                assert np.array_equal(bits(got[m, :, :, c]), bits(want[m, :, :, c])), (name, t, m, channel)
        sub = bm.get_states(robots, mappers=shuffled)
        assert np.array_equal(bits(sub), bits(expected(cfg, episodes, t, shuffled))), (name, t)


# ---- 2: the hand-written chain of the public functions, stage by stage ----------------------------------------------------------------
@pytest.mark.parametrize('name', ['full_spatial', 'full_nonspatial'])
def test_every_stage_equals_the_hand_written_chain_of_the_public_functions(simq_mod, episodes, name):
    cfg = CONFIGS[name]
    bm = build(simq_mod, episodes, cfg)
    chains = [Chain(simq_mod, ep['room_width'], ep['room_length'], [ep['types']], ep['masks'], ep['mask_names'], ep['receptacle_position'])
              for ep in episodes]
    for t in range(2):
        rnds = [ep['rounds'][t] for ep in episodes]
        bm.update(*frames_of(simq_mod, rnds))
        got = bm.get_states(states_of(simq_mod, rnds))
        for e, (chain, rnd) in enumerate(zip(chains, rnds)):
            chain.update(*frames_of(simq_mod, [rnd]))
            want = chain.get_states(cfg, [rnd['robots']])
            for r in range(3):
                m, tag = 3 * e + r, (name, t, e, r)
                assert np.array_equal(bits(bm.overhead[m]), bits(chain.overhead[r])), tag
                assert np.array_equal(host(bm.occupancy[m]), host(chain.occupancy[r])), tag
                assert np.array_equal(host(bm.room_masks[m]), chain.room_mask), tag
                assert np.array_equal(host(bm.configuration_space[m]), host(chain.cspace[r])), tag
                assert np.array_equal(host(bm.cspace_thin[m]), host(chain.thin[r])), tag
                assert np.array_equal(host(bm.closest_cspace_indices[m]), host(chain.closest[r])), tag
                for d in range(2):
                    assert np.array_equal(bits(bm.stage_maps[('image', d, m)]), bits(want['images'][d * 3 + r])), tag + (d,)
                assert np.array_equal(bits(bm.stage_maps[('history', m)]), bits(want['history'][r])), tag
                assert np.array_equal(bits(bm.stage_maps[('intention', m)]), bits(want['intention'][r])), tag
                if name == 'full_spatial':
                    for q in range(2):
                        assert np.array_equal(bits(bm.stage_maps[('channel', m, q)]), bits(want['channels'][2 * r + q])), tag + (q,)
                assert np.array_equal(bits(got[m]), bits(want['states'][r])), tag
            assert np.array_equal(bits(bm.distance_to_receptacle_maps[e]), bits(chain.receptacle_map))
    assert host(bm.occupancy_status).tolist() == [0] * 6


# ---- 3: the snapped entry on its own -----------------------------------------------------------------------------------------------
def snap_grids():
    """Three grids (8 x 9, 40 x 33, 184 x 232) with obstacles, their closest free cells, and per grid sources that are free already, on
    an occupied cell (the snap moves them) and on the border."""
    from occupancy_maps_oracle import closest_free
    rng = np.random.RandomState(7)
    out = []
    for R, C in ((8, 9), (40, 33), (184, 232)):
        g = np.zeros((R, C), np.uint8)
        g[1:R - 1, 1:C - 1] = 1
        for _ in range(3 + R // 8):
            i, j = rng.randint(1, R - 2), rng.randint(1, C - 2)
            g[i:i + max(2, R // 10), j:j + max(2, C // 12)] = 0
        g[R // 2, 1:C - 1] = 1                                      # (one free row keeps the free cells connected enough to be interesting)
        closest = closest_free(g)
        free, blocked = np.argwhere(g != 0), np.argwhere(g[1:R - 1, 1:C - 1] == 0) + 1
        srcs = [tuple(free[rng.randint(len(free))]), tuple(free[0]), tuple(blocked[rng.randint(len(blocked))]), tuple(blocked[-1]),
                (0, 0), (R - 1, C - 1), (0, C // 2), (R // 2, 0)]
        out.append((g, closest, [(int(i), int(j)) for i, j in srcs]))
    return out


def test_snapped_entry_equals_the_host_snapped_images_in_one_mixed_launch(simq_mod):
    from simq import _lib, grid_paths
    cases = snap_grids()
    grids, closest = [g for g, _, _ in cases], [c for _, c, _ in cases]
    sources, index = [], []
    for k, (g, c, srcs) in enumerate(cases):
        sources += srcs
        index += [k] * len(srcs)
    snapped = [(int(closest[k][0, i, j]), int(closest[k][1, i, j])) for k, (i, j) in zip(index, sources)]
    moved = sum(s != p for s, p in zip(snapped, sources))
    assert moved >= 12 and any(grids[k][i, j] == 0 for k, (i, j) in zip(index, sources)) and all(grids[k][i, j] != 0 for k, (i, j) in zip(index, snapped))
    _lib.lib.c.simq_launch_counts_reset()
    kw = dict(pixels_per_meter=96.0, unreachable_to_max=True, scale=0.25, grid_index=index)
    got = simq_mod.grid_distance_images(grids, sources, closest=closest, **kw)
    assert _lib.launch_counts() == {'grid_distance_snapped': 1}
    want = simq_mod.grid_distance_images(grids, snapped, **kw)
    assert len(got) == len(want) == len(sources)
    for p, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape == grids[index[p]].shape and np.array_equal(bits(a), bits(b)), (p, sources[p])
        if p % 8 in (0, 2):                                         # and the numpy oracle on a free and on a moved source of every grid
            assert np.array_equal(bits(a), bits(mapper_image(distance_image(grids[index[p]], snapped[p]), 96.0, 0.25))), p
    # without the epilogue, device tensors read in place: one [G, rows, cols] tensor and one [G, 2, rows, cols] tensor
    g2, c2 = torch.from_numpy(np.stack([grids[2]] * 2)).cuda(), torch.from_numpy(np.stack([closest[2]] * 2)).cuda()
    plain = simq_mod.grid_distance_images(g2, cases[2][2][:4], grid_index=[0, 1, 1, 0], closest=c2)
    assert tuple(plain.shape) == (4, 184, 232)
    for p in range(4):
        assert np.array_equal(bits(plain[p]), bits(distance_image(grids[2], snapped[16 + p]))), p


def test_snapped_entry_status_codes_fill_and_neighbours(simq_mod):
    """A closest pair that names no cell of its grid, or an occupied one, is status 3; an upstream word is passed on; both images hold the
    fill, the problems around them are right, and the public function raises in the operator's words."""
    from simq import grid_paths
    from simq._lib import SimqError
    cases = snap_grids()
    g, closest, srcs = cases[1]
    bad = closest.copy()
    bad[:, srcs[2][0], srcs[2][1]] = (40, 3)                        # row 40 of a 40-row grid
    bad[:, srcs[3][0], srcs[3][1]] = (-1, -1)                       # what a configuration space without a free cell leaves
    bad[:, srcs[4][0], srcs[4][1]] = np.argwhere(g == 0)[5]         # inside the grid, on an occupied cell
    upstream = torch.tensor([0, 1, 0, 7], dtype=torch.int32, device='cuda')
    sources = srcs[:6] + [srcs[0], srcs[1]]
    out, status, uniform, shapes, entry = grid_paths._enqueue([g, cases[0][0]], sources + [cases[0][2][0]], 96.0, True, 0.25, None, [0] * 8 + [1],
                                                              [bad, cases[0][1]], None, upstream, [0, 2, 0, 0, 2, 0, 1, 3, 0])
    assert entry == 'simq_grid_distance_images_snapped' and not uniform
    images = [host(v) for v in __import__('simq')._batch.views(out.view(-1), shapes)]
    assert host(status).tolist() == [0, 0, 3, 3, 3, 0, 1, 7, 0]
    for p in (2, 3, 4, 6, 7):
        assert np.array_equal(bits(images[p]), bits(np.full(g.shape, grid_paths.SNAPPED_FILL, np.float32))), p
    for p in (0, 1, 5):
        src = (int(closest[0][sources[p]]), int(closest[1][sources[p]]))
        assert np.array_equal(bits(images[p]), bits(mapper_image(distance_image(g, src), 96.0, 0.25))), p
    src = cases[0][2][0]
    assert np.array_equal(bits(images[8]), bits(mapper_image(distance_image(cases[0][0], (int(cases[0][1][0][src]), int(cases[0][1][1][src]))), 96.0, 0.25)))
    with pytest.raises(SimqError, match=r'simq_grid_distance_images_snapped: the closest cell of 3 source\(s\) is no free cell of their grid '
                                        r'\(status 3 at problems \[2, 3, 4\]\)'):
        simq_mod.grid_distance_images([g], sources[:6], grid_index=[0] * 6, closest=[bad])
    # the library refuses a descriptor before it launches anything: a source outside the grid, overlapping buffers
    with pytest.raises(SimqError, match=r'problem 0: source \(40, 0\) outside its 40 x 33 grid'):
        simq_mod.grid_distance_images([g], [(40, 0)], closest=[closest])
    both = torch.zeros(2 * g.size, dtype=torch.float32, device='cuda')
    as_grid = both.view(torch.uint8)[:g.size].view(g.shape)
    with pytest.raises(SimqError, match='d_out overlaps d_grids'):
        simq_mod.grid_distance_images([as_grid], [(1, 1)], closest=torch.from_numpy(closest).cuda()[None], out=both[:g.size].view((1,) + g.shape))


def test_snapped_entry_64_problems_sharing_4_grids(simq_mod):
    from occupancy_maps_oracle import closest_free
    rng = np.random.RandomState(11)
    grids = []
    for k in range(4):
        g = (rng.rand(40, 33) > 0.3).astype(np.uint8)
        g[0, :] = g[-1, :] = 0
        grids.append(g)
    closest = np.stack([closest_free(g) for g in grids])
    index = [int(k) for k in rng.randint(0, 4, 64)]
    sources = [(int(rng.randint(40)), int(rng.randint(33))) for _ in index]
    d_grids, d_closest = torch.from_numpy(np.stack(grids)).cuda(), torch.from_numpy(closest).cuda()
    out = torch.full((64, 40, 33), -7.0, device='cuda')
    got = simq_mod.grid_distance_images(d_grids, sources, grid_index=index, closest=d_closest, out=out)
    assert got is out
    memo = {}
    for p, (k, (i, j)) in enumerate(zip(index, sources)):
        src = (k, int(closest[k, 0, i, j]), int(closest[k, 1, i, j]))
        if src not in memo:
            memo[src] = distance_image(grids[k], src[1:])
        assert np.array_equal(bits(got[p]), bits(memo[src])), (p, k, i, j)


# ---- 4: out= is a slice of a dirty ring -------------------------------------------------------------------------------------------
def test_out_is_a_slice_of_a_dirty_ring(simq_mod, episodes):
    cfg = CONFIGS['full_spatial']
    bm = build(simq_mod, episodes, cfg)
    rnds = [ep['rounds'][0] for ep in episodes]
    bm.update(*frames_of(simq_mod, rnds))
    C = len(bm.channels)
    ring = torch.full((10, 96, 96, C), float('nan'), device='cuda')
    ring.view(torch.int32).fill_(0x7FC0BEEF)                        # a NaN with a payload: any element left unwritten shows
    got = bm.get_states(states_of(simq_mod, rnds), out=ring[2:8])
    assert got.data_ptr() == ring[2:8].data_ptr()
    assert np.array_equal(bits(ring[2:8]), bits(expected(cfg, episodes, 0, range(6))))
    assert (bits(ring[:2]) == 0x7FC0BEEF).all() and (bits(ring[8:]) == 0x7FC0BEEF).all()
    with pytest.raises(ValueError, match='out must be a contiguous float32 device tensor'):
        bm.get_states(states_of(simq_mod, rnds), out=ring[:, :, :, :C - 1])


# ---- 5: launches and read-backs do not grow with the mappers -----------------------------------------------------------------------
def test_launch_and_read_back_counts(simq_mod, episodes, monkeypatch):
    from simq import _batch, _lib
    cfg = CONFIGS['full_spatial']
    counts = {}
    real = _batch.bad_problems
    calls = []
    monkeypatch.setattr(_batch, 'bad_problems', lambda *a, **k: calls.append(1) or real(*a, **k))
    ep = episodes[0]
    for envs in ((0,), (0, 0)):                                     # M = 3 and M = 6 in one room; M = 1 is the object of three, one named
        bm = build(simq_mod, episodes, cfg, envs)
        rnds = [ep['rounds'][0]] * len(envs)
        frames, robots = frames_of(simq_mod, rnds), states_of(simq_mod, rnds)
        for mappers in ([1], None):
            M = 1 if mappers else bm.num_mappers
            use = pick(frames, mappers) if mappers else frames
            _lib.lib.c.simq_launch_counts_reset()
            del calls[:]
            bm.update(*use, mappers=mappers)
            assert len(calls) == 1, (M, 'update')
            after_update = _lib.launch_counts()
            bm.get_states(robots, mappers=mappers)
            assert len(calls) == 2, (M, 'get_states')
            counts[M] = (after_update, _lib.launch_counts())
    assert sorted(counts) == [1, 3, 6]
    assert counts[1][0] == counts[3][0] == counts[6][0] == {'observation_maps': 1, 'occupancy_maps': 1}
    assert counts[1][1] == counts[3][1] == counts[6][1]
    assert counts[6][1] == {'observation_maps': 1, 'occupancy_maps': 1, 'grid_distance_snapped': 1, 'intention_maps': 1, 'local_state': 1}


# ---- 6: a mapper whose room is fully occupied -------------------------------------------------------------------------------------
def test_a_fully_occupied_room_is_a_status_that_names_its_mapper(simq_mod, episodes):
    from simq._lib import SimqError
    cfg = CONFIGS['full_spatial']
    bm = build(simq_mod, episodes, cfg)
    rnds = [ep['rounds'][0] for ep in episodes]
    frames, robots = frames_of(simq_mod, rnds), states_of(simq_mod, rnds)
    bm.occupancy[4].fill_(1)                                        # every cell of the room an obstacle: no free cell is left
    with pytest.raises(SimqError, match=r'simq_occupancy_maps: mapper\(s\) 4 \(environment 1, robot 1\) have a configuration space without a free cell'):
        bm.update(*frames)
    assert host(bm.occupancy_status).tolist() == [0, 0, 0, 0, 1, 0]
    assert not host(bm.configuration_space[4]).any()
    # every other mapper was updated, and its next states are right
    good = [0, 1, 2, 3, 5]
    states = bm.get_states(robots, mappers=good)
    assert np.array_equal(bits(states), bits(expected(cfg, episodes, 0, good)))
    # the mapper itself is reported, after the chain has run: its distance channels come from the fill, the others' states are right
    out = torch.full((6, 96, 96, len(bm.channels)), 5.0, device='cuda')
    with pytest.raises(SimqError, match=r'no distance images for mapper\(s\) 4 \(environment 1, robot 1\)'):
        bm.get_states(robots, out=out)
    want = expected(cfg, episodes, 0, range(6))
    for m in good:
        assert np.array_equal(bits(out[m]), bits(want[m])), m
    for c in (3, 4):
        assert bm.channels[c].startswith('shortest_path') and not host(out[4, :, :, c]).any()
    # before any update every mapper is refused in the same way
    fresh = build(simq_mod, episodes, cfg)
    with pytest.raises(SimqError, match=r'status \[4, 4, 4, 4, 4, 4, 4, 4\]'):
        fresh.get_states(robots)


# ---- 7: reset of one environment ----------------------------------------------------------------------------------------------------
def test_reset_of_one_environment_leaves_the_other_bit_identical(simq_mod, episodes):
    cfg = CONFIGS['full_nonspatial']
    bm = build(simq_mod, episodes, cfg)
    for t in range(2):
        rnds = [ep['rounds'][t] for ep in episodes]
        bm.update(*frames_of(simq_mod, rnds))
    robots = states_of(simq_mod, rnds)
    kinds = ('overhead', 'occupancy', 'configuration_space', 'cspace_thin', 'closest_cspace_indices')
    before = {k: [host(t).copy() for t in getattr(bm, k)] for k in kinds}
    states = host(bm.get_states(robots)).copy()
    assert all(before[k][m].any() for k in kinds for m in range(6))
    bm.reset([0])
    for k in kinds:
        for m in range(6):
            now = host(getattr(bm, k)[m])
            assert np.array_equal(now, before[k][m]) if m >= 3 else not now.any(), (k, m)
    assert host(bm.occupancy_status).tolist() == [4, 4, 4, 0, 0, 0]
    assert np.array_equal(host(bm.room_masks[0]), oracle.room_mask(0.5, 1.0))
    assert np.array_equal(bits(bm.get_states(robots, mappers=[3, 4, 5])), bits(states[3:]))
    # the reset environment starts its episode over: round 0 alone gives round 0's states
    rnds0 = [ep['rounds'][0] for ep in episodes]
    frames = frames_of(simq_mod, rnds0)
    bm.update(*pick(frames, [0, 1, 2]), mappers=[0, 1, 2])
    got = bm.get_states([states_of(simq_mod, rnds0)[0], robots[1]])
    assert np.array_equal(bits(got[:3]), bits(expected(cfg, episodes, 0, range(3)))) and np.array_equal(bits(got[3:]), bits(states[3:]))


# ---- 8: grid_distance_images without closest= is what it was --------------------------------------------------------------------
def test_grid_distance_images_without_closest_is_unchanged(simq_mod, golden_dir):
    """The fixtures of the existing distance-image test, through the wrapper as it was called before it had closest=: the same entry
    point, one launch, the same bits; one mixed-shape call over every grid of a file as well."""
    from simq import _lib
    n = 0
    for f in sorted(glob.glob(os.path.join(golden_dir, 'grid_paths_*.npz'))):
        z = np.load(f)
        grids, sources, index, want = [], [], [], []
        for k, name in enumerate(str(x) for x in z['names']):
            grids.append(z['grid_' + name])
            _lib.lib.c.simq_launch_counts_reset()
            got = simq_mod.grid_distance_images([grids[k]], [tuple(s) for s in z['src_' + name]], grid_index=[0] * len(z['src_' + name]))
            assert _lib.launch_counts() == {'grid_distance': 1}
            assert np.array_equal(bits(got), bits(z['dist_' + name])), name
            sources += [tuple(int(x) for x in s) for s in z['src_' + name]]
            index += [k] * len(z['src_' + name])
            want += list(z['dist_' + name])
        got = simq_mod.grid_distance_images(grids, sources, grid_index=index)
        for p in range(len(sources)):
            assert np.array_equal(bits(got[p]), bits(want[p])), (f, p)
        n += len(sources)
    assert n >= 25


# ---- the thin delegates ------------------------------------------------------------------------------------------------------------
def test_shortest_paths_and_distances_to_receptacle_delegate_to_the_stored_tensors(simq_mod, episodes):
    cfg = CONFIGS['full_spatial']
    bm = build(simq_mod, episodes, cfg, (0, 0))                     # one room: the delegates take [M, rows, cols] tensors
    rnds = [episodes[0]['rounds'][0]] * 2
    bm.update(*frames_of(simq_mod, rnds))
    assert bm.uniform and tuple(bm.configuration_space.shape) == (6, 184, 232)
    sources = [r['position'] for r in rnds[0]['robots']]
    targets = [(-0.35, -0.15), (0.35, 0.1), (0.0, 0.0)]
    keep_all = lambda coords, tolerance: coords                     # (scikit-image's simplifier is not what is under test)
    got = bm.shortest_paths(sources, targets, mappers=[3, 4, 5], simplify=keep_all)
    want = simq_mod.shortest_paths(bm.configuration_space, bm.cspace_thin, bm.closest_cspace_indices, sources, targets, [3, 4, 5], keep_all)
    assert got == want and len(got) == 3
    d = bm.distances_to_receptacle([targets, targets[:1]], mappers=[5, 0])
    w = simq_mod.distances_to_receptacle(bm.configuration_space, bm.closest_cspace_indices, [episodes[0]['receptacle_position']] * 2,
                                         [targets, targets[:1]], [5, 0])
    assert all(np.array_equal(a, b) for a, b in zip(d, w)) and [len(a) for a in d] == [3, 1]
