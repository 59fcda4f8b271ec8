"""GPU: simq_local_state_images / simq.local_state_images against the reference Mapper's own images (tests/golden/local_maps_*.npz) and
the numpy oracle (tests/local_maps_oracle.py), bit for bit (compared as int32 bit patterns)."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest
import torch

import local_maps_oracle as oracle
from grid_paths_oracle import distance_image, mapper_image

pytestmark = pytest.mark.gpu

SENTINEL = 123.0


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'local_maps_*.npz')))
    assert len(files) == 2, files
    return [(os.path.basename(f), oracle.load_fixture(f)) for f in files]


def assert_states_equal(got, want, channels, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for p in range(got.shape[0]):
        for c in range(got.shape[3]):
            bad = int((got[p, :, :, c] != want[p, :, :, c]).sum())
            assert bad == 0, '%s: problem %d channel %d %r: %d of 9216 pixels differ' % (what, p, c, channels[p][c], bad)


def fixture_inputs(fx):
    """poses and per-problem robot lists (one list object per environment) of a fixture for simq.local_state_images."""
    from simq.local_maps import RobotStamp
    envs = {e: [RobotStamp(*r) for r in robots] for e, robots in fx['robot_poses'].items()}
    return [(s['position'], s['heading']) for s in fx['states']], [envs[s['env']] for s in fx['states']]


def test_every_fixture_through_the_python_interface(simq_mod, golden_dir):
    n = 0
    for name, fx in fixtures(golden_dir):
        poses, robots = fixture_inputs(fx)
        got = simq_mod.local_state_images(torch.from_numpy(fx['maps']).cuda(), fx['channels'], poses, robots=robots, masks=fx['masks'])
        assert got.dtype == torch.float32 and tuple(got.shape) == fx['want'].shape and got.is_cuda
        assert_states_equal(got, fx['want'], [fx['channels']] * len(poses), name)
        # numpy maps are uploaded, a device mask bank is taken as it is: the same result
        again = simq_mod.local_state_images(list(fx['maps']), fx['channels'], poses, robots=robots, masks=torch.from_numpy(fx['masks']).cuda())
        assert np.array_equal(bits(again), bits(got))
        n += got.shape[0] * got.shape[3]
    assert n >= 40


def rotation_struct(lm, rot):
    R, off, shape = rot
    return lm.Rotation((ctypes.c_double * 4)(*np.asarray(R, np.float64).reshape(-1)), (ctypes.c_double * 2)(*off),
                       (ctypes.c_int32 * 2)(int(shape[0]), int(shape[1])))


def test_every_fixture_through_the_c_abi_with_the_stored_doubles(simq_mod, golden_dir):
    """No scipy on this path: the rotation matrices, offsets and shapes are the float64 values the fixture stores."""
    from simq import _lib, local_maps as lm
    for name, fx in fixtures(golden_dir):
        maps = torch.from_numpy(fx['maps']).cuda()
        masks = torch.from_numpy(fx['masks']).cuda()
        G, rows, cols = maps.shape
        c_maps = (lm.LocalMap * G)(*[lm.LocalMap(maps[k].data_ptr(), rows, cols) for k in range(G)])
        robots, begin = [], {}
        for e, env in sorted(fx['robots'].items()):
            begin[e] = (len(robots), len(env))
            for pixel, rot, mask, seg, val, seg_mask in env:
                robots.append(lm.LocalRobot(rotation_struct(lm, rot), pixel[0], pixel[1], mask, seg, val, seg_mask))
        c_robots = (lm.LocalRobot * len(robots))(*robots)
        P, C = len(fx['states']), len(fx['channels'])
        c_probs = (lm.LocalProblem * P)(*[lm.LocalProblem(rotation_struct(lm, s['rot']), s['pixel'][0], s['pixel'][1], rows, cols, *begin[s['env']])
                                          for s in fx['states']])
        chans = []
        for spec in fx['channels']:
            kind = spec if isinstance(spec, str) else spec[0]
            chans.append(lm.LocalChannel(lm.KINDS[kind], spec[1] if kind in ('map', 'distance', 'overhead') else 0,
                                         spec[1] if kind == 'constant' else 0.0, 0))
        c_chans = (lm.LocalChannel * (P * C))(*(chans * P))
        need = _lib.lib.c.simq_local_state_desc_bytes(G, len(robots), P, C)
        desc = torch.empty(need, dtype=torch.uint8, device='cuda')
        out = torch.full((P, 96, 96, C), SENTINEL, device='cuda')
        _lib.lib.c.simq_launch_counts_reset()
        _lib.lib.call('simq_local_state_images', c_maps, G, _lib.ptr(masks), masks.shape[0], c_robots, len(robots), c_probs, P, c_chans, C,
                      _lib.ptr(desc), ctypes.c_int64(need), _lib.ptr(out), ctypes.c_int64(out.numel()), _lib.stream_ptr())
        assert _lib.lib.c.simq_launch_count(b'local_state') == 1                       # one launch for all problems
        assert_states_equal(out, fx['want'], [fx['channels']] * P, name)


def random_batch(rng, masks, n_envs, C, robots_per_env=None):
    """Environments of 1-4 robots on mixed map shapes, each robot one problem; every channel kind among the C channels (when C allows)."""
    from simq.local_maps import RobotStamp
    maps, poses, robots, channels, meta = [], [], [], [], []
    for e in range(n_envs):
        rows, cols = [(184, 232), (232, 232), (136, 136), (150, 301)][e % 4]
        base = len(maps)
        maps += [(rng.rand(rows, cols) * 4 - 1).astype(np.float32), (rng.rand(rows, cols) * 2).astype(np.float32),
                 (rng.rand(rows, cols) * 0.5).astype(np.float32)]
        nr = robots_per_env or 1 + e % 4
        env, stamps = [], []
        for r in range(nr):
            px = (int(rng.randint(68, rows - 68 + 1)), int(rng.randint(68, cols - 68 + 1)))
            position = ((px[1] + rng.uniform(0.05, 0.95) - cols / 2) / 96.0, (rows / 2 - px[0] - rng.uniform(0.05, 0.95)) / 96.0)
            heading = rng.choice([0.0, math.pi / 2, -math.pi / 2, math.pi, math.pi / 4, -3 * math.pi / 4, math.pi / 6]) if rng.rand() < 0.2 \
                else rng.uniform(-math.pi, math.pi)
            mask, seg_mask = int(rng.randint(len(masks))), int(rng.randint(len(masks)))
            seg, val = float(rng.randint(5, 9)) / 8, float(rng.choice([0.5, 1.0]))
            env.append(RobotStamp(position, float(heading), mask, seg, val, seg_mask))
            assert oracle.position_to_pixel_indices(position[0], position[1], (rows, cols)) == px
            stamps.append((px, oracle.mask_rotation(float(heading)), mask, seg, val, seg_mask))
        menu = [('map', base), ('distance', base + 1), ('overhead', base + 2), 'robots', ('constant', float(rng.randn())), ('distance', base),
                ('map', base + 2), 'robots', ('overhead', base + 1), ('constant', -1.5)]
        for r in range(nr):
            chans = [menu[(r + e + k) % len(menu)] for k in range(C)]
            poses.append((env[r].position, env[r].heading))
            robots.append(env)
            channels.append(chans)
            meta.append((stamps[r][0], float(env[r].heading), stamps, (rows, cols)))
    return maps, poses, robots, channels, meta


def oracle_states(maps, channels, meta, masks):
    return np.stack([oracle.state(maps, chans, px, oracle.crop_rotation(h), stamps, masks, map_shape=shape)
                     for chans, (px, h, stamps, shape) in zip(channels, meta)])


def test_random_problems_in_one_launch_against_the_oracle(simq_mod, golden_dir):
    """>= 200 problems of mixed shapes, robots and channel kinds in one launch.  Random headings put the centre of the even-sized rotated
    image within an ulp of x.5, where a contracted or reordered coordinate picks the neighbouring pixel: such a kernel fails here."""
    from simq import _lib
    masks = oracle.load_fixture(os.path.join(golden_dir, 'local_maps_184x232.npz'))['masks']
    rng = np.random.RandomState(77)
    maps, poses, robots, channels, meta = random_batch(rng, masks, 84, 10)
    assert len(poses) >= 200
    # the set tells the evaluation orders apart: on a map whose pixels are all distinct, the order (offset + oi * R0) + oj * R1 picks
    # another pixel than the reference's order in some of these problems
    moved = 0
    for px, h, _, shape in meta:
        ident = np.arange(shape[0] * shape[1], dtype=np.float32).reshape(shape)
        rot = oracle.crop_rotation(h)
        moved += int((oracle.local_map(ident, px, rot) != oracle.local_map(ident, px, rot, offset_first=True)).sum())
    assert moved >= 1
    d_maps = [torch.from_numpy(m).cuda() for m in maps]
    _lib.lib.c.simq_launch_counts_reset()
    got = simq_mod.local_state_images(d_maps, channels, poses, robots=robots, masks=masks)
    assert _lib.lib.c.simq_launch_count(b'local_state') == 1
    assert_states_equal(got, oracle_states(maps, channels, meta, masks), channels, 'random C = 10')
    for C in range(1, 10):
        maps, poses, robots, channels, meta = random_batch(rng, masks, 4, C)
        got = simq_mod.local_state_images(maps, channels, poses, robots=robots, masks=masks, map_shape=[m[3] for m in meta])
        assert_states_equal(got, oracle_states(maps, channels, meta, masks), channels, 'random C = %d' % C)


def test_channels_without_a_map_take_the_shape_from_map_shape(simq_mod, golden_dir):
    fx = oracle.load_fixture(os.path.join(golden_dir, 'local_maps_232x232.npz'))
    poses, robots = fixture_inputs(fx)
    s = fx['states'][0]
    got = simq_mod.local_state_images([], ['robots', ('constant', 2.5)], poses[:1], robots=robots[:1], masks=fx['masks'], map_shape=(232, 232))
    want = oracle.state([], ['robots', ('constant', 2.5)], s['pixel'], s['rot'], fx['robots'][s['env']], fx['masks'], map_shape=(232, 232))
    assert np.array_equal(bits(got[0]), bits(want)) and float(got[0, :, :, 0].max()) > 0


def test_distance_images_chain_into_states_on_the_device(simq_mod):
    """grid_distance_images with the Mapper epilogue -> 'distance' channels, the tensor handed over as it is (no host copy between the
    two launches), equals oracle(mapper_image(distance_image(...))) of tests/grid_paths_oracle.py."""
    rng = np.random.RandomState(9)
    scale = 0.25
    for rows, cols, room in ((184, 232, (44, 92)), (232, 232, (92, 92))):
        grid = np.zeros((rows, cols), np.uint8)
        i0, j0 = rows // 2 - room[0] // 2, cols // 2 - room[1] // 2
        grid[i0:i0 + room[0], j0:j0 + room[1]] = 1
        for _ in range(4):
            i, j = i0 + rng.randint(room[0] - 6), j0 + rng.randint(room[1] - 6)
            grid[i:i + 6, j:j + 6] = 0
        ii, jj = np.nonzero(grid)
        picks = rng.choice(ii.size, 4, replace=False)
        srcs = [(int(ii[k]), int(jj[k])) for k in picks]
        headings = [0.0, math.pi / 4] + list(rng.uniform(-math.pi, math.pi, 2))
        # robot k stands at source k: position of that pixel's centre
        poses = [(((j + 0.5 - cols / 2) / 96.0, (rows / 2 - i - 0.5) / 96.0), float(h)) for (i, j), h in zip(srcs, headings)]
        imgs = simq_mod.grid_distance_images([grid], srcs, grid_index=[0] * 4, pixels_per_meter=96, unreachable_to_max=True, scale=scale)
        assert imgs.is_cuda and tuple(imgs.shape) == (4, rows, cols)
        channels = [[('distance', k), ('distance', 0), ('map', k)] for k in range(4)]
        got = simq_mod.local_state_images(imgs, channels, poses)
        host = [mapper_image(distance_image(grid, s), 96.0, scale) for s in srcs]
        for k in range(4):
            assert oracle.position_to_pixel_indices(poses[k][0][0], poses[k][0][1], (rows, cols)) == srcs[k]
            want = oracle.state(host, channels[k], srcs[k], oracle.crop_rotation(poses[k][1]))
            assert np.array_equal(bits(got[k]), bits(want)), (rows, cols, k)
            assert float(got[k, :, :, 0].min()) == 0.0


def test_out_slice_of_a_ring_and_the_q_network_on_it(simq_mod, golden_dir):
    """out= a slice of a [capacity, 96, 96, C] tensor (DeviceReplayBuffer.states has this layout): only that slice is written, and the
    states feed FCN.infer_argmax_batch where they lie, giving the actions of the host-built states."""
    from simq import synth
    from oracle import fcn as ofcn
    fx = oracle.load_fixture(os.path.join(golden_dir, 'local_maps_184x232.npz'))
    sel = [0, 4, 9]
    all_poses, all_robots = fixture_inputs(fx)
    poses, robots = [all_poses[p] for p in sel], [all_robots[p] for p in sel]
    channels = [('overhead', 2), 'robots', ('distance', 1), ('map', 1)]                 # the 4-channel state of BASELINE configs[1]
    want = np.stack([oracle.state(fx['maps'], channels, fx['states'][p]['pixel'], fx['states'][p]['rot'], fx['robots'][fx['states'][p]['env']],
                                  fx['masks']) for p in sel])
    ring = torch.full((8, 96, 96, 4), SENTINEL, device='cuda')
    got = simq_mod.local_state_images(torch.from_numpy(fx['maps']).cuda(), channels, poses, robots=robots, masks=fx['masks'], out=ring[2:5])
    assert got.data_ptr() == ring[2].data_ptr()
    host = ring.cpu().numpy()
    assert np.array_equal(bits(host[2:5]), bits(want))
    assert (host[:2] == SENTINEL).all() and (host[5:] == SENTINEL).all()
    net = simq_mod.FCN(4, 2)
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(4, 2, 2)))
    net.eval()
    on_device, _ = net.infer_argmax_batch([ring[k:k + 1] for k in (2, 3, 4)])
    from_host, _ = net.infer_argmax_batch([want[k] for k in range(3)])
    assert on_device == from_host and all(0 <= a < 2 * 96 * 96 for a in on_device)


def test_each_validation_rule_raises_and_launches_nothing(simq_mod):
    from simq import _lib
    from simq.local_maps import RobotStamp
    SimqError = _lib.SimqError
    gm = torch.rand(184, 232, device='cuda')
    masks = np.ones((2, 96, 96), np.float32)
    out = torch.full((1, 96, 96, 2), SENTINEL, device='cuda')
    chans = [('map', 0), 'robots']
    centre = ((0.0, 0.0), 0.3)

    def refused(match, maps=None, channels=chans, pose=centre, robots=None, out_=None, masks_=masks):
        _lib.lib.c.simq_launch_counts_reset()
        with pytest.raises(SimqError, match=match):
            simq_mod.local_state_images([gm] if maps is None else maps, channels, [pose], robots=robots, masks=masks_,
                                        out=out if out_ is None else out_)
        torch.cuda.synchronize()
        assert _lib.lib.c.simq_launch_count(b'local_state') == 0
        assert bool((out == SENTINEL).all())

    # the crop leaves the map: pixel rows 67 / 117, pixel columns 67 / 165 (the reference would wrap or clip the slice silently)
    for pos in ((0.0, 0.255), (0.0, -0.265), (-0.505, 0.0), (0.515, 0.0), (3.0, 3.0)):
        refused('crop around pixel', pose=(pos, 0.0))
    # a robot whose stamp leaves the map
    refused('stamp of robot 0', robots=[[RobotStamp((0.0, 0.5), 0.0, 0, 0.625)]])
    refused('stamp of robot 1', robots=[[RobotStamp((0.0, 0.0), 0.0, 0, 0.625), RobotStamp((1.2, 0.0), 1.0, 0, 0.625)]])
    # indices
    refused('outside the bank', robots=[[RobotStamp((0.0, 0.0), 0.0, 2, 0.625)]])
    refused('outside the bank', robots=[[RobotStamp((0.0, 0.0), 0.0, 0, 0.625, 1.0, 5)]])
    # maps of another shape than the problem's; maps smaller than a crop
    refused('the problem\'s maps are', maps=[gm, torch.rand(232, 232, device='cuda')], channels=[('map', 0), ('map', 1)])
    refused('rows, cols >= 136', maps=[torch.rand(100, 232, device='cuda')])
    # out overlapping an input map / the mask bank
    big = torch.full((2 * 96 * 96 + 184 * 232,), 0.5, device='cuda')
    refused('overlaps map 0', maps=[big[96 * 96:96 * 96 + 184 * 232].view(184, 232)], out_=big[:2 * 96 * 96].view(1, 96, 96, 2))
    bank = torch.ones(2 * 96 * 96, device='cuda')
    refused('overlaps the mask bank', robots=[[RobotStamp((0.0, 0.0), 0.0, 0, 0.625)]], masks_=bank.view(2, 96, 96), out_=bank.view(1, 96, 96, 2))
    # the library still works afterwards, and the legal extremes are accepted
    ok = simq_mod.local_state_images([gm], chans, [((-0.5, 0.25), 0.3), ((0.5, -0.25), -2.0)], robots=[[RobotStamp((0.0, 0.0), 0.0, 0, 0.625)]] * 2,
                                     masks=masks)
    assert tuple(ok.shape) == (2, 96, 96, 2) and bool(torch.isfinite(ok).all())


def test_c_abi_validation_rules_on_real_buffers_launch_nothing(simq_mod, golden_dir):
    """The rules the Python layer cannot break (rotated shapes, non-finite doubles, robot ranges, buffer sizes), through the C-ABI on a
    fixture's real device buffers with one field corrupted at a time: refused, nothing launched, the output keeps its sentinel."""
    import copy
    from simq import _lib, local_maps as lm
    fx = oracle.load_fixture(os.path.join(golden_dir, 'local_maps_184x232.npz'))
    poses, robots = fixture_inputs(fx)
    out = torch.full(fx['want'].shape, SENTINEL, device='cuda')
    args, _, keep = lm._prepare(torch.from_numpy(fx['maps']).cuda(), fx['channels'], poses, robots, fx['masks'], out, None)
    ROBOTS, PROBS, CHANS, DESC_BYTES, OUT_FLOATS = 4, 6, 8, 11, 13      # positions in simq_local_state_images' argument list

    def refused(match, edit):
        a = list(args)
        for k in (ROBOTS, PROBS, CHANS):
            a[k] = copy.deepcopy(a[k])
        edit(a)
        _lib.lib.c.simq_launch_counts_reset()
        assert _lib.lib.c.simq_local_state_images(*a) == -1
        assert match in _lib.last_error(), (match, _lib.last_error())
        torch.cuda.synchronize()
        assert _lib.lib.c.simq_launch_count(b'local_state') == 0 and bool((out == SENTINEL).all())

    def setter(index, item, path, value):
        def edit(a):
            obj = a[index][item]
            for name in path[:-1]:
                obj = getattr(obj, name)
            if isinstance(path[-1], tuple):
                getattr(obj, path[-1][0])[path[-1][1]] = value
            else:
                setattr(obj, path[-1], value)
        return edit

    refused('rotated crop shape', setter(PROBS, 3, ('rot', ('shape', 0)), 135))
    refused('rotated crop shape', setter(PROBS, 3, ('rot', ('shape', 1)), 194))
    refused('not finite', setter(PROBS, 5, ('rot', ('r', 2)), float('nan')))
    refused('not finite', setter(PROBS, 5, ('rot', ('offset', 1)), float('inf')))
    refused('rotated mask shape', setter(ROBOTS, 2, ('rot', ('shape', 0)), 137))
    refused('not finite', setter(ROBOTS, 2, ('rot', ('r', 0)), float('-inf')))
    refused('outside the 12 given', setter(PROBS, 0, ('robot_count',), 13))
    refused('outside the 12 given', setter(PROBS, 0, ('robot_begin',), -1))
    refused('outside the bank', setter(ROBOTS, 0, ('seg_mask',), 5))
    refused('outside the 3 given', setter(CHANS, 7, ('map',), 3))
    refused('kind 9', setter(CHANS, 7, ('kind',), 9))
    refused('crop around pixel', setter(PROBS, 1, ('pixel_i',), 67))

    def smaller(index, by):
        def edit(a):
            a[index] = ctypes.c_int64(a[index].value - by)
        return edit
    refused('d_out holds', smaller(OUT_FLOATS, 1))
    refused('d_desc holds', smaller(DESC_BYTES, 8))
    # untouched, the same arguments run
    _lib.lib.call('simq_local_state_images', *args)
    assert np.array_equal(bits(out), bits(fx['want']))
    del keep


def test_single_image_drop_ins_equal_the_batched_call(simq_mod, golden_dir):
    fx = oracle.load_fixture(os.path.join(golden_dir, 'local_maps_232x232.npz'))
    poses = [(s['position'], s['heading']) for s in fx['states']]
    batch = simq_mod.local_state_images(fx['maps'], [('map', 0), ('distance', 1)], poses).cpu().numpy()
    for p, (position, heading) in enumerate(poses):
        a = simq_mod.local_map(fx['maps'][0], position, heading)
        b = simq_mod.local_distance_map(fx['maps'][1], position, heading)
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (96, 96)
        assert np.array_equal(bits(a), bits(batch[p, :, :, 0])) and np.array_equal(bits(b), bits(batch[p, :, :, 1]))
        assert np.array_equal(bits(a), bits(fx['want'][p, :, :, 0])) and np.array_equal(bits(b), bits(fx['want'][p, :, :, 1]))
        assert b.min() == 0
