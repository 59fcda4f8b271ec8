"""CPU: the mapper oracle (tests/mapper_oracle.py: Mapper.update / get_state as the chain of the pinned stage oracles) against the
reference Mapper's own rounds (tests/golden/mapper_*.npz, tools/gen_mapper_golden.py), bit for bit; the channel count and order of
every flag set; and the argument checks of simq.BatchedMapper that need no device."""
import glob
import os

import numpy as np
import pytest

import mapper_oracle as oracle


def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))
    assert [os.path.basename(f) for f in files] == ['mapper_184x232.npz', 'mapper_232x232.npz'], files
    return [(os.path.basename(f), oracle.load_fixture(f)) for f in files]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_the_oracle_equals_every_fixture_bit_for_bit(golden_dir):
    """Every round of both episodes: the frames through Maps.update, then every distinct channel image of every robot, computed once
    under the configuration that holds them all (per intention encoding and kind of intention channels)."""
    n = 0
    for fname, fx in fixtures(golden_dir):
        assert oracle.padded_room_shape(fx['room_width'], fx['room_length']) == tuple(int(x) for x in fname[len('mapper_'):-4].split('x'))
        maps = [oracle.Maps(fx['room_width'], fx['room_length'], t) for t in fx['types']]
        receptacle_map = oracle.distance_to_receptacle_map(maps[0].shape, fx['receptacle_position'], 0.25)
        assert len(fx['rounds']) >= 2 and sorted(fx['groups']) == [0, 0, 1]                 # groups of unequal sizes
        seen_lifting = seen_idle = False
        for t, rnd in enumerate(fx['rounds']):
            for m, frame in zip(maps, rnd['frames']):
                assert m.update(frame['depth'], frame['ids'], frame['geometry'], frame['ranges']) == 0
            robots = rnd['robots']
            seen_lifting |= any(r['lift_state'] == 'lifting' for r in robots)
            seen_idle |= any(r['idle'] for r in robots)
            for r in range(len(robots)):
                got = {}
                cfgs = [oracle.config(**{f: True for f in oracle.FLAGS})]                     # all of them once, then only what is new
                cfgs += [oracle.config(use_intention_map=True, intention_map_encoding=enc) for enc in ('circle', 'binary', 'line')]
                cfgs += [oracle.config(use_intention_channels=True, intention_channel_encoding='nonspatial')]
                for cfg in cfgs:
                    images = oracle.channel_images(cfg, maps[r], robots, r, fx['masks'], fx['mask_names'], fx['receptacle_position'], receptacle_map)
                    got.update({oracle.image_key(cfg, name): img for name, img in images.items()})
                assert sorted(got) == sorted(rnd['images']), (fname, t, r)
                for key, img in got.items():
                    assert img.dtype == np.float32 and np.array_equal(bits(img), bits(rnd['images'][key][r])), (fname, t, r, key)
                    n += 1
        assert seen_lifting and seen_idle
    assert n == 2 * 3 * 3 * 16


def test_expected_states_stack_the_stored_images_in_the_reference_order(golden_dir):
    _, fx = fixtures(golden_dir)[0]
    rnd = fx['rounds'][0]
    for name, cfg in oracle.configurations().items():
        state = oracle.expected_state(cfg, rnd['images'], 1, 3)
        assert state.dtype == np.float32 and state.shape == (96, 96, len(oracle.channel_names(cfg, 3))), name
    full = oracle.expected_state(oracle.configurations()['full_nonspatial'], rnd['images'], 0, 3)
    assert full.shape[2] == 11 and np.array_equal(full[:, :, 0], rnd['images']['overhead'][0])
    # the nonspatial channels are constant images; those of the idle robot are zero
    assert all(np.ptp(full[:, :, c]) == 0 for c in range(7, 11))


def test_channel_count_and_order_of_every_flag_set():
    """envs.py:2067-2112: overhead, robot map, distance to receptacle, shortest path to receptacle, shortest path, history, intention,
    then the intention channels of the other robots (one each when spatial, two when nonspatial)."""
    from simq import mapper
    order = ['robots', 'distance_to_receptacle', 'shortest_path_to_receptacle', 'shortest_path', 'history', 'intention']
    assert mapper.FLAGS == oracle.FLAGS
    for bits_ in range(1 << 7):
        flags = {f: bool(bits_ >> k & 1) for k, f in enumerate(mapper.FLAGS)}
        for kind, per in (('spatial', 1), ('nonspatial', 2)):
            for n_robots in (1, 3, 4):
                want = ['overhead'] + [n for f, n in zip(mapper.FLAGS, order) if flags[f]]
                want += ['intention_channel_%d' % k for k in range(per * (n_robots - 1))] if flags['use_intention_channels'] else []
                assert mapper.channel_names(flags, kind, n_robots) == want
                assert oracle.channel_names(dict(flags, intention_channel_encoding=kind), n_robots) == want
    # the networks' channel counts of the reference's configurations: 4 (overhead, robots, two distance maps) and 5 (+ intention map)
    assert len(mapper.channel_names({'use_robot_map': True, 'use_distance_to_receptacle_map': True, 'use_shortest_path_map': True,
                                     'use_intention_map': True})) == 5


def test_host_side_constants_and_maps_equal_the_oracle(golden_dir):
    from simq import arch, mapper
    for t in oracle.BASE_LENGTH:
        assert (np.floor(arch.get_robot_radius(t) * 96), mapper.math.ceil(arch.ROBOT_HALF_WIDTH * 96)) == oracle.radii(t)
    assert arch.SEG_VALUES == oracle.SEG_VALUES
    for width, length in ((0.5, 1.0), (1.0, 1.0)):
        assert mapper.padded_room_shape(width, length) == oracle.padded_room_shape(width, length)
        assert np.array_equal(mapper.room_mask(width, length), oracle.room_mask(width, length))
    got = mapper.distance_to_receptacle_map((184, 232), (0.425, 0.175, 0), 0.25)
    assert np.array_equal(bits(got), bits(oracle.distance_to_receptacle_map((184, 232), (0.425, 0.175, 0), 0.25)))


def build(golden_dir, **kw):
    from simq import mapper
    _, fx = fixtures(golden_dir)[0]
    masks = {name: fx['masks'][k] for k, name in enumerate(fx['mask_names'])}
    args = dict(room_width=fx['room_width'], room_length=fx['room_length'], robot_types=[fx['types']], robot_masks=masks, group_indices=[fx['groups']],
                receptacle_position=fx['receptacle_position'])
    args.update(kw)
    return mapper.BatchedMapper(**args), fx


def test_argument_checks_that_need_no_device_raise_value_errors_in_the_operators_words(golden_dir):
    import torch
    from simq import mapper
    with pytest.raises(ValueError, match='unknown_encoding'):
        build(golden_dir, use_intention_map=True, intention_map_encoding='unknown_encoding')
    with pytest.raises(ValueError, match="intention_channel_encoding 'polar'"):
        build(golden_dir, intention_channel_encoding='polar')
    with pytest.raises(ValueError, match=r"robot type 'flying_robot'"):
        build(golden_dir, robot_types=[['lifting_robot', 'lifting_robot', 'flying_robot']])
    with pytest.raises(ValueError, match=r'\[3\] robots, \[2\] group indices'):
        build(golden_dir, group_indices=[[0, 1]])
    with pytest.raises(ValueError, match="robot_masks\\['lifting_robot_with_cube'\\]"):
        build(golden_dir, robot_masks={'lifting_robot': np.zeros((96, 96), np.float32), 'pushing_robot': np.zeros((96, 96), np.float32)})
    with pytest.raises(ValueError, match='need receptacle_position'):
        build(golden_dir, receptacle_position=None, use_shortest_path_to_receptacle_map=True)
    with pytest.raises(ValueError, match='same number of robots'):
        build(golden_dir, robot_types=[['pushing_robot'], ['pushing_robot', 'pushing_robot']], group_indices=None, use_intention_channels=True)
    with pytest.raises(ValueError, match='2 values for 1 environments'):
        build(golden_dir, room_width=[0.5, 1.0])

    bm, fx = build(golden_dir, use_shortest_path_map=True)
    assert bm.num_mappers == 3 and bm.channels == ['overhead', 'robots', 'shortest_path'] and bm.shapes == [(184, 232)] * 3
    robots = [[mapper.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'], r['history_path'])
               for r in fx['rounds'][0]['robots']]]
    # a wrong robot count: an environment of three robots described by two, two environments described to an object of one
    with pytest.raises(ValueError, match='environment 0 has 3 robots, got 2 robot states'):
        bm.get_states([robots[0][:2]])
    with pytest.raises(ValueError, match='2 lists for 1 environments'):
        bm.get_states(robots * 2)
    with pytest.raises(ValueError, match='robot 2 is a pushing_robot, got the state of a lifting_robot'):
        bm.get_states([robots[0][:2] + [robots[0][2]._replace(robot_type='lifting_robot')]])
    # an `out` of the wrong shape, dtype or kind
    with pytest.raises(ValueError, match=r'out must be a contiguous float32 device tensor of shape \(3, 96, 96, 3\), got torch.float32 \(3, 96, 96, 4\)'):
        bm.get_states(robots, out=torch.empty((3, 96, 96, 4)))
    with pytest.raises(ValueError, match=r'shape \(2, 96, 96, 3\)'):
        bm.get_states(robots, mappers=[2, 0], out=torch.empty((3, 96, 96, 3)))
    with pytest.raises(ValueError, match='got torch.float64'):
        bm.get_states(robots, out=torch.empty((3, 96, 96, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match='distinct mappers in 0 .. 2'):
        bm.get_states(robots, mappers=[0, 3])
    with pytest.raises(ValueError, match='distinct mappers'):
        bm.update(None, None, None, None, mappers=[1, 1])
    with pytest.raises(ValueError, match='no environment 1'):
        bm.reset([1])
    if not torch.cuda.is_available():
        # no quiet CPU path: with its arguments in order a call says that it needs the device
        from simq._lib import SimqError
        with pytest.raises(SimqError, match='need an MI355X'):
            bm.get_states(robots)


def test_closest_arguments_of_grid_distance_images_are_checked_before_any_device_is_needed():
    from simq import grid_paths
    grid = np.ones((8, 9), np.uint8)
    good = np.zeros((2, 8, 9), np.int32)
    for kw, words in ((dict(closest=[np.zeros((2, 8, 9), np.int64)]), 'closest\\[0\\] must be an int32 \\[2, rows, cols\\] array'),
                      (dict(closest=[np.zeros((2, 9, 8), np.int32)]), 'a grid of \\(8, 9\\) but closest\\[0\\] is \\(2, 9, 8\\)'),
                      (dict(closest=[good, good]), '2 closest blocks but 1 sources'),
                      (dict(closest=[good], closest_index=[1]), 'closest_index must name one of the 1 closest blocks'),
                      (dict(closest_index=[0]), 'need closest=')):
        with pytest.raises(ValueError, match=words):
            grid_paths.grid_distance_images([grid], [(1, 1)], **kw)
