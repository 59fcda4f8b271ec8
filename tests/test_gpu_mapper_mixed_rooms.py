"""GPU: BatchedMapper(one_drawing_launch=True) on the two-room object of tests/test_gpu_mapper.py (both golden episodes, E = 2, M = 6:
rooms of 184 x 232 and 232 x 232 cells).  A get_states whose mappers have both room shapes draws every history map, intention map and
spatial channel map in one simq_intention_maps_shapes launch: the states equal the golden ones and those of an
object without the option bit for bit, in the list form and in the RobotArrays form, the stage maps equal the per-shape tensors of
today's calls, and the launches, the read-back, `into=` / `pools=` and the naming order are what they were."""
import glob
import os

import numpy as np
import pytest
import torch

import mapper_oracle as oracle

pytestmark = pytest.mark.gpu

CONFIGS = oracle.configurations()
NAMES = ['full_spatial', 'use_history_map']
SENT32, SENT16 = 0x7FC0BEEF, 0x7FC1


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)


def raw(t):
    return t.detach().cpu().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


@pytest.fixture(scope='module')
def episodes(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))
    assert len(files) == 2, files
    return [oracle.load_fixture(f) for f in files]


def build(S, episodes, cfg, **kw):
    masks = {name: episodes[0]['masks'][k] for k, name in enumerate(episodes[0]['mask_names'])}
    flags = {f: cfg[f] for f in oracle.FLAGS}
    rest = {k: v for k, v in cfg.items() if k not in oracle.FLAGS}
    return S.BatchedMapper([f['room_width'] for f in episodes], [f['room_length'] for f in episodes], [f['types'] for f in episodes], masks,
                           [f['groups'] for f in episodes], [f['receptacle_position'] for f in episodes], **flags, **rest, **kw)


def round_inputs(S, episodes, t):
    from simq.observation import CameraGeometry, IdRanges
    depth, ids, geoms, ranges, robots = [], [], [], [], []
    for ep in episodes:
        rnd = ep['rounds'][t]
        for f in rnd['frames']:
            depth.append(f['depth'])
            ids.append(f['ids'])
            geoms.append(CameraGeometry(*f['geometry']))
            ranges.append(IdRanges(*f['ranges']))
        robots.append([S.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'],
                                    r['history_path']) for r in rnd['robots']])
    return (depth, ids, geoms, ranges), robots


def expected(cfg, episodes, t, mappers):
    return np.stack([oracle.expected_state(cfg, episodes[m // 3]['rounds'][t]['images'], m % 3, 3) for m in mappers])


@pytest.fixture(scope='module')
def updated(S, episodes):
    """{configuration name: (the object with the option, the object without it, the robots), after the update of round 0}."""
    made = {}

    def get(name):
        if name not in made:
            frames, robots = round_inputs(S, episodes, 0)
            pair = [build(S, episodes, CONFIGS[name], one_drawing_launch=flag) for flag in (True, False)]
            for bm in pair:
                bm.update(*frames)
            assert pair[0].shapes == [(184, 232)] * 3 + [(232, 232)] * 3 and pair[0].one_drawing_launch and not pair[1].one_drawing_launch
            made[name] = (pair[0], pair[1], robots)
        return made[name]
    return get


def per_shape_maps(S, bm, robots, mappers, cfg):
    """What an object without the option hands out as stage maps, from two simq.intention_maps calls written out here: per room shape
    the history maps, the intention maps and the spatial channel maps of the named mappers of that shape."""
    out = {}
    for shape in sorted(set(bm.shapes[m] for m in mappers)):
        keys, paths, encodings = [], [], []
        for kind, encoding in (('history', 'history'), ('intention', cfg['intention_map_encoding'])):
            if not cfg['use_' + kind + '_map']:
                continue
            for p, m in enumerate(mappers):
                if bm.shapes[m] == shape:
                    others = [r for k, r in enumerate(robots[m // 3]) if k != m % 3 and not r.idle]
                    keys.append((kind, p))
                    paths.append([r.target if encoding == 'circle' else r.history_path if kind == 'history' else r.intention_path for r in others])
                    encodings.append(encoding)
        if cfg['use_intention_channels'] and cfg['intention_channel_encoding'] == 'spatial':
            for p, m in enumerate(mappers):
                if bm.shapes[m] == shape:
                    env, me = robots[m // 3], robots[m // 3][m % 3]
                    dists = [np.sqrt((r.position[0] - me.position[0])**2 + (r.position[1] - me.position[1])**2) for r in env]
                    for q, k in enumerate([int(k) for k in np.argsort(dists) if k != m % 3]):
                        keys.append(('channel', p, q))
                        paths.append([] if env[k].idle else [env[k].target])
                        encodings.append('circle')
        maps = S.intention_maps(paths, shape, encodings, cfg['intention_map_scale'], cfg['intention_map_line_thickness'])
        out.update({key: maps[i] for i, key in enumerate(keys)})
    return out


@pytest.mark.parametrize('name', NAMES)
def test_both_forms_give_the_golden_states_and_the_per_shape_stage_maps(S, episodes, updated, monkeypatch, name):
    from simq import _batch, _lib as L
    cfg = CONFIGS[name]
    bm, plain, robots = updated(name)
    ra = S.RobotArrays.from_states(bm, robots)
    searches = int(cfg['use_shortest_path_to_receptacle_map'] or cfg['use_shortest_path_map'])
    log = dict({'intention_maps_shapes': 1, 'local_state': 1}, **({'grid_distance_snapped': 1} if searches else {}))
    reads, real = [], _batch.bad_problems
    monkeypatch.setattr(_batch, 'bad_problems', lambda *a, **k: reads.append(1) or real(*a, **k))
    for mappers in (list(range(6)), [4, 1, 5, 0]):
        want = expected(cfg, episodes, 0, mappers)
        before = plain.get_states(robots, mappers=mappers)
        before_maps = dict(plain.stage_maps)
        by_hand = per_shape_maps(S, bm, robots, mappers, cfg)
        assert set(by_hand) == {k for k in before_maps if k[0] != 'image'}
        for form in (robots, ra):
            tag = (name, mappers, type(form).__name__)
            del reads[:]
            L.lib.c.simq_launch_counts_reset()
            got = bm.get_states(form, mappers=mappers)
            assert L.launch_counts() == log, tag
            assert len(reads) == searches, tag
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
            assert np.array_equal(bits(got), bits(want)), tag
            assert np.array_equal(bits(got), bits(before)), tag
            assert set(bm.stage_maps) == set(before_maps) and len(bm.stage_maps) == len(before_maps), tag
            for key, tensor in before_maps.items():
                mine = bm.stage_maps[key]
                assert tuple(mine.shape) == tuple(tensor.shape) and np.array_equal(bits(mine), bits(tensor)), tag + (key,)
            for key, tensor in by_hand.items():
                assert np.array_equal(bits(bm.stage_maps[key]), bits(tensor)), tag + (key,)
            # the drawn maps of a call are views of one flat tensor, in the order of the jobs
            drawn = [bm.stage_maps[k] for k in sorted(by_hand, key=lambda k: (('history', 'intention', 'channel').index(k[0]),) + k[1:])]
            at = drawn[0].data_ptr()
            for view in drawn:
                assert view.data_ptr() == at, tag
                at += 4 * view.numel()


def test_full_spatial_round_by_round(S, episodes):
    """Every round of the golden episodes, the update between them: both forms against the golden states."""
    cfg = CONFIGS['full_spatial']
    bm = build(S, episodes, cfg, one_drawing_launch=True)
    for t in range(len(episodes[0]['rounds'])):
        frames, robots = round_inputs(S, episodes, t)
        bm.update(*frames)
        want = expected(cfg, episodes, t, range(6))
        assert np.array_equal(bits(bm.get_states(robots)), bits(want)), t
        assert np.array_equal(bits(bm.get_states(S.RobotArrays.from_states(bm, robots))), bits(want)), t


def test_mappers_of_one_room_make_the_call_they_made(S, episodes, updated):
    from simq import _lib as L
    cfg = CONFIGS['full_spatial']
    bm, _, robots = updated('full_spatial')
    ra = S.RobotArrays.from_states(bm, robots)
    for mappers in ([3, 5, 4], [1], [0, 1, 2]):
        for form in (robots, ra):
            L.lib.c.simq_launch_counts_reset()
            got = bm.get_states(form, mappers=mappers)
            assert L.launch_counts() == {'grid_distance_snapped': 1, 'intention_maps': 1, 'local_state': 1}, mappers
            assert np.array_equal(bits(got), bits(expected(cfg, episodes, 0, mappers))), mappers
            assert tuple(bm.stage_maps[('history', 0)].shape) == bm.shapes[mappers[0]]


def test_a_shuffled_subset_across_both_rooms_follows_the_naming_order(S, episodes, updated):
    cfg = CONFIGS['full_spatial']
    bm, _, robots = updated('full_spatial')
    ra = S.RobotArrays.from_states(bm, robots)
    rng = np.random.RandomState(3)
    seen = set()
    for _ in range(4):
        mappers = [int(m) for m in rng.permutation(6)[:rng.randint(2, 6)]]
        if len({m // 3 for m in mappers}) < 2:
            mappers.append(5 - mappers[0])
        seen.add(tuple(mappers))
        want = expected(cfg, episodes, 0, mappers)
        for form in (robots, ra):
            got = bm.get_states(form, mappers=mappers)
            assert np.array_equal(bits(got), bits(want)), mappers
            for p, m in enumerate(mappers):
                assert tuple(bm.stage_maps[('intention', p)].shape) == bm.shapes[m], (mappers, p)
    assert len(seen) >= 3


def test_states_into_two_rings_are_the_slot_bytes_of_the_per_shape_path(S, episodes, updated):
    """get_states(into=, pools=) with a ring per robot group, fp32 and bf16: the object with the option and the one without write the
    same bytes into the same slots, in both forms."""
    from simq import _lib as L
    bm, plain, robots = updated('full_spatial')
    C = len(bm.channels)
    mappers = [4, 1, 5, 0]
    group_of = lambda m: episodes[m // 3]['groups'][m % 3]
    groups = sorted({g for ep in episodes for g in ep['groups']})
    assert len(groups) == 2 and len({group_of(m) for m in mappers}) == 2

    def rings():
        made = {g: S.AliasedDeviceReplayBuffer(8, C, pool_slots=12, dtype=d) for g, d in zip(groups, ('fp32', 'bf16'))}
        for r in made.values():
            r.pool.view(torch.int16).fill_(SENT16) if r.pool.dtype == torch.bfloat16 else r.pool.view(torch.int32).fill_(SENT32)
            r.reserve(3)                                            # (dropped at once: the free list is no longer in slot order)
        torch.cuda.synchronize()
        return made

    pools, slots = [], []
    for obj, form in ((plain, robots), (bm, robots), (bm, S.RobotArrays.from_states(bm, robots))):
        mine = rings()
        hs = [mine[group_of(m)].reserve(1)[0] for m in mappers]
        L.lib.c.simq_launch_counts_reset()
        got = obj.get_states(form, mappers=mappers, into=hs, pools=list(mine.values()))
        counts = L.launch_counts()
        assert all(g is h for g, h in zip(got, hs))
        assert counts == {'grid_distance_snapped': 1, 'intention_maps' if obj is plain else 'intention_maps_shapes': 2 if obj is plain else 1,
                          'local_state_pools': 1}, counts
        torch.cuda.synchronize()
        pools.append({g: raw(r.pool) for g, r in mine.items()})
        slots.append([(group_of(m), h.slot) for m, h in zip(mappers, hs)])
    assert slots[0] == slots[1] == slots[2]
    for g in groups:
        assert np.array_equal(pools[0][g], pools[1][g]) and np.array_equal(pools[0][g], pools[2][g]), g
    want = expected(CONFIGS['full_spatial'], episodes, 0, mappers)
    for p, (g, slot) in enumerate(slots[0]):
        if g == groups[0]:                                          # the fp32 ring holds the golden state as it is
            assert np.array_equal(pools[1][g][slot], bits(want[p])), p
