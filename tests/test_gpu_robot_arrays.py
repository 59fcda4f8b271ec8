"""GPU: BatchedMapper.get_states on a simq.RobotArrays against the list form on the same object and against the reference Mapper's
rounds (tests/golden/mapper_*.npz).  The two fixture episodes live in one object (E = 2, M = 6: two room shapes, two robot groups, a
lifting robot, an idle robot).  The array form has to give the same states bit for bit, make the same library calls with the same
descriptor bytes, keep the status protocol and the `into=` protocol, and do so without the scalar helpers of the list form."""
import ctypes
import glob
import math
import os
import random

import numpy as np
import pytest
import torch

import mapper_oracle as oracle

pytestmark = pytest.mark.gpu

CONFIGS = oracle.configurations()
SHUFFLED = [4, 1, 5, 0]
SENT = 0x7FC0BEEF                                                   # a NaN with a payload: any element left unwritten shows


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.int32)


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


def build(S, episodes, cfg):
    masks = {name: episodes[0]['masks'][k] for k, name in enumerate(episodes[0]['mask_names'])}
    flags = {f: cfg[f] for f in oracle.FLAGS}
    rest = {k: v for k, v in cfg.items() if k not in oracle.FLAGS}
    return S.BatchedMapper([f['room_width'] for f in episodes], [f['room_length'] for f in episodes], [f['types'] for f in episodes], masks,
                           [f['groups'] for f in episodes], [f['receptacle_position'] for f in episodes], **flags, **rest)


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
    """{configuration name: an object after the update of round 0}, each made once and only read by the tests that share it."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = build(S, episodes, CONFIGS[name])
            made[name].update(*round_inputs(S, episodes, 0)[0])
        return made[name]
    return get


# ---- the library calls of a get_states, as comparable values --------------------------------------------------------------------------
# per entry: the arguments that are output or scratch pointers of the call (or the slot table of the handles, which differ between two
# calls), and (output pointer, element count) where later calls read the output
ENTRIES = {'simq_grid_distance_images_snapped': ((6, 7, 14), (7, 8)), 'simq_intention_maps': ((7, 9), (9, 10)),
           'simq_local_state_images': ((10, 12), None), 'simq_local_state_images_slots': ((10, 11), None)}


def value(arg):
    if isinstance(arg, ctypes.Array):
        return ('table', bytes(arg))
    if hasattr(arg, 'tobytes'):
        return ('table', arg.tobytes())
    return ('scalar', arg.value if hasattr(arg, 'value') else arg)


def recorded(L, monkeypatch, fn):
    """(fn()'s result or exception, the library calls it made: [(entry, [argument values])], the read-backs it made).  In the map table
    of stage 3 an address inside the output of an earlier call of the same sequence becomes (that call, byte offset): the outputs of
    two sequences lie elsewhere, what is compared is which element of which stage every map names."""
    from simq import _batch, local_maps
    calls, reads = [], []
    real, real_bad = L.Lib.call, _batch.bad_problems
    with monkeypatch.context() as mp:
        mp.setattr(L.Lib, 'call', staticmethod(lambda name, *a, **k: calls.append((name, [value(x) for x in a])) or real(name, *a, **k)))
        mp.setattr(_batch, 'bad_problems', lambda *a, **k: reads.append(1) or real_bad(*a, **k))
        try:
            result = fn()
        except Exception as e:
            result = e
    outputs, seen = [], []
    for name, args in calls:
        assert name in ENTRIES, name
        skip, output = ENTRIES[name]
        if name.startswith('simq_local_state_images'):
            maps = np.frombuffer(args[0][1], local_maps.LOCAL_MAP).copy()
            for k, (lo, n) in enumerate(outputs):
                inside = (maps['d_data'] >= lo) & (maps['d_data'] < lo + 4 * n)
                maps['d_data'][inside] = ((k + 1) << 56) + (maps['d_data'][inside] - lo)
            args[0] = ('table', maps.tobytes())
        if output is not None:
            outputs.append((args[output[0]][1], args[output[1]][1]))
        seen.append((name, [a for k, a in enumerate(args) if k not in skip]))
    return result, seen, len(reads)


def same_calls(a, b, tag):
    assert [name for name, _ in a] == [name for name, _ in b], tag
    for (name, x), (_, y) in zip(a, b):
        assert len(x) == len(y), (tag, name)
        for k, (u, v) in enumerate(zip(x, y)):
            assert u == v, (tag, name, k, u[0], len(u[1]) if u[0] == 'table' else (u[1], v[1]))


# ---- 1: every configuration, round by round, against the golden and against the list form -----------------------------------------------
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_array_form_equals_the_golden_and_the_list_form_round_by_round(S, episodes, name):
    cfg = CONFIGS[name]
    bm = build(S, episodes, cfg)
    for t in range(len(episodes[0]['rounds'])):
        frames, robots = round_inputs(S, episodes, t)
        bm.update(*frames)
        ra = S.RobotArrays.from_states(bm, robots)
        for mappers in (None, SHUFFLED):
            want = expected(cfg, episodes, t, mappers or range(6))
            by_list = bm.get_states(robots, mappers=mappers)
            list_maps = dict(bm.stage_maps)
            got = bm.get_states(ra, mappers=mappers)
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
            assert np.array_equal(bits(got), bits(want)), (name, t, mappers)
            assert np.array_equal(bits(got), bits(by_list)), (name, t, mappers)
            assert set(bm.stage_maps) == set(list_maps) and len(bm.stage_maps) == len(list_maps), (name, t, mappers)
            for key, tensor in list_maps.items():
                assert bm.stage_maps[key].shape == tensor.shape and np.array_equal(bits(bm.stage_maps[key]), bits(tensor)), (name, t, mappers, key)
        # an environment that no named mapper belongs to is not read
        alone = S.RobotArrays.from_states(bm, [None, robots[1]])
        assert np.array_equal(bits(bm.get_states(alone, mappers=[5, 3])), bits(expected(cfg, episodes, t, [5, 3]))), (name, t)


# ---- 2: the same library calls ----------------------------------------------------------------------------------------------------------
def same_calls_of_both_forms(L, monkeypatch, bm, cfg, robots, ra, mappers, shapes, tag):
    """Both forms of one get_states make the same library calls, and the calls are the ones the configuration asks for: one search
    when it has a shortest-path channel (and then one read-back), one drawing launch per room shape when it draws, one stage 3."""
    a, calls_a, reads_a = recorded(L, monkeypatch, lambda: bm.get_states(robots, mappers=mappers))
    b, calls_b, reads_b = recorded(L, monkeypatch, lambda: bm.get_states(ra, mappers=mappers))
    assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor), (tag, a, b)
    same_calls(calls_a, calls_b, tag)
    searches = int(cfg['use_shortest_path_to_receptacle_map'] or cfg['use_shortest_path_map'])
    draws = cfg['use_history_map'] or cfg['use_intention_map'] or (cfg['use_intention_channels'] and cfg['intention_channel_encoding'] == 'spatial')
    stages = [n for n, _ in calls_a]
    assert stages == ['simq_grid_distance_images_snapped'] * searches + ['simq_intention_maps'] * (shapes if draws else 0) + \
        ['simq_local_state_images'], (tag, stages)
    assert reads_a == reads_b == searches, tag
    assert np.array_equal(bits(a), bits(b)), tag


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_both_forms_make_the_same_library_calls(S, episodes, updated, monkeypatch, name):
    from simq import _lib as L
    bm = updated(name)
    robots = round_inputs(S, episodes, 0)[1]
    ra = S.RobotArrays.from_states(bm, robots)
    for mappers in (None, SHUFFLED, [2]):
        same_calls_of_both_forms(L, monkeypatch, bm, CONFIGS[name], robots, ra, mappers, 1 if mappers == [2] else 2, (name, mappers))


@pytest.mark.parametrize('name', ['use_distance_to_receptacle_map', 'full_spatial'])
def test_same_library_calls_where_two_environments_share_a_receptacle_map(S, episodes, monkeypatch, name):
    """Environments 0 and 2 have one room and one receptacle, so one distance-to-receptacle map: stage 3's map table names it once,
    at the mapper that uses it first -- of environment 0, or of environment 2 where `mappers` comes to that one first."""
    from simq import _lib as L
    three = [episodes[0], episodes[1], episodes[0]]
    bm = build(S, three, CONFIGS[name])
    frames, robots = round_inputs(S, three, 0)
    bm.update(*frames)
    assert bm.distance_to_receptacle_maps[0] is bm.distance_to_receptacle_maps[2] is not bm.distance_to_receptacle_maps[1]
    ra = S.RobotArrays.from_states(bm, robots)
    for mappers in (None, [7, 1, 4, 6, 0, 8], [8, 2]):
        same_calls_of_both_forms(L, monkeypatch, bm, CONFIGS[name], robots, ra, mappers, 1 if mappers == [8, 2] else 2, (name, mappers))


# ---- 3: poses the golden rounds do not reach --------------------------------------------------------------------------------------------
QUARTERS = list(range(-4, 5))                                       # the headings k * pi / 4: every one is given to a compared mapper


def quarter_turns(draw):
    """{mapper: k} of one draw: two mappers have the heading k * pi / 4.  Over the 8 draws every k of -4 .. 4 comes up (draw d gives
    QUARTERS[d] and QUARTERS[(d + 4) % 9]: 0 .. 7 and 4 .. 8, 0, 1, 2) and every mapper of both environments has some of them."""
    return {draw % 6: QUARTERS[draw], (draw + 3) % 6: QUARTERS[(draw + 4) % 9]}


def random_robots(S, episodes, rng, draw):
    """Robot states of both environments: positions inside the room, headings random / multiples of pi / 4 / +-pi and 0, random idle
    and lifting flags, targets, and paths of 1 to 12 waypoints (a path may repeat a waypoint).  Besides the multiple of pi / 4 that
    is drawn at random, the mappers of quarter_turns(draw) get theirs, so that none of the nine depends on the seed."""
    envs, fixed = [], quarter_turns(draw)
    for e, ep in enumerate(episodes):
        w, l = ep['room_width'] / 2 - 0.05, ep['room_length'] / 2 - 0.05
        point = lambda: (float(rng.uniform(-l, l)), float(rng.uniform(-w, w)))
        env = []
        for k, (kind, proto) in enumerate(zip(ep['types'], ep['rounds'][0]['robots'])):
            heading = [float(rng.uniform(-math.pi, math.pi)), float(rng.randint(-4, 5)) * math.pi / 4, math.pi, -math.pi, 0.0][(draw + k) % 5]
            if 3 * e + k in fixed:
                heading = fixed[3 * e + k] * math.pi / 4
            idle = bool(rng.rand() < 0.3)
            path = lambda: [point() for _ in range(rng.randint(1, 13))]
            intention, history = path(), path()
            if len(intention) > 2 and rng.rand() < 0.5:
                intention[1] = intention[0]
            env.append(S.RobotState(point(), heading, kind, 'lifting' if rng.rand() < 0.5 else 'ready', idle, None if idle else point() + (0.0,),
                                    None if idle else intention, None if idle else history))
        envs.append(env)
    return envs


@pytest.mark.parametrize('name', ['full_spatial', 'full_nonspatial'])
def test_random_poses_give_the_states_of_the_list_form(S, episodes, updated, name):
    bm = updated(name)
    rng = np.random.RandomState(5)
    compared = set()                                                # the k whose heading k * pi / 4 a compared state was rotated by
    for draw in range(8):
        robots = random_robots(S, episodes, rng, draw)
        ra = S.RobotArrays.from_states(bm, robots)
        turned = quarter_turns(draw)
        mappers = None
        if draw % 2:                                                # four mappers in a random order, the two quarter turns among them
            rest = [m for m in range(6) if m not in turned]
            mappers = [int(m) for m in rng.permutation(sorted(turned) + [rest[k] for k in rng.permutation(4)[:2]])]
        for m, k in turned.items():
            assert (mappers is None or m in mappers) and ra.heading[m] == robots[m // 3][m % 3].heading == k * math.pi / 4, (draw, m, k)
            compared.add(k)
        want = bm.get_states(robots, mappers=mappers)
        got = bm.get_states(ra, mappers=mappers)
        assert np.array_equal(bits(got), bits(want)), (name, draw, mappers)
    assert compared == set(QUARTERS) and -4 * math.pi / 4 == -math.pi and 4 * math.pi / 4 == math.pi


# ---- 4: none of the scalar helpers ------------------------------------------------------------------------------------------------------
def test_array_form_does_not_use_the_scalar_helpers(S, episodes, updated, monkeypatch):
    from simq import intention_drawing, local_maps, mapper
    cfg = CONFIGS['full_spatial']
    bm = build(S, episodes, cfg)                                    # (an object of its own: nothing it needs has been made before)
    frames, robots = round_inputs(S, episodes, 0)
    bm.update(*frames)
    ra = S.RobotArrays.from_states(bm, robots)

    def refuse(*a, **k):
        raise AssertionError('a scalar helper of the list form was called')
    for module, helper in ((local_maps, 'rotation'), (local_maps, '_rotation_struct'), (local_maps, 'position_to_pixel_indices'),
                           (intention_drawing, 'position_to_pixel_indices'), (intention_drawing, 'segments'), (intention_drawing, '_length'),
                           (mapper, '_distance')):
        monkeypatch.setattr(module, helper, refuse)
    with pytest.raises(AssertionError, match='scalar helper'):      # the list form does call them
        bm.get_states(robots)
    for mappers in (None, SHUFFLED):
        assert np.array_equal(bits(bm.get_states(ra, mappers=mappers)), bits(expected(cfg, episodes, 0, mappers or range(6))))


# ---- 5: into= ---------------------------------------------------------------------------------------------------------------------------
def test_array_form_writes_into_reserved_slots_as_the_list_form_does(S, episodes, updated, monkeypatch):
    from simq import _lib as L
    cfg = CONFIGS['full_spatial']
    bm = updated('full_spatial')
    robots = round_inputs(S, episodes, 0)[1]
    ra = S.RobotArrays.from_states(bm, robots)
    want = expected(cfg, episodes, 0, SHUFFLED)
    rings, handles, calls = [], [], []
    for form in (robots, ra):
        ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=len(bm.channels), pool_slots=12)
        ring.pool.view(torch.int32).fill_(SENT)
        ring.reserve(3)                                             # (dropped at once: the free list is no longer in slot order)
        hs = ring.reserve(4)
        got, seen, reads = recorded(L, monkeypatch, lambda: bm.get_states(form, mappers=SHUFFLED, into=hs))
        assert len(got) == 4 and all(g is h for g, h in zip(got, hs)) and reads == 1
        assert [n for n, _ in seen][-1] == 'simq_local_state_images_slots' and 'simq_local_state_images' not in [n for n, _ in seen]
        for n, args in seen:                                        # (the pools are two: their addresses differ, nothing else may)
            if n == 'simq_local_state_images_slots':
                assert args[11] == ('scalar', ring.pool.data_ptr())
                del args[11]
        rings.append(ring)
        handles.append(hs)
        calls.append(seen)
    same_calls(calls[0], calls[1], 'into')
    torch.cuda.synchronize()
    assert [h.slot for h in handles[0]] == [h.slot for h in handles[1]]
    pools = [bits(r.pool) for r in rings]
    assert np.array_equal(pools[0], pools[1])
    for p, h in enumerate(handles[1]):
        assert np.array_equal(pools[1][h.slot], bits(want[p])) and np.array_equal(bits(np.asarray(h)), bits(want[p])), p
    assert (pools[1][sorted(set(range(12)) - {h.slot for h in handles[1]})] == SENT).all()
    # the handles are transitions like any other
    ring, hs = rings[1], handles[1]
    ring.push(hs[0], 3, 1.0, hs[1])
    ring.push(hs[1], 4, 0.0, None)
    random.seed(1)
    idx = ring.sample_indices(2)
    random.seed(1)
    batch = ring.sample(2)
    torch.cuda.synchronize()
    assert np.array_equal(bits(batch.state), pools[1][[int(ring.buffer[i].state) for i in idx]])
    # section 18's checks of `into`, before anything is launched
    with pytest.raises(ValueError, match='3 handles for 4 states'):
        bm.get_states(ra, mappers=SHUFFLED, into=hs[:3])
    with pytest.raises(ValueError, match='`into` and `out`'):
        bm.get_states(ra, mappers=SHUFFLED, into=hs, out=torch.empty((4, 96, 96, len(bm.channels)), device='cuda'))


@pytest.mark.parametrize('mode', [True, 'index', False], ids=['upload_stream', 'index', 'consuming_stream'])
def test_stream_order_with_the_array_form_writing(S, episodes, updated, mode):
    """Section 18's stream-order test with get_states(into=) in the place of adopt: the slots are written behind a long kernel on a
    side stream and sampled at once from the default stream."""
    name = 'use_intention_map_ramp'                                 # (no distance images: the call ends without a read-back)
    cfg, bm = CONFIGS[name], updated(name)
    robots = round_inputs(S, episodes, 0)[1]
    ra = S.RobotArrays.from_states(bm, robots)
    want = expected(cfg, episodes, 0, range(6))
    ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=len(bm.channels), pool_slots=12, upload_stream=mode)
    ring.pool.view(torch.int32).fill_(SENT)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        if hasattr(torch.cuda, '_sleep'):                           # tens of milliseconds of work ahead of the write
            torch.cuda._sleep(60_000_000)
        else:
            big = torch.empty(1 << 28, device='cuda')
            for _ in range(40):
                big.fill_(1.0)
        hs = bm.get_states(ra, into=ring.reserve(6))
    for k in range(6):
        ring.push(hs[k], k, 0.5 * k, hs[(k + 1) % 6] if k % 3 else None)
    random.seed(5)
    idx = ring.sample_indices(4)
    random.seed(5)
    batch = ring.sample(4)
    torch.cuda.synchronize()
    assert np.array_equal(bits(batch.state), bits(np.stack([want[i] for i in idx])))
    assert np.array_equal(bits(batch.next_state), bits(np.stack([want[(i + 1) % 6] for i in idx if i % 3])))


# ---- 6: the status protocol -------------------------------------------------------------------------------------------------------------
def test_a_mapper_without_an_update_names_itself_after_the_states_are_written(S, episodes, monkeypatch):
    from simq import _lib as L
    from simq._lib import SimqError
    cfg = CONFIGS['full_spatial']
    bm = build(S, episodes, cfg)
    frames, robots = round_inputs(S, episodes, 0)
    good = [0, 1, 2, 3, 5]
    bm.update(*[[part[m] for m in good] for part in frames], mappers=good)
    ra = S.RobotArrays.from_states(bm, robots)
    outs, errors = [], []
    for form in (robots, ra):
        out = torch.full((6, 96, 96, len(bm.channels)), 5.0, device='cuda')
        error, _, reads = recorded(L, monkeypatch, lambda: bm.get_states(form, out=out))
        assert isinstance(error, SimqError) and reads == 1, error
        outs.append(bits(out))
        errors.append(str(error))
    assert errors[0] == errors[1] and 'no distance images for mapper(s) 4 (environment 1, robot 1)' in errors[1] and 'status [4, 4]' in errors[1]
    assert np.array_equal(outs[0], outs[1])
    want = expected(cfg, episodes, 0, range(6))
    for m in good:
        assert np.array_equal(outs[1][m], bits(want[m])), m
    for c in (3, 4):
        assert bm.channels[c].startswith('shortest_path') and not outs[1][4, :, :, c].any()
    assert np.array_equal(bits(bm.get_states(ra, mappers=good)), bits(want[good]))
