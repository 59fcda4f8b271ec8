"""CPU: what device-resident transitions check before they need a device -- the three places a new entry point is
named, the host refusals of simq_replay_scatter and simq_local_state_images_slots (fake device pointers, never dereferenced), the
bookkeeping of AliasedDeviceReplayBuffer.reserve / discard / push on handles, and the `into=` argument checks."""
import ctypes
import fnmatch
import gc
import glob
import os
import re

import numpy as np
import pytest
import torch

import mapper_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('simq_replay_scatter', 'simq_local_state_images_slots', 'simq_local_state_slots_desc_bytes')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_new_entry_points_are_named_in_the_header_the_map_file_and_the_ctypes_table(L):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'simq.h')).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'libsimq.map')).read()
    exported = re.search(r'global:\s*([^;]+);', version_script).group(1).split()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        proto = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, header)
        assert proto, '%s is not declared in include/simq.h' % name
        assert any(fnmatch.fnmatchcase(name, pattern) for pattern in exported), (name, exported)
        assert hasattr(raw, name), 'libsimq.so does not export %s' % name
        assert name in L.EXPORTS and len(L._SIGS[name][1]) == proto.group(1).count(',') + 1, name
    assert len(L._SIGS['simq_replay_scatter'][1]) == 9 and len(L._SIGS['simq_local_state_images_slots'][1]) == 16
    c = L.lib.c
    assert c.simq_local_state_slots_desc_bytes(3, 5, 7, 4) == c.simq_local_state_desc_bytes(3, 5, 7, 4) + 7 * 8
    assert c.simq_local_state_slots_desc_bytes(0, 0, -1, 1) == -1


def test_scatter_refuses_bad_slot_tables_before_any_device_call(L):
    c = L.lib.c
    SRC, POOL, DESC = 0x10000000, 0x20000000, 0x30000000
    item, pool_slots = 20, 9

    def call(slots, count=None, src=SRC, pool=POOL, desc=DESC, desc_bytes=1 << 10, item=item, pool_slots=pool_slots):
        count = len(slots) if count is None else count
        return c.simq_replay_scatter(ctypes.c_void_p(src), item, (ctypes.c_int64 * max(len(slots), 1))(*slots), count, ctypes.c_void_p(pool),
                                     pool_slots, ctypes.c_void_p(desc), desc_bytes, None)

    def refused(word, *a, **kw):
        assert call(*a, **kw) == -1, (a, kw)
        assert word in L.last_error(), (word, L.last_error())

    refused('NULL', [1], src=None)
    refused('NULL', [1], desc=None)
    refused('count = 0', [], count=0)
    refused('count = 65536', [0] * 4, count=65536)
    refused('item_floats = 0', [1], item=0)
    refused('pool_slots = 0', [0], pool_slots=0)
    refused('aligned', [1], src=SRC + 2)
    refused('aligned', [1], desc=DESC + 4)
    refused('slot -1 outside the pool of 9', [3, -1])
    refused('slot 9 outside the pool of 9', [9])
    refused('slot 3 is named twice', [3, 8, 0, 3])
    refused('d_desc holds 15 bytes, the slot table takes 16', [1, 2], desc_bytes=15)
    # the source or the scratch inside the pool: refused only when a WRITTEN slot shares a byte with it
    row = item * 4
    refused('slot 2 overlaps d_src', [5, 2], src=POOL + row)                       # rows 1 and 2
    refused('slot 3 overlaps d_src', [3], src=POOL + 3 * row - 4)                   # the last float of the row is the slot's first
    refused('slot 2 overlaps d_src', [2], src=POOL + 3 * row - 4 - (row - 4))      # ... and its first float the slot's last
    refused('slot 8 overlaps d_desc', [8], desc=POOL + 8 * row + 8, src=SRC)
    refused('d_src overlaps d_desc', [1], desc=SRC + 8)
    # the same layouts with the written slots elsewhere pass every host check: the call then reaches the device (none here: it fails
    # in the copy of the slot table, not in a check)
    if not torch.cuda.is_available():
        for slots, kw in (([5, 3], dict(src=POOL + row)), ([4], dict(src=POOL + 3 * row - 4)), ([7], dict(desc=POOL + 8 * row + 8))):
            assert call(slots, **kw) == -2, (slots, kw, L.last_error())


def test_local_state_slots_refuses_bad_slot_tables_before_any_device_call(L):
    from simq import local_maps as lm
    c = L.lib.c
    MAPS, MASKS, DESC, POOL = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    item = 96 * 96 * 4                                                              # one channel: bytes of a slot
    rot = lm.Rotation((ctypes.c_double * 4)(1, 0, -0.0, 1), (ctypes.c_double * 2)(0, 0), (ctypes.c_int32 * 2)(136, 136))

    def call(slots, n=None, maps=MAPS, desc=DESC, desc_bytes=1 << 20, pool=POOL, pool_slots=8, kind=0):
        n = len(slots) if n is None else n
        probs = (lm.LocalProblem * max(n, 1))(*[lm.LocalProblem(rot, 92, 116, 184, 232, 0, 0)] * max(n, 1))
        chans = (lm.LocalChannel * max(n, 1))(*[lm.LocalChannel(kind, 0, 0.0, 0)] * max(n, 1))
        a_maps = (lm.LocalMap * 1)(lm.LocalMap(maps, 184, 232))
        return c.simq_local_state_images_slots(a_maps, 1, ctypes.c_void_p(MASKS), 2, None, 0, probs, n, chans, 1,
                                               (ctypes.c_int64 * max(len(slots), 1))(*slots), ctypes.c_void_p(desc), desc_bytes,
                                               ctypes.c_void_p(pool), pool_slots, None)

    def refused(word, *a, **kw):
        assert call(*a, **kw) == -1, (a, kw)
        assert word in L.last_error(), (word, L.last_error())

    refused('NULL', [1], pool=None)
    refused('n = 0', [1], n=0)
    refused('pool_slots = 0', [0], pool_slots=0)
    refused('aligned', [1], pool=POOL + 2)
    refused('slot -1 outside the pool of 8', [-1, 2])
    refused('slot 8 outside the pool of 8', [2, 8])
    refused('slot 2 is named twice', [2, 5, 2])
    need = c.simq_local_state_slots_desc_bytes(1, 0, 2, 1)
    assert need == 16 + 2 * 80 + 2 * 16 + 2 * 8
    refused('d_desc holds %d bytes, the descriptors and the slot table take %d' % (need - 1, need), [1, 2], desc_bytes=need - 1)
    # a 184 x 232 map placed in the pool covers slots 3 .. 7 (170 752 bytes from slot 3 on, 36 864 each)
    assert -(-184 * 232 * 4 // item) == 5
    for s in (3, 7):
        refused('slot %d overlaps map 0' % s, [0, s], maps=POOL + 3 * item)
    refused('slot 1 overlaps d_desc', [1], desc=POOL + item + 64)
    refused('slot 0 overlaps the mask bank', [0], pool=MASKS)
    # the descriptors' own checks are the dense entry's, under this entry's name
    refused('local_state_images_slots: problem 0 channel 0: kind 5', [1], kind=5)
    if not torch.cuda.is_available():
        assert call([0, 2, 1], maps=POOL + 3 * item) == -2, L.last_error()           # every check passed: refused by the missing device


def cpu_pool(C=3, slots=6, capacity=4):
    from simq import learner
    return learner.AliasedDeviceReplayBuffer(capacity, C, device='cpu', pool_slots=slots)


def test_reserve_discard_and_push_keep_the_slot_counts(L):
    from simq import learner
    ring = cpu_pool()
    hs = ring.reserve(4)
    assert [type(h) for h in hs] == [learner._PoolObs] * 4 and all(isinstance(h, learner._DeviceObs) and h.pool is ring for h in hs)
    assert len({h.slot for h in hs}) == 4 and ring.observations_resident == 4 and hs[0].shape == (96, 96, 3)
    with pytest.raises(learner.SimqError, match='6 slots, 2 free, 3 wanted'):
        ring.reserve(3)
    assert ring.observations_resident == 4
    ring.pool[hs[0].slot].fill_(2.0)
    ring.pool[hs[1].slot].fill_(3.0)
    ring.push(hs[0], 5, 0.5, hs[1])
    ring.push(hs[1], 6, 1.5, None)                                              # the same handle: one slot
    assert ring.observations_resident == 4 and ring._ref[hs[1].slot] == 3 and len(ring) == 2
    assert int(ring.buffer[0].next_state) == int(ring.buffer[1].state) == hs[1].slot and type(ring.buffer[0].state) is learner._DeviceObs
    assert np.asarray(hs[1]).shape == (96, 96, 3) and (np.asarray(ring.buffer[1].state) == 3.0).all() and (np.asarray(hs[0])[:, :, 1] == 2.0).all()
    kept = [hs[0].slot, hs[1].slot]
    del hs[2:]
    gc.collect()
    assert ring.observations_resident == 2
    ring.discard(hs)
    ring.discard(hs)
    assert ring.observations_resident == 2 and not hs[0].alive               # the transitions keep both slots
    with pytest.raises(learner.SimqError, match='discarded'):
        ring.push(hs[0], 0, 0.0, None)
    with pytest.raises(learner.SimqError, match='discarded'):
        np.asarray(hs[0])
    arr = np.zeros((96, 96, 3), np.float32)
    for k in range(4):                                                          # the ring wraps: the handle-pushed transitions let go
        ring.push(arr, k, 0.0, None)
    assert ring.observations_resident == 1 and all(ring._ref[s] == 0 for s in kept) and len(ring._free) == 5
    # handles of another pool and the refusals that name adopt()
    other = cpu_pool()
    h = other.reserve(1)[0]
    before = (len(ring), ring.position, ring.observations_resident)
    with pytest.raises(learner.SimqError, match='another pool.*adopt'):
        ring.push(h, 0, 0.0, None)
    with pytest.raises(learner.SimqError, match='another pool.*adopt'):
        ring.push(arr, 0, 0.0, h)
    with pytest.raises(learner.SimqError, match='handles of this pool'):
        ring.discard([h])
    assert (len(ring), ring.position, ring.observations_resident) == before and other.observations_resident == 1


def test_transition_tracker_hands_handles_on_by_identity():
    from simq.learner import TransitionTracker
    ring = cpu_pool(slots=12, capacity=8)
    h = ring.reserve(6)
    tracker = TransitionTracker([[h[0], h[1]], [h[2]]])
    tracker.update_action([[3, 4], [5]])
    out = tracker.update_step_completed([[0.5, 0.25], [1.0]], [[h[3], None], [h[4]]], False)
    assert [len(o) for o in out] == [1, 1] and out[0][0][0] is h[0] and out[0][0][3] is h[3] and out[1][0][3] is h[4]
    tracker.update_action([[6, None], [7]])
    out2 = tracker.update_step_completed([[0.0, 0.0], [0.0]], [[h[5], None], [None]], True)
    assert out2[0][0][0] is h[3] and out2[0][0][3] is h[5] and out2[0][1][0] is h[1] and out2[0][1][3] is None and out2[1][0][0] is h[4]
    for t in out[0] + out[1] + out2[0] + out2[1]:
        ring.push(*t)
    assert ring.observations_resident == 6 and int(ring.buffer[0].next_state) == int(ring.buffer[2].state) == h[3].slot


def mapper_fixture(golden_dir):
    from simq import mapper
    fx = mapper_oracle.load_fixture(sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))[0])
    masks = {name: fx['masks'][k] for k, name in enumerate(fx['mask_names'])}
    bm = mapper.BatchedMapper(room_width=fx['room_width'], room_length=fx['room_length'], robot_types=[fx['types']], robot_masks=masks,
                              group_indices=[fx['groups']], receptacle_position=fx['receptacle_position'], use_shortest_path_map=True)
    robots = [[mapper.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'], r['history_path'])
               for r in fx['rounds'][0]['robots']]]
    return bm, robots


def test_into_is_checked_before_a_device_is_needed(golden_dir):
    import simq
    from simq._lib import SimqError
    bm, robots = mapper_fixture(golden_dir)
    C = len(bm.channels)
    ring, other = cpu_pool(C, 8), cpu_pool(C, 8)
    hs, foreign = ring.reserve(4), other.reserve(1)
    with pytest.raises(ValueError, match='`into` and `out`'):
        bm.get_states(robots, into=hs[:3], out=torch.empty((3, 96, 96, C)))
    with pytest.raises(ValueError, match='4 handles for 3 states'):
        bm.get_states(robots, into=hs)
    with pytest.raises(ValueError, match='1 handles for 2 states'):
        bm.get_states(robots, mappers=[2, 0], into=hs[:1])
    with pytest.raises(ValueError, match='more than one pool'):
        bm.get_states(robots, into=hs[:2] + foreign)
    with pytest.raises(ValueError, match='named twice'):
        bm.get_states(robots, into=[hs[0], hs[1], hs[0]])
    with pytest.raises(ValueError, match='takes the handles of AliasedDeviceReplayBuffer.reserve'):
        bm.get_states(robots, into=[hs[0], hs[1], np.zeros((96, 96, C), np.float32)])
    with pytest.raises(ValueError, match='%d channels, the states have %d' % (C + 1, C)):
        bm.get_states(robots, into=cpu_pool(C + 1, 8).reserve(3))
    ring.discard(hs[3:])
    with pytest.raises(ValueError, match='discarded'):
        bm.get_states(robots, into=hs[1:])
    # simq.local_state_images: the same checks, before the device is asked for
    good = np.zeros((184, 232), np.float32)
    pose = ((0.0, 0.0), 0.0)
    one = cpu_pool(1, 8)
    h1 = one.reserve(3)
    with pytest.raises(ValueError, match='`into` and `out`'):
        simq.local_state_images([good], [('map', 0)], [pose], into=h1[:1], out=torch.empty((1, 96, 96, 1)))
    with pytest.raises(ValueError, match='3 handles for 2 states'):
        simq.local_state_images([good], [('map', 0)], [pose, pose], into=h1)
    with pytest.raises(ValueError, match='more than one pool'):
        simq.local_state_images([good], [('map', 0)], [pose, pose], into=[h1[0], hs[0]])
    with pytest.raises(ValueError, match='named twice'):
        simq.local_state_images([good], [('map', 0)], [pose, pose], into=[h1[0], h1[0]])
    if not torch.cuda.is_available():
        # no quiet CPU path: with its handles in order a call says that it needs the device
        with pytest.raises(SimqError, match='need an MI355X'):
            bm.get_states(robots, into=hs[:3])
        with pytest.raises(SimqError, match='need an MI355X'):
            simq.local_state_images([good], [('map', 0)], [pose], into=h1[:1])
    assert ring.observations_resident == 3 and one.observations_resident == 3
