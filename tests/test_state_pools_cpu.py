"""CPU: what states into several pools check before they need a device -- the three places the two new entry
points are named, every host refusal of simq_local_state_images_pools at its edge (fake device pointers, never dereferenced), and the
`pools=` argument checks of BatchedMapper.get_states and simq.local_state_images on rings that live on the host.

Pools, maps, the mask bank and d_desc are aligned to their elements, so two of them cannot share exactly one byte: the edges below are
one ELEMENT shared (refused) against none (accepted)."""
import ctypes
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

import test_device_transitions_cpu as tdc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('simq_local_state_images_pools', 'simq_local_state_pools_desc_bytes')


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
    assert len(L._SIGS['simq_local_state_images_pools'][1]) == 16 and len(L._SIGS['simq_local_state_pools_desc_bytes'][1]) == 5
    assert re.search(r'#define\s+SIMQ_LOCAL_MAX_POOLS\s+16\b', header) and '"local_state_pools"' in open(os.path.join(ROOT, 'include', 'simq.h')).read()
    # the structures as the header lays them out
    assert ctypes.sizeof(L.LocalPool) == 24 and ctypes.sizeof(L.LocalDest) == 16
    assert (L.LocalPool.pool_slots.offset, L.LocalPool.bf16.offset, L.LocalDest.pool.offset) == (8, 16, 8)
    c = L.lib.c
    assert c.simq_local_state_pools_desc_bytes(3, 5, 7, 4, 2) == c.simq_local_state_slots_desc_bytes(3, 5, 7, 4) + 2 * 24 + 7 * 16
    assert c.simq_local_state_pools_desc_bytes(0, 0, -1, 1, 1) == -1 and c.simq_local_state_pools_desc_bytes(0, 0, 1, 1, -1) == -1


MAPS, MASKS, DESC, POOL0, POOL1 = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
ITEM32, ITEM16 = 96 * 96 * 4, 96 * 96 * 2                                         # one channel: bytes of a slot of either type
MAP_BYTES = 184 * 232 * 4
TWO = [(POOL0, 8, 0), (POOL1, 16, 1)]                                             # (d_pool, pool_slots, bf16)


def test_pools_entry_refuses_bad_tables_before_any_device_call(L):
    from simq import local_maps as lm
    c = L.lib.c
    rot = lm.Rotation((ctypes.c_double * 4)(1, 0, -0.0, 1), (ctypes.c_double * 2)(0, 0), (ctypes.c_int32 * 2)(136, 136))

    def call(dests, pools=TWO, n=None, n_pools=None, maps=MAPS, masks=MASKS, desc=DESC, desc_bytes=1 << 20, kind=0):
        n = len(dests) if n is None else n
        probs = (lm.LocalProblem * max(n, 1))(*[lm.LocalProblem(rot, 92, 116, 184, 232, 0, 0)] * max(n, 1))
        chans = (lm.LocalChannel * max(n, 1))(*[lm.LocalChannel(kind, 0, 0.0, 0)] * max(n, 1))
        a_maps = (lm.LocalMap * 1)(lm.LocalMap(maps, 184, 232))
        table = (L.LocalPool * max(len(pools), 1))(*[L.LocalPool(p, s, b, 0) for p, s, b in pools])
        a_dests = (L.LocalDest * max(len(dests), 1))(*[L.LocalDest(slot, pool, 0) for pool, slot in dests])
        return c.simq_local_state_images_pools(a_maps, 1, ctypes.c_void_p(masks), 2, None, 0, probs, n, chans, 1, table,
                                               len(pools) if n_pools is None else n_pools, a_dests, ctypes.c_void_p(desc), desc_bytes, None)

    def refused(word, *a, **kw):
        assert call(*a, **kw) == -1, (a, kw)
        assert word in L.last_error(), (word, L.last_error())

    def accepted(*a, **kw):
        """Every host check passed: without a device the call then fails in the copy of the descriptors, not in a check."""
        if not torch.cuda.is_available():
            assert call(*a, **kw) == -2, (a, kw, L.last_error())

    one = [(0, 1)]
    refused('n = 0', one, n=0)
    refused('n_pools = 0 (1 .. 16)', one, n_pools=0)
    many = [(POOL0 + k * 0x1000000, 8, 0) for k in range(17)]
    refused('n_pools = 17 (1 .. 16)', one, pools=many)
    accepted(one, pools=many[:16])
    refused('pool 0: NULL d_pool', one, pools=[(None, 8, 0), TWO[1]])
    refused('pool 0: d_pool must be 4-byte aligned', one, pools=[(POOL0 + 2, 8, 0), TWO[1]])
    refused('pool 1: d_pool must be 2-byte aligned', one, pools=[TWO[0], (POOL1 + 1, 16, 1)])
    accepted(one, pools=[TWO[0], (POOL1 + 2, 16, 1)])                              # (a bf16 pool needs no more than its element's alignment)
    refused('pool 1: bf16 = 2', one, pools=[TWO[0], (POOL1, 16, 2)])
    refused('pool 1: bf16 = -1', one, pools=[TWO[0], (POOL1, 16, -1)])
    refused('pool 1: pool_slots = 0', one, pools=[TWO[0], (POOL1, 0, 1)])
    refused('pool 0: pool_slots = %d' % ((1 << 40) // ITEM32 + 1), one, pools=[(POOL0, (1 << 40) // ITEM32 + 1, 0)])
    refused('aligned', one, desc=DESC + 4)
    need = c.simq_local_state_pools_desc_bytes(1, 0, 2, 1, 2)
    assert need == 16 + 2 * 80 + 2 * 16 + 2 * 8 + 2 * 24 + 2 * 16
    refused('d_desc holds %d bytes, the descriptors, the pool table and the destinations take %d' % (need - 1, need), [(0, 1), (1, 2)],
            desc_bytes=need - 1)
    accepted([(0, 1), (1, 2)], desc_bytes=need)
    # two pools: the last element of one is the first of the other; one pool listed twice; end to end is fine
    refused('pool 0 overlaps pool 1', one, pools=[TWO[0], (POOL0 + 8 * ITEM32 - 2, 16, 1)])
    refused('pool 0 overlaps pool 1', one, pools=[(POOL1 + 16 * ITEM16 - 4, 8, 0), TWO[1]])
    refused('pool 0 overlaps pool 1', one, pools=[TWO[0], TWO[0]])
    refused('pool 0 overlaps pool 2', one, pools=[TWO[0], TWO[1], (POOL0 + 7 * ITEM32, 4, 1)])
    accepted(one, pools=[TWO[0], (POOL0 + 8 * ITEM32, 16, 1)])
    accepted(one, pools=[(POOL1 + 16 * ITEM16, 8, 0), TWO[1]])
    # destinations
    refused('problem 1: pool -1 outside the 2 given', [(0, 1), (-1, 1)])
    refused('problem 0: pool 2 outside the 2 given', [(2, 1), (0, 1)])
    refused('slot -1 outside pool 0 of 8', [(1, 3), (0, -1)])
    refused('slot 8 outside pool 0 of 8', [(0, 8), (1, 8)])
    refused('slot 16 outside pool 1 of 16', [(0, 7), (1, 16)])
    refused('slot 3 of pool 0 is named twice', [(0, 3), (1, 3), (0, 3)])
    refused('slot 15 of pool 1 is named twice', [(1, 15), (0, 3), (1, 3), (1, 15)])
    accepted([(0, 3), (1, 3)])                                                    # the same slot number in two pools
    accepted([(1, 0), (1, 15)])                                                   # a listed pool that receives nothing
    # a 184 x 232 map placed in the fp32 pool covers slots 3 .. 7, in the bf16 pool slots 3 .. 12; the written slots elsewhere: accepted
    assert -(-MAP_BYTES // ITEM32) == 5 and -(-MAP_BYTES // ITEM16) == 10
    for s in (3, 7):
        refused('slot %d of pool 0 overlaps map 0' % s, [(1, 4), (0, s)], maps=POOL0 + 3 * ITEM32)
    accepted([(0, 0), (0, 2), (1, 4)], maps=POOL0 + 3 * ITEM32)
    for s in (3, 12):
        refused('slot %d of pool 1 overlaps map 0' % s, [(0, 4), (1, s)], maps=POOL1 + 3 * ITEM16)
    accepted([(1, 2), (1, 13), (0, 4)], maps=POOL1 + 3 * ITEM16)
    # ... the map's last float the slot's first two elements, and its first float the slot's last two
    refused('slot 13 of pool 1 overlaps map 0', [(1, 13)], maps=POOL1 + 13 * ITEM16 + 4 - MAP_BYTES)
    accepted([(1, 13)], maps=POOL1 + 13 * ITEM16 - MAP_BYTES)
    refused('slot 2 of pool 1 overlaps map 0', [(1, 2)], maps=POOL1 + 3 * ITEM16 - 4)
    refused('slot 2 of pool 0 overlaps map 0', [(0, 2)], maps=POOL0 + 3 * ITEM32 - 4)
    # the mask bank (two masks) and d_desc
    refused('slot 2 of pool 0 overlaps the mask bank', [(1, 1), (0, 2)], masks=POOL0 + 3 * ITEM32 - 4)
    refused('slot 4 of pool 0 overlaps the mask bank', [(0, 4)], masks=POOL0 + 3 * ITEM32)
    accepted([(0, 2), (0, 5), (1, 3)], masks=POOL0 + 3 * ITEM32)                  # (the bank is slots 3 and 4 of the fp32 pool)
    refused('slot 6 of pool 1 overlaps the mask bank', [(1, 6)], masks=POOL1 + 3 * ITEM16)     # (slots 3 .. 6 of the bf16 pool)
    accepted([(1, 2), (1, 7)], masks=POOL1 + 3 * ITEM16)
    refused('slot 5 of pool 1 overlaps d_desc', [(0, 5), (1, 5)], desc=POOL1 + 5 * ITEM16 + 8)
    refused('slot 5 of pool 1 overlaps d_desc', [(1, 5)], desc=POOL1 + 6 * ITEM16 - 8)         # its first 8 bytes the slot's last
    refused('slot 6 of pool 1 overlaps d_desc', [(1, 6)], desc=POOL1 + 6 * ITEM16 - 8)
    accepted([(1, 4), (1, 7), (0, 5)], desc=POOL1 + 5 * ITEM16 + 8)
    refused('slot 1 of pool 0 overlaps d_desc', [(0, 1)], desc=POOL0 + ITEM32 + 64)
    # the descriptors' own checks are the dense entry's, under this entry's name
    refused('local_state_images_pools: problem 0 channel 0: kind 5', one, kind=5)
    refused('NULL', one, desc=None)
    accepted([(0, 0), (1, 2), (0, 1)], maps=POOL0 + 3 * ITEM32)


def meta_pool(C, slots=8):
    """A ring on another device than cpu_pool's that needs no GPU: torch's `meta` device allocates nothing."""
    from simq import learner
    return learner.AliasedDeviceReplayBuffer(4, C, device='meta', pool_slots=slots)


def test_pools_is_checked_before_a_device_is_needed(golden_dir):
    import simq
    from simq import mapper
    from simq._lib import SimqError
    bm, robots = tdc.mapper_fixture(golden_dir)
    C = len(bm.channels)
    a, b, unlisted = tdc.cpu_pool(C, 8), tdc.cpu_pool(C, 8), tdc.cpu_pool(C, 8)
    ha, hb, hu = a.reserve(3), b.reserve(2), unlisted.reserve(1)
    mixed = [ha[0], hb[0], ha[1]]
    arrays = mapper.RobotArrays.from_states(bm, robots)

    def both(match, **kw):
        for form in (robots, arrays):                                             # the list form and the RobotArrays form
            with pytest.raises(ValueError, match=match):
                bm.get_states(form, **kw)

    both('`pools` without `into`', pools=[a, b])
    both('`pools` lists the rings of `into`', pools=[a, b], out=torch.empty((3, 96, 96, C)))
    both('`into` and `out`', pools=[a, b], into=mixed, out=torch.empty((3, 96, 96, C)))
    both(r'0 pools \(1 \.\. 16\)', into=mixed, pools=[])
    both(r'17 pools \(1 \.\. 16\)', into=mixed, pools=[a, b] + [tdc.cpu_pool(C, 1) for _ in range(15)])
    both('a pool is named twice', into=mixed, pools=[a, b, a])
    both('pools are AliasedDeviceReplayBuffers, got Tensor', into=mixed, pools=[a, b.pool])
    both('the pools live on more than one device', into=mixed, pools=[a, b, meta_pool(C)])
    both('a pool holds states of %d channels, the states have %d' % (C + 1, C), into=mixed, pools=[a, b, tdc.cpu_pool(C + 1, 8)])
    both('a handle belongs to a pool that is not listed', into=[ha[0], hb[0], hu[0]], pools=[a, b])
    both('a handle belongs to a pool that is not listed', into=mixed, pools=[a])
    both('2 handles for 3 states', into=mixed[:2], pools=[a, b])
    both('a handle is named twice', into=[ha[0], hb[0], ha[0]], pools=[a, b])
    both('takes the handles of AliasedDeviceReplayBuffer.reserve', into=[ha[0], hb[0], np.zeros((96, 96, C), np.float32)], pools=[a, b])
    # without pools= the refusal of handles of two pools is the one it was
    both('get_states\\(into=\\): the handles belong to more than one pool', into=mixed)
    # simq.local_state_images: the same checks, before the device is asked for
    good, pose = np.zeros((184, 232), np.float32), ((0.0, 0.0), 0.0)
    p1, q1 = tdc.cpu_pool(1, 8), tdc.cpu_pool(1, 8)
    h1, g1 = p1.reserve(2), q1.reserve(2)

    def local(match, n=2, **kw):
        with pytest.raises(ValueError, match=match):
            simq.local_state_images([good], [('map', 0)], [pose] * n, **kw)

    local('`pools` without `into`', pools=[p1, q1])
    local('`pools` lists the rings of `into`', pools=[p1], out=torch.empty((2, 96, 96, 1)))
    local(r'0 pools \(1 \.\. 16\)', into=[h1[0], g1[0]], pools=())
    local('a pool is named twice', into=[h1[0], g1[0]], pools=[p1, q1, q1])
    local('more than one device', into=[h1[0], g1[0]], pools=[p1, q1, meta_pool(1)])
    local('a pool holds states of 3 channels, the states have 1', into=[h1[0], g1[0]], pools=[p1, q1, tdc.cpu_pool(3, 8)])
    local('a pool that is not listed', into=[h1[0], g1[0]], pools=[p1])
    local('a handle is named twice', into=[g1[1], g1[1]], pools=[p1, q1])
    local('3 handles for 2 states', into=[h1[0], g1[0], g1[1]], pools=[p1, q1])
    local('local_state_images\\(into=\\): the handles belong to more than one pool', into=[h1[0], g1[0]])
    if not torch.cuda.is_available():
        # no quiet CPU path: with its handles and its pools in order a call says that it needs the device
        for kw in (dict(into=mixed, pools=[a, b]), dict(into=ha, pools=[a]), dict(into=mixed, pools=[b, unlisted, a])):
            with pytest.raises(SimqError, match='need an MI355X'):
                bm.get_states(robots, **kw)
        with pytest.raises(SimqError, match='need an MI355X'):
            simq.local_state_images([good], [('map', 0)], [pose] * 2, into=[h1[0], g1[0]], pools=[p1, q1])
    assert (a.observations_resident, b.observations_resident, unlisted.observations_resident) == (3, 2, 1)
    assert (p1.observations_resident, q1.observations_resident) == (2, 2)
