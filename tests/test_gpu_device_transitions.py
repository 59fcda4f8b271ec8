"""GPU: device-resident transitions -- simq_replay_scatter and simq_local_state_images_slots on their own, then the
handles of AliasedDeviceReplayBuffer.reserve / adopt through push, sample, the policies, BatchedMapper.get_states(into=), checkpoints and
the visualisations.  Everything here is a copy or index bookkeeping: every comparison is bit for bit."""
import ctypes
import gc
import glob
import os
import random
import types

import numpy as np
import pytest
import torch

import local_maps_oracle
import mapper_oracle

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF                    # a NaN with a payload: any element written, or left unwritten, shows
W = 96


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


@pytest.fixture(scope='module')
def L(S):
    from simq import _lib
    return _lib


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def sentinel(*shape):
    t = torch.empty(shape, dtype=torch.float32, device='cuda')
    t.view(torch.int32).fill_(SENT)
    return t


def slots_array(slots):
    return (ctypes.c_int64 * max(len(slots), 1))(*slots)


def shuffled_slots(rng, count, pool_slots):
    """`count` distinct slots in random order, slot 0 and the last slot among them (count == 1: one of the two)."""
    rest = [int(s) for s in rng.permutation(np.arange(1, pool_slots - 1))[:max(count - 2, 0)]]
    picked = ([0, pool_slots - 1] if count >= 2 else [0]) + rest
    return [picked[k] for k in rng.permutation(len(picked))]


# ---- simq_replay_scatter --------------------------------------------------------------------------------------------------------------
def scatter(L, src, item, slots, pool, pool_slots, count=None, desc=None, desc_bytes=None):
    count = len(slots) if count is None else count
    desc = torch.empty(max(8 * count, 8), dtype=torch.uint8, device='cuda') if desc is None else desc
    rc = L.lib.c.simq_replay_scatter(L.ptr(src), item, slots_array(slots), count, L.ptr(pool), pool_slots, L.ptr(desc),
                                     8 * count if desc_bytes is None else desc_bytes, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


# (floats the source / the pool start behind a 16-byte boundary): aligned; the issue's source 4 bytes off (rows move float by float);
# both 4 bytes off (a scalar head of three floats before the vectors)
OFFSETS = [(0, 0), (1, 0), (1, 1)]


@pytest.mark.parametrize('offsets', OFFSETS, ids=['aligned', 'src+4B', 'src+4B,pool+4B'])
@pytest.mark.parametrize('count', [1, 3, 64])
@pytest.mark.parametrize('item', [1, 5, 36864])
def test_scatter_moves_rows_to_their_slots_and_nothing_else(L, item, count, offsets):
    rng = np.random.RandomState(1000 * count + item % 97)
    pool_slots = count + 6
    for slots in ([[0], [pool_slots - 1]] if count == 1 else [shuffled_slots(rng, count, pool_slots)]):
        src_store = torch.randn(count * item + 4, device='cuda')
        pool_store = sentinel(pool_slots * item + 4)
        src = src_store[offsets[0]:offsets[0] + count * item].view(count, item)
        pool = pool_store[offsets[1]:offsets[1] + pool_slots * item].view(pool_slots, item)
        assert src.data_ptr() % 16 == 4 * offsets[0] and pool.data_ptr() % 16 == 4 * offsets[1]
        L.lib.c.simq_launch_counts_reset()
        assert scatter(L, src, item, slots, pool, pool_slots) == 0, L.last_error()
        assert L.lib.c.simq_launch_count(b'replay_scatter') == 1
        got, want = bits(pool), bits(src)
        for p, s in enumerate(slots):
            assert np.array_equal(got[s], want[p]), (item, count, offsets, p, s)
        unnamed = sorted(set(range(pool_slots)) - set(slots))
        assert (got[unnamed] == SENT).all()
        assert (bits(pool_store[:offsets[1]]) == SENT).all() and (bits(pool_store[offsets[1] + pool_slots * item:]) == SENT).all()
        if item % 4 == 0 and offsets[1] == 0:                         # (simq_replay_gather moves float4s of an aligned ring)
            index = torch.tensor(slots, dtype=torch.int64, device='cuda')
            back = torch.empty((count, item), device='cuda')
            L.lib.call('simq_replay_gather', L.ptr(pool), item, L.ptr(index), count, L.ptr(back), L.stream_ptr())
            assert np.array_equal(bits(back), want)


def test_scatter_slot_offset_beyond_two_to_the_31_floats(L):
    item, pool_slots = W * W * 8, 30000
    assert (pool_slots - 1) * item > 2 ** 31
    try:
        pool = torch.empty((pool_slots, W, W, 8), dtype=torch.float32, device='cuda')
    except RuntimeError as e:                                         # (torch.cuda.OutOfMemoryError is one)
        pytest.skip('no room for a pool of %.1f GB: %s' % (pool_slots * item * 4 / 1e9, str(e)[:80]))
    src = torch.randn((2, W, W, 8), device='cuda')
    pool[1].view(torch.int32).fill_(SENT)
    pool[pool_slots - 2].view(torch.int32).fill_(SENT)
    assert scatter(L, src, item, [pool_slots - 1, 0], pool, pool_slots) == 0, L.last_error()
    assert np.array_equal(bits(pool[pool_slots - 1]), bits(src[0])) and np.array_equal(bits(pool[0]), bits(src[1]))
    assert (bits(pool[1]) == SENT).all() and (bits(pool[pool_slots - 2]) == SENT).all()
    index = torch.tensor([0, pool_slots - 1], dtype=torch.int64, device='cuda')
    back = torch.empty((2, W, W, 8), device='cuda')
    L.lib.call('simq_replay_gather', L.ptr(pool), item, L.ptr(index), 2, L.ptr(back), L.stream_ptr())
    assert np.array_equal(bits(back[0]), bits(src[1])) and np.array_equal(bits(back[1]), bits(src[0]))
    del pool
    torch.cuda.empty_cache()


def test_scatter_refusals_write_nothing_and_launch_nothing(L):
    item, pool_slots = 20, 9
    pool = sentinel(pool_slots, item)
    src = torch.randn((3, item), device='cuda')

    def refused(match, slots, src=src, **kw):
        L.lib.c.simq_launch_counts_reset()
        assert scatter(L, src, item, slots, pool, pool_slots, **kw) != 0
        assert match in L.last_error(), (match, L.last_error())
        assert L.launch_counts() == {} and (bits(pool) == SENT).all()

    refused('slot -1 outside the pool of 9', [2, -1, 4])
    refused('slot 9 outside the pool of 9', [2, 9, 4])
    refused('slot 4 is named twice', [4, 2, 4])
    refused('count = 0', [], count=0)
    refused('slot 2 overlaps d_src', [5, 2], src=pool[1:3])
    refused('d_desc holds 23 bytes', [2, 5, 4], desc_bytes=23)
    refused('slot 5 overlaps d_desc', [5], desc=pool[5].view(torch.uint8))
    # a source that lies in the same pool, in slots the call does not write, is accepted
    pool[1:3].copy_(src[:2])
    assert scatter(L, pool[1:3], item, [8, 0], pool, pool_slots) == 0, L.last_error()
    assert np.array_equal(bits(pool[8]), bits(src[0])) and np.array_equal(bits(pool[0]), bits(src[1]))
    assert (bits(pool[3:8]) == SENT).all()


# ---- simq_local_state_images_slots ---------------------------------------------------------------------------------------------------
def local_fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'local_maps_*.npz')))
    assert len(files) == 2, files
    return [(os.path.basename(f), local_maps_oracle.load_fixture(f)) for f in files]


def rotation_struct(lm, rot):
    R, off, shape = rot
    return lm.Rotation((ctypes.c_double * 4)(*np.asarray(R, np.float64).reshape(-1)), (ctypes.c_double * 2)(*off),
                       (ctypes.c_int32 * 2)(int(shape[0]), int(shape[1])))


class Tables:
    """The host descriptors of one fixture for the C ABI, from the float64 values the fixture stores (no scipy on this path)."""

    def __init__(self, fx, maps, masks, channels=None, problems=None):
        from simq import local_maps as lm
        self.maps, self.masks = maps, masks
        self.G, self.rows, self.cols = (len(maps), fx['maps'].shape[1], fx['maps'].shape[2])
        self.c_maps = (lm.LocalMap * max(self.G, 1))(*[lm.LocalMap(m.data_ptr(), self.rows, self.cols) for m in maps])
        robots, begin = [], {}
        for e, env in sorted(fx['robots'].items()):
            begin[e] = (len(robots), len(env))
            for pixel, rot, mask, seg, val, seg_mask in env:
                robots.append(lm.LocalRobot(rotation_struct(lm, rot), pixel[0], pixel[1], mask, seg, val, seg_mask))
        self.c_robots, self.n_robots = (lm.LocalRobot * len(robots))(*robots), len(robots)
        states = fx['states'] if problems is None else [fx['states'][p] for p in problems]
        self.P = len(states)
        self.c_probs = (lm.LocalProblem * self.P)(*[lm.LocalProblem(rotation_struct(lm, s['rot']), s['pixel'][0], s['pixel'][1], self.rows, self.cols,
                                                                    *begin[s['env']]) for s in states])
        chans = []
        for spec in (fx['channels'] if channels is None else channels):
            kind = spec if isinstance(spec, str) else spec[0]
            chans.append(lm.LocalChannel(lm.KINDS[kind], spec[1] if kind in ('map', 'distance', 'overhead') else 0,
                                         spec[1] if kind == 'constant' else 0.0, 0))
        self.C = len(chans)
        self.c_chans = (lm.LocalChannel * (self.P * self.C))(*(chans * self.P))

    def head(self):
        from simq import _lib
        return (self.c_maps if self.G else None, self.G, _lib.ptr(self.masks), self.masks.shape[0], self.c_robots, self.n_robots, self.c_probs,
                self.P, self.c_chans, self.C)

    def dense(self, L):
        need = L.lib.c.simq_local_state_desc_bytes(self.G, self.n_robots, self.P, self.C)
        desc = torch.empty(need, dtype=torch.uint8, device='cuda')
        out = sentinel(self.P, W, W, self.C)
        L.lib.call('simq_local_state_images', *self.head(), L.ptr(desc), ctypes.c_int64(need), L.ptr(out), ctypes.c_int64(out.numel()), L.stream_ptr())
        torch.cuda.synchronize()
        return out

    def slotted(self, L, slots, pool, n=None, desc_bytes=None, head=None):
        need = L.lib.c.simq_local_state_slots_desc_bytes(self.G, self.n_robots, self.P, self.C)
        assert need == L.lib.c.simq_local_state_desc_bytes(self.G, self.n_robots, self.P, self.C) + 8 * self.P
        desc = torch.empty(need, dtype=torch.uint8, device='cuda')
        head = list(self.head() if head is None else head)
        if n is not None:
            head[7] = n
        rc = L.lib.c.simq_local_state_images_slots(*head, slots_array(slots), L.ptr(desc), ctypes.c_int64(need if desc_bytes is None else desc_bytes),
                                                   L.ptr(pool), ctypes.c_int64(pool.shape[0]), L.stream_ptr())
        torch.cuda.synchronize()
        return rc


def device_inputs(fx):
    maps = torch.from_numpy(fx['maps']).cuda()
    return [maps[k] for k in range(maps.shape[0])], torch.from_numpy(fx['masks']).cuda()


def check_slotted(L, t, want, name):
    rng = np.random.RandomState(t.P * 64 + t.C)
    pool = sentinel(t.P + 5, W, W, t.C)
    slots = shuffled_slots(rng, t.P, t.P + 5)
    L.lib.c.simq_launch_counts_reset()
    assert t.slotted(L, slots, pool) == 0, L.last_error()
    assert L.launch_counts() == {'local_state_slots': 1}
    got, dense = bits(pool), bits(t.dense(L))
    for p, s in enumerate(slots):
        assert np.array_equal(got[s], dense[p]), (name, p, s)
        if want is not None:
            assert np.array_equal(got[s], bits(want[p])), (name, p, s)
    assert (got[sorted(set(range(t.P + 5)) - set(slots))] == SENT).all(), name
    return pool, slots


def test_local_state_slots_equal_the_golden_states_and_the_dense_entry(L, golden_dir):
    for name, fx in local_fixtures(golden_dir):
        maps, masks = device_inputs(fx)
        check_slotted(L, Tables(fx, maps, masks), fx['want'], name)
        # one channel; one problem (slot 0 only); the 64 constant channels the entry allows, no map named
        check_slotted(L, Tables(fx, maps, masks, channels=fx['channels'][:1]), fx['want'][..., :1], name + ' C=1')
        check_slotted(L, Tables(fx, maps, masks, problems=[len(fx['states']) - 1]), fx['want'][-1:], name + ' P=1')
        values = [float(np.float32(0.37 * k - 5)) for k in range(64)]
        t = Tables(fx, [], masks, channels=[('constant', v) for v in values])
        pool, slots = check_slotted(L, t, None, name + ' C=64')
        for s in slots:
            assert np.array_equal(bits(pool[s]), bits(np.broadcast_to(np.asarray(values, np.float32), (W, W, 64))))


def test_local_state_slots_refusals_and_maps_in_the_same_allocation(L, golden_dir):
    name, fx = local_fixtures(golden_dir)[0]
    maps, masks = device_inputs(fx)
    t = Tables(fx, maps, masks)
    n_slots = t.P + 12
    pool = sentinel(n_slots, W, W, t.C)
    good = list(range(t.P))

    def refused(match, slots, **kw):
        before = bits(pool).copy()
        L.lib.c.simq_launch_counts_reset()
        assert t.slotted(L, slots, pool, **kw) != 0
        assert match in L.last_error(), (match, L.last_error())
        assert L.launch_counts() == {} and np.array_equal(bits(pool), before)

    refused('slot -1 outside the pool', [-1] + good[1:])
    refused('slot %d outside the pool of %d' % (n_slots, n_slots), good[:-1] + [n_slots])
    if t.P >= 2:
        refused('slot 1 is named twice', [1] + good[1:])
    refused('n = 0', good, n=0)
    refused('d_desc holds', good, desc_bytes=L.lib.c.simq_local_state_slots_desc_bytes(t.G, t.n_robots, t.P, t.C) - 1)
    # map 0 moved into the pool itself: it spans `span` slots from slot t.P + 2 on
    item, size = W * W * t.C, t.rows * t.cols
    span = -(-size // item)
    assert t.P + 2 + span <= n_slots - 1
    inside = pool.view(-1)[(t.P + 2) * item:(t.P + 2) * item + size].view(t.rows, t.cols)
    inside.copy_(maps[0])
    moved = Tables(fx, [inside] + maps[1:], masks)
    before = bits(pool).copy()
    L.lib.c.simq_launch_counts_reset()
    assert moved.slotted(L, good[:-1] + [t.P + 2 + span - 1], pool) != 0          # a written slot is the map's last one
    assert 'slot %d overlaps map 0' % (t.P + 2 + span - 1) in L.last_error(), L.last_error()
    assert L.launch_counts() == {} and np.array_equal(bits(pool), before)
    # the same map, no written slot touching it: accepted and read in place, the last slot of the pool among the written ones
    slots = good[:-1] + [n_slots - 1]
    assert moved.slotted(L, slots, pool) == 0, L.last_error()
    for p, s in enumerate(slots):
        assert np.array_equal(bits(pool[s]), bits(fx['want'][p])), (name, p, s)
    after = bits(pool)
    rest = sorted(set(range(n_slots)) - set(slots))
    assert np.array_equal(after[rest], before[rest])


# ---- the replay rings -----------------------------------------------------------------------------------------------------------------
def scripted_transitions(C, n, seed):
    """`n` transitions of robot group 0 of a scripted episode driven through simq.TransitionTracker: two robots, observations that are
    [96,96,C] arrays, the array handed out as next_state IS the next state (identity), terminal transitions at episode ends."""
    from simq import synth
    from simq.learner import TransitionTracker
    rng = np.random.RandomState(seed)
    pool = iter(synth.make_states(4 * n + 8, C, seed))
    tracker = TransitionTracker([[next(pool), next(pool)]])
    out = []
    while len(out) < n:
        tracker.update_action([[int(rng.randint(2 * W * W)) for _ in range(2)]])
        done = bool(rng.rand() < 0.15)
        state = [[None if done else next(pool) if rng.rand() < 0.7 else None for _ in range(2)]]
        reward = [[float(np.float32(rng.randn())) for _ in range(2)]]
        out += tracker.update_step_completed(reward, state, done)[0]
        if done:
            tracker = TransitionTracker([[next(pool), next(pool)]])
    out = out[:n]
    assert any(ns is None for _, _, _, ns in out) and any(a[3] is b[0] for a in out for b in out)
    return out


def same_batch(a, b):
    assert a.non_final_mask == b.non_final_mask
    for k in ('state', 'next_state', 'action', 'reward', 'nonfinal_pos'):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                                       y.view(torch.int32) if y.dtype == torch.float32 else y), k


def same_records(a, b):
    assert len(a.buffer) == len(b.buffer) and a.position == b.position
    for x, y in zip(a.buffer, b.buffer):
        assert (x.action, x.reward, x.next_state is None) == (y.action, y.reward, y.next_state is None)
        assert np.array_equal(bits(np.asarray(x.state)), bits(np.asarray(y.state)))
        if x.next_state is not None:
            assert np.array_equal(bits(np.asarray(x.next_state)), bits(np.asarray(y.next_state)))


class AdoptOnPush:
    """Feeds a handle ring the transitions an ndarray ring gets: an array becomes a handle (adopt) when it is first pushed, and the handle
    it got as next_state is the object pushed as the following state -- then it is let go, as the tracker lets go of it."""

    def __init__(self, ring):
        self.ring, self.waiting = ring, {}

    def handle(self, arr, keep):
        if arr is None:
            return None
        h = self.waiting.pop(id(arr), None)
        if h is None:
            h = self.ring.adopt(torch.from_numpy(arr)[None].cuda())[0]
        if keep:
            self.waiting[id(arr)] = h
        return h

    def push(self, s, a, r, ns):
        self.ring.push(self.handle(s, False), a, r, self.handle(ns, True))


def test_handle_ring_equals_the_ndarray_ring_push_by_push(S, monkeypatch):
    from simq import learner
    uploads = []
    real = learner._PinnedStaging.upload
    monkeypatch.setattr(learner._PinnedStaging, 'upload', lambda self, arr, dst: uploads.append(self) or real(self, arr, dst))
    C = 3
    host_ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=C, pool_slots=12)
    dev_ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=C, pool_slots=12)
    feeder = AdoptOnPush(dev_ring)
    for k, (s, a, r, ns) in enumerate(scripted_transitions(C, 20, 11)):
        host_ring.push(s, a, r, ns)
        feeder.push(s, a, r, ns)
        assert host_ring.observations_resident == dev_ring.observations_resident, k
        assert len(host_ring) == len(dev_ring) and host_ring.position == dev_ring.position
        if len(host_ring) >= 4 and any(t.next_state is not None for t in host_ring.buffer):
            random.seed(100 + k)
            idx = host_ring.sample_indices(4)
            if all(host_ring.buffer[i].next_state is None for i in idx):
                continue                                                  # (sample() raises for such a draw, as train.py:112 does)
            random.seed(100 + k)
            want = host_ring.sample(4)
            random.seed(100 + k)
            got = dev_ring.sample(4)
            torch.cuda.synchronize()
            same_batch(got, want)
    assert len(host_ring) == 8 and host_ring.position == 20 % 8
    same_records(dev_ring, host_ring)
    assert uploads and not [u for u in uploads if u is dev_ring._staging]


@pytest.mark.parametrize('mode', [True, 'index', False], ids=['upload_stream', 'index', 'consuming_stream'])
def test_stream_order_of_slot_writes_and_gathers(S, mode):
    from simq import synth
    C = 3
    states = synth.make_states(12, C, 21)
    ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=C, pool_slots=12, upload_stream=mode)
    ring.pool.view(torch.int32).fill_(SENT)
    staged = torch.from_numpy(states).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def busy():                                                           # tens of milliseconds of work ahead of the write
        if hasattr(torch.cuda, '_sleep'):
            torch.cuda._sleep(60_000_000)
        else:
            big = torch.empty(1 << 28, device='cuda')
            for _ in range(40):
                big.fill_(1.0)

    # 1: adopt behind a long kernel on a side stream, sample at once from the default stream
    with torch.cuda.stream(side):
        busy()
        fresh = staged[:8].clone()
        hs = ring.adopt(fresh)
    for k in range(8):
        ring.push(hs[k], k, 0.5 * k, hs[(k + 1) % 8] if k % 3 else None)
    random.seed(5)
    idx = ring.sample_indices(4)
    random.seed(5)
    batch = ring.sample(4)
    want_state = np.stack([states[i] for i in idx])
    want_next = np.stack([states[(i + 1) % 8] for i in idx if i % 3])
    # 2: release the slots (new transitions overwrite the ring, the handles go) and re-adopt them with other states right behind the
    #    gather, again behind nothing on a side stream: the batch gathered before keeps its values
    slots_before = sorted(h.slot for h in hs)
    del hs
    later = [states[8 + k] for k in range(4)]                             # (four array objects: the ring keys on identity)
    for k in range(8):
        ring.push(later[k % 4], 0, 0.0, None)
    gc.collect()
    assert ring.observations_resident == 4
    with torch.cuda.stream(side):
        again = ring.adopt(torch.flip(staged[:8], dims=[0]).contiguous())
    assert set(h.slot for h in again) & set(slots_before)
    torch.cuda.synchronize()
    assert np.array_equal(bits(batch.state), bits(want_state)) and np.array_equal(bits(batch.next_state), bits(want_next))
    for k, h in enumerate(again):
        assert np.array_equal(bits(np.asarray(h)), bits(states[7 - k]))


def test_lifetime_of_handles_that_are_never_pushed(S):
    from simq import synth
    from simq._lib import SimqError
    ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=3, pool_slots=12)
    x = torch.from_numpy(synth.make_states(4, 3, 31)).cuda()
    for explicit in (False, True):
        base = ring.observations_resident
        hs = ring.adopt(x)
        assert ring.observations_resident == base + 4
        ring.push(hs[0], 1, 0.0, hs[1])
        if explicit:
            ring.discard(hs[2:])
            ring.discard(hs[2:])                                          # (a second discard gives nothing back twice)
            with pytest.raises(SimqError, match='discarded'):
                ring.push(hs[2], 0, 0.0, None)
        else:
            del hs[2:]
            gc.collect()
        assert ring.observations_resident == base + 2
        del hs
        gc.collect()
        assert ring.observations_resident == base + 2                     # the transition keeps both slots
    free = 12 - ring.observations_resident
    with pytest.raises(SimqError, match='observation pool exhausted'):
        ring.reserve(free + 1)
    assert 12 - ring.observations_resident == free
    rest = ring.reserve(free)
    assert len(rest) == free and ring.observations_resident == 12
    del rest
    gc.collect()
    assert 12 - ring.observations_resident == free
    # a handle of another pool and a device tensor are refused, and say what to call
    other = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=3, pool_slots=12)
    h = other.adopt(x[:1])
    for bad in (h[0], x[0]):
        with pytest.raises(SimqError, match='adopt'):
            ring.push(bad, 0, 0.0, None)
        with pytest.raises(SimqError, match='adopt'):
            ring.push(np.asarray(h[0]), 0, 0.0, bad)
    assert 12 - ring.observations_resident == free and len(ring) == 2


def test_two_ring_buffer_takes_device_tensors(S, monkeypatch):
    from simq import learner, synth
    uploads = []
    real = learner._PinnedStaging.upload
    monkeypatch.setattr(learner._PinnedStaging, 'upload', lambda self, arr, dst: uploads.append(self) or real(self, arr, dst))
    C = 3
    for mode in (True, False):
        host_ring = S.DeviceReplayBuffer(8, C, upload_stream=mode)
        dev_ring = S.DeviceReplayBuffer(8, C, upload_stream=mode)
        for k, (s, a, r, ns) in enumerate(scripted_transitions(C, 11, 41)):
            host_ring.push(s, a, r, ns)
            ds = torch.from_numpy(s).cuda()
            dns = None if ns is None else torch.from_numpy(ns).cuda()
            dev_ring.push(ds[None] if k % 2 else ds, a, r, dns)
        host_ring.sync_ring()
        dev_ring.sync_ring()
        torch.cuda.synchronize()
        same_records(dev_ring, host_ring)
        for seed in (1, 2):
            random.seed(seed)
            want = host_ring.sample(4)
            random.seed(seed)
            got = dev_ring.sample(4)
            torch.cuda.synchronize()
            same_batch(got, want)
        assert not [u for u in uploads if u is dev_ring._staging]
        with pytest.raises(learner.SimqError, match='contiguous float32'):
            dev_ring.push(torch.zeros((W, W, C + 1), device='cuda'), 0, 0.0, None)


# ---- the policies ----------------------------------------------------------------------------------------------------------------------
def adopt_structure(ring, envs, keep_host):
    """The same nested [env][group][robot] lists with every ndarray but those at the flat positions `keep_host` replaced by a handle."""
    flat = [s for st in envs for g in st for s in g if s is not None]
    hs = iter(ring.adopt(torch.from_numpy(np.stack(flat)).cuda()))
    out, k = [], 0
    for st in envs:
        out.append([])
        for g in st:
            out[-1].append([])
            for s in g:
                h = None if s is None else next(hs)
                out[-1][-1].append(None if s is None else s if k in keep_host else h)
                k += s is not None
    return out


def policy_envs(C, seed):
    from simq import synth
    s = list(synth.make_states(9, C, seed))
    return [[[s[0], None, s[1]], [s[2]]], [[None, s[3], None], [None]], [[s[4], s[5], s[6]], [s[7]]]]


def same_info(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        for ga, gb in zip(a[key], b[key]):
            for xa, xb in zip(ga, gb):
                assert (xa is None) == (xb is None), key
                if xa is not None:
                    assert np.array_equal(bits(xa), bits(xb)), key


@pytest.mark.parametrize('kind', ['dqn', 'intention', 'intention_train'])
def test_policies_step_on_handles_as_on_the_arrays(S, kind):
    cfg = types.SimpleNamespace(robot_config=[{'lifting_robot': 3}, {'pushing_robot': 1}], num_input_channels=4 if kind == 'dqn' else 5,
                                final_exploration=0.01, checkpoint_path=None)
    train = kind == 'intention_train'
    pol = (S.DQNPolicy if kind == 'dqn' else S.DQNIntentionPolicy)(cfg, train=train, random_seed=3)
    for n in pol.policy_nets + getattr(pol, 'intention_nets', []):
        n.train() if train else n.eval()
    C = 4 if kind != 'intention_train' else 5                            # (train mode: the state carries the ground-truth map)
    envs = policy_envs(C, 51)
    ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=C, pool_slots=24)
    for keep_host in ((), (1, 4, 7)):                                     # every state a handle; handles and ndarrays mixed
        handles = adopt_structure(ring, envs, set(keep_host))
        for eps in (0.0, 0.5):
            random.seed(17)
            want = [pol.step(st, exploration_eps=eps) for st in envs]
            random.seed(17)
            assert [pol.step(st, exploration_eps=eps) for st in handles] == want, (kind, keep_host, eps)
            random.seed(17)
            assert pol.step_many(handles, exploration_eps=eps) == want, (kind, keep_host, eps)
        random.seed(23)
        want_a, want_info = pol.step(envs[0], exploration_eps=0.0, debug=True)
        random.seed(23)
        got_a, got_info = pol.step(handles[0], exploration_eps=0.0, debug=True)
        assert got_a == want_a
        same_info(got_info, want_info)
    assert all(n.training == train for n in pol.policy_nets + getattr(pol, 'intention_nets', []))


# ---- BatchedMapper.get_states(into=) ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def episodes(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))
    assert len(files) == 2, files
    return [mapper_oracle.load_fixture(f) for f in files]


def build_mapper(S, episodes, cfg):
    masks = {name: episodes[0]['masks'][k] for k, name in enumerate(episodes[0]['mask_names'])}
    flags = {f: cfg[f] for f in mapper_oracle.FLAGS}
    rest = {k: v for k, v in cfg.items() if k not in mapper_oracle.FLAGS}
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


def test_mapper_writes_its_states_into_pool_slots(S, L, episodes, monkeypatch):
    cfg = mapper_oracle.configurations()['full_spatial']
    bm = build_mapper(S, episodes, cfg)
    frames, robots = round_inputs(S, episodes, 0)
    bm.update(*frames)
    C = len(bm.channels)
    shuffled = [4, 1, 5, 0]
    want = np.stack([mapper_oracle.expected_state(cfg, episodes[m // 3]['rounds'][0]['images'], m % 3, 3) for m in shuffled])
    ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=C, pool_slots=12)
    ring.pool.view(torch.int32).fill_(SENT)
    ring.reserve(3)                                                       # (dropped at once: the free list is no longer in slot order)
    keep = ring.reserve(2)
    names = []
    real = L.Lib.call
    monkeypatch.setattr(L.Lib, 'call', staticmethod(lambda name, *a, **k: names.append(name) or real(name, *a, **k)))
    hs = ring.reserve(4)
    got = bm.get_states(robots, mappers=shuffled, into=hs)
    assert len(got) == 4 and all(g is h for g, h in zip(got, hs))
    assert names.count('simq_local_state_images_slots') == 1 and 'simq_local_state_images' not in names
    torch.cuda.synchronize()
    pool = bits(ring.pool)
    for p, h in enumerate(hs):
        assert np.array_equal(pool[h.slot], bits(want[p])), p
        assert np.array_equal(bits(np.asarray(h)), bits(want[p]))
    assert (pool[sorted(set(range(12)) - {h.slot for h in hs})] == SENT).all()
    # without into= the call is the one it always was
    del names[:]
    dense = bm.get_states(robots, mappers=shuffled)
    assert names.count('simq_local_state_images') == 1 and 'simq_local_state_images_slots' not in names
    assert np.array_equal(bits(dense), bits(want))
    # the handles are transitions like any other
    ring.push(hs[0], 3, 1.0, hs[1])
    ring.push(hs[1], 4, 0.0, None)
    random.seed(1)
    idx = ring.sample_indices(2)
    random.seed(1)
    batch = ring.sample(2)
    torch.cuda.synchronize()
    assert np.array_equal(bits(batch.state), pool[[int(ring.buffer[i].state) for i in idx]])
    # simq.local_state_images(into=) on its own fixture; without into= its call is unchanged as well
    name, fx = local_fixtures(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))[0]
    from simq.local_maps import RobotStamp
    envs = {e: [RobotStamp(*r) for r in rs] for e, rs in fx['robot_poses'].items()}
    poses, stamps = [(s['position'], s['heading']) for s in fx['states']], [envs[s['env']] for s in fx['states']]
    ring2 = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=len(fx['channels']), pool_slots=len(poses) + 3)
    del names[:]
    h2 = S.local_state_images(torch.from_numpy(fx['maps']).cuda(), fx['channels'], poses, robots=stamps, masks=fx['masks'], into=ring2.reserve(len(poses)))
    assert names == ['simq_local_state_images_slots']
    del names[:]
    d2 = S.local_state_images(torch.from_numpy(fx['maps']).cuda(), fx['channels'], poses, robots=stamps, masks=fx['masks'])
    assert names == ['simq_local_state_images']
    for p, h in enumerate(h2):
        assert np.array_equal(bits(np.asarray(h)), bits(fx['want'][p])) and np.array_equal(bits(d2[p]), bits(fx['want'][p]))
    del keep


def test_mapper_without_an_update_raises_after_writing(S, episodes):
    from simq._lib import SimqError
    cfg = mapper_oracle.configurations()['full_spatial']
    fresh = build_mapper(S, episodes, cfg)
    _, robots = round_inputs(S, episodes, 0)
    ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=len(fresh.channels), pool_slots=8)
    ring.pool.view(torch.int32).fill_(SENT)
    hs = ring.reserve(6)
    with pytest.raises(SimqError, match=r'status \[4, 4, 4, 4, 4, 4, 4, 4\]'):
        fresh.get_states(robots, into=hs)
    torch.cuda.synchronize()
    pool = bits(ring.pool)
    assert all((pool[h.slot] != SENT).all() for h in hs)                  # every state was written before the one read-back
    assert (pool[sorted(set(range(8)) - {h.slot for h in hs})] == SENT).all()
    # the argument checks come before any launch
    with pytest.raises(ValueError, match='into'):
        fresh.get_states(robots, into=hs, out=torch.empty((6, W, W, len(fresh.channels)), device='cuda'))
    with pytest.raises(ValueError, match='5 handles for 6 states'):
        fresh.get_states(robots, into=hs[:5])
    wrong = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=len(fresh.channels) + 1, pool_slots=8)
    with pytest.raises(ValueError, match='channels'):
        fresh.get_states(robots, into=wrong.reserve(6))


# ---- checkpoints and visualisations ------------------------------------------------------------------------------------------------
def test_handle_filled_ring_saves_loads_and_resumes(S, tmp_path):
    C = 4
    transitions = scripted_transitions(C, 11, 61)
    host_ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=C, pool_slots=12)
    dev_ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=C, pool_slots=12)
    feeder = AdoptOnPush(dev_ring)
    for s, a, r, ns in transitions:
        host_ring.push(s, a, r, ns)
        feeder.push(s, a, r, ns)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9)
    path = S.save_checkpoint(tmp_path, 7, 2, [opt], [dev_ring])
    loaded = S.load_checkpoint(path)['replay_buffers'][0]
    same_records(loaded, host_ring)
    alias = [(i, j) for i, x in enumerate(host_ring.buffer) for j, y in enumerate(host_ring.buffer)
             if x.next_state is not None and int(x.next_state) == int(y.state)]
    assert alias and all(loaded.buffer[i].next_state is loaded.buffer[j].state for i, j in alias)      # one array, pickled once
    from simq import checkpoint
    t, e, rings = checkpoint.resume(path, [opt], device='cuda')
    assert (t, e) == (7, 2)
    same_records(rings[0], host_ring)
    random.seed(9)
    want = host_ring.sample(4)
    random.seed(9)
    got = rings[0].sample(4)
    random.seed(9)
    mine = dev_ring.sample(4)
    torch.cuda.synchronize()
    same_batch(got, want)
    same_batch(mine, want)
    # the resumed ring goes on taking handles
    h = rings[0].adopt(torch.from_numpy(transitions[0][0])[None].cuda())
    rings[0].push(h[0], 1, 0.0, None)
    assert np.array_equal(bits(np.asarray(rings[0].buffer[(rings[0].position - 1) % 8].state)), bits(transitions[0][0]))


def test_a_handle_renders_as_its_array(S):
    from simq import synth
    states = synth.make_states(2, 4, 71)
    outputs = np.random.RandomState(72).randn(2, 2, W, W).astype(np.float32)
    ring = S.AliasedDeviceReplayBuffer(capacity=8, num_input_channels=4, pool_slots=12)
    hs = ring.adopt(torch.from_numpy(states).cuda())
    want = S.state_output_visualizations(list(states), list(outputs))
    got = S.state_output_visualizations(hs, list(outputs))
    ring.push(hs[0], 0, 0.0, hs[1])
    record = S.state_output_visualizations([ring.buffer[0].state, ring.buffer[0].next_state], list(outputs))
    torch.cuda.synchronize()
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(record), bits(want))
    assert np.array_equal(bits(np.asarray(hs[1])), bits(states[1])) and np.asarray(hs[0], dtype=np.float64).dtype == np.float64
