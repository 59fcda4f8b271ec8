"""GPU: states of several robot groups written into their pools by one launch -- simq_local_state_images_pools on
its own, then `pools=` through simq.local_state_images, BatchedMapper.get_states in both its forms, the rings' stream order and a
TransitionTracker episode.  The entry computes what the slots entries compute and only places it: every comparison is bit for bit."""
import ctypes
import gc
import random
import types

import numpy as np
import pytest
import torch

import mapper_oracle
import test_gpu_bf16_states as tb
import test_gpu_device_transitions as tdt

pytestmark = pytest.mark.gpu

W = 96
SENT32, SENT16 = tb.SENT32, tb.SENT16
CFG = 'full_spatial'
SHUFFLED = [4, 1, 5, 0]


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


@pytest.fixture(scope='module')
def L(S):
    from simq import _lib
    return _lib


@pytest.fixture(scope='module')
def fixtures(golden_dir):
    """[(name, fixture, device maps, device masks, the fp32 states of the dense entry)], made once and only read."""
    from simq import _lib
    out = []
    for name, fx in tdt.local_fixtures(golden_dir):
        maps, masks = tdt.device_inputs(fx)
        out.append((name, fx, maps, masks, tdt.Tables(fx, maps, masks).dense(_lib)))
    return out


def sentinel(dtype, *shape):
    return tb.sentinel16(*shape) if dtype == torch.bfloat16 else tb.sentinel32(*shape)


def raw(t):
    """The bits of a pool tensor: uint16 of a bf16 one, uint32 of an fp32 one."""
    return tb.bits16(t) if t.dtype == torch.bfloat16 else tb.bits32(t)


def rounded_like(pool, f32):
    """The bits a pool of `pool`'s type holds for the fp32 states `f32`: themselves, or rounded once on the host."""
    return tb.bits16(tb.host_bf16(f32)) if pool.dtype == torch.bfloat16 else tb.bits32(f32)


def untouched(pool, written):
    rest = sorted(set(range(pool.shape[0])) - set(written))
    return (raw(pool)[rest] == (SENT16 if pool.dtype == torch.bfloat16 else SENT32)).all()


def pooled(L, t, pools, dests):
    """simq_local_state_images_pools of the tables `t` into the pool tensors `pools`; dests: (pool, slot) per problem."""
    need = L.lib.c.simq_local_state_pools_desc_bytes(t.G, t.n_robots, t.P, t.C, len(pools))
    assert need == L.lib.c.simq_local_state_slots_desc_bytes(t.G, t.n_robots, t.P, t.C) + 24 * len(pools) + 16 * t.P
    table = (L.LocalPool * len(pools))(*[L.LocalPool(q.data_ptr(), q.shape[0], int(q.dtype == torch.bfloat16), 0) for q in pools])
    a_dests = (L.LocalDest * len(dests))(*[L.LocalDest(slot, pool, 0) for pool, slot in dests])
    rc = L.lib.c.simq_local_state_images_pools(*t.head(), table, len(pools), a_dests, L.ptr(tb.scratch(need)), ctypes.c_int64(need), L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def spread(rng, P, pools):
    """Problems round-robin over the pools, each pool's slots shuffled (slot 0 and its last slot among them)."""
    count = [len(range(k, P, len(pools))) for k in range(len(pools))]
    slots = [iter(tdt.shuffled_slots(rng, n, q.shape[0]) if n else []) for n, q in zip(count, pools)]
    return [(p % len(pools), next(slots[p % len(pools)])) for p in range(P)]


def check_pooled(L, t, f32, pools, dests, tag):
    L.lib.c.simq_launch_counts_reset()
    assert pooled(L, t, pools, dests) == 0, L.last_error()
    assert L.launch_counts() == {'local_state_pools': 1}
    for p, (k, s) in enumerate(dests):
        assert np.array_equal(raw(pools[k][s]), rounded_like(pools[k], f32[p])), (tag, p, k, s)
    for k, q in enumerate(pools):
        assert untouched(q, [s for kk, s in dests if kk == k]), (tag, k)


# ---- 1. the raw ABI on both fixtures ------------------------------------------------------------------------------------------------
def test_pools_entry_equals_the_golden_states_and_the_slots_entries(L, fixtures):
    for name, fx, maps, masks, f32 in fixtures:
        t = tdt.Tables(fx, maps, masks)
        assert np.array_equal(tb.bits32(f32), tb.bits32(fx['want']))                 # the dense entry gives the golden states
        rng = np.random.RandomState(7 * t.P + t.C)
        n = [len(range(k, t.P, 3)) for k in range(3)]
        pools = [sentinel(torch.float32, n[0] + 7, W, W, t.C), sentinel(torch.bfloat16, n[1] + 5, W, W, t.C), sentinel(torch.float32, n[2] + 3, W, W, t.C)]
        dests = spread(rng, t.P, pools)
        check_pooled(L, t, fx['want'], pools, dests, name)
        # one pool: the bytes of simq_local_state_images_slots, and of _slots_bf16, in the whole pool
        for dtype in (torch.float32, torch.bfloat16):
            slots = tdt.shuffled_slots(rng, t.P, t.P + 5)
            mine, theirs = sentinel(dtype, t.P + 5, W, W, t.C), sentinel(dtype, t.P + 5, W, W, t.C)
            check_pooled(L, t, f32, [mine], [(0, s) for s in slots], (name, dtype))
            if dtype == torch.float32:
                assert t.slotted(L, slots, theirs) == 0, L.last_error()
            else:
                tb.slotted16(L, t, slots, theirs)
            assert np.array_equal(raw(mine), raw(theirs)), (name, dtype)


def test_pools_entry_refusals_write_nothing_and_launch_nothing(L, fixtures):
    name, fx, maps, masks, f32 = fixtures[0]
    t = tdt.Tables(fx, maps, masks)
    pools = [sentinel(torch.float32, t.P + 2, W, W, t.C), sentinel(torch.bfloat16, t.P + 2, W, W, t.C)]
    good = [(p % 2, p) for p in range(t.P)]

    def refused(match, dests, pools=pools):
        L.lib.c.simq_launch_counts_reset()
        assert pooled(L, t, pools, dests) != 0
        assert match in L.last_error(), (match, L.last_error())
        assert L.launch_counts() == {} and all(untouched(q, []) for q in pools)

    refused('pool 2 outside the 2 given', [(2, 0)] + good[1:])
    refused('slot %d outside pool 0 of %d' % (t.P + 2, t.P + 2), [(0, t.P + 2)] + good[1:])
    refused('slot -1 outside pool 1 of', good[:-1] + [(1, -1)])
    if t.P >= 3:
        refused('slot 2 of pool 0 is named twice', [(0, 2)] + good[1:])
    refused('pool 0 overlaps pool 1', good, pools=[pools[0], pools[0][1:]])
    check_pooled(L, t, f32, pools, good, name)


# ---- 2. the smallest shapes that can go wrong ---------------------------------------------------------------------------------------
def test_pools_entry_at_its_smallest_shapes(L, fixtures):
    name, fx, maps, masks, f32 = fixtures[0]
    last = len(fx['states']) - 1
    # P = 1, into either type of a table of two
    t = tdt.Tables(fx, maps, masks, problems=[last])
    for k in (0, 1):
        pools = [sentinel(torch.float32, 3, W, W, t.C), sentinel(torch.bfloat16, 3, W, W, t.C)]
        check_pooled(L, t, f32[last:], pools, [(k, 2 - k)], (name, 'P=1', k))
    # C = 1
    t = tdt.Tables(fx, maps, masks, channels=fx['channels'][:1])
    pools = [sentinel(torch.bfloat16, t.P + 1, W, W, 1), sentinel(torch.float32, t.P + 1, W, W, 1)]
    check_pooled(L, t, f32[..., :1], pools, [(p % 2, t.P - p) for p in range(t.P)], (name, 'C=1'))
    # C = 64 constant channels (no map named), odd slots of a bf16 pool among the destinations
    values = [float(np.float32(0.37 * k - 5)) for k in range(64)]
    t = tdt.Tables(fx, [], masks, channels=[('constant', v) for v in values], problems=[0, last])
    want = np.broadcast_to(np.asarray(values, np.float32), (2, W, W, 64))
    pools = [sentinel(torch.bfloat16, 4, W, W, 64), sentinel(torch.float32, 2, W, W, 64)]
    check_pooled(L, t, want, pools, [(0, 3), (0, 1)], (name, 'C=64 bf16'))
    pools = [sentinel(torch.bfloat16, 4, W, W, 64), sentinel(torch.float32, 2, W, W, 64)]
    check_pooled(L, t, want, pools, [(1, 1), (0, 3)], (name, 'C=64 mixed'))
    # C = 5 into a bf16 pool that begins 2 bytes behind a 4-byte boundary: every slot begins on an odd element
    five = (list(fx['channels']) + [('constant', 1.5)] * 5)[:5]
    t = tdt.Tables(fx, maps, masks, channels=five)
    want = t.dense(L)
    store = sentinel(torch.bfloat16, (t.P + 3) * W * W * 5 + 2)
    odd = store[1:1 + (t.P + 3) * W * W * 5].view(t.P + 3, W, W, 5)
    assert odd.data_ptr() % 4 == 2 and (W * W * 5 * 2) % 4 == 0
    pools = [odd, sentinel(torch.float32, t.P + 1, W, W, 5)]
    check_pooled(L, t, want, pools, [(p % 2, t.P + 2 - p if p % 2 == 0 else p) for p in range(t.P)], (name, 'C=5'))
    assert (tb.bits16(store[:1]) == SENT16).all() and (tb.bits16(store[-1:]) == SENT16).all()


def test_a_map_in_an_unwritten_slot_of_a_listed_pool_is_read_in_place(L, fixtures):
    name, fx, maps, masks, f32 = fixtures[0]
    t = tdt.Tables(fx, maps, masks)
    item, size = W * W * t.C, t.rows * t.cols
    span = -(-size // item)
    n_slots = t.P + 3 + span
    pool, other = sentinel(torch.float32, n_slots, W, W, t.C), sentinel(torch.bfloat16, t.P + 1, W, W, t.C)
    inside = pool.view(-1)[(t.P + 1) * item:(t.P + 1) * item + size].view(t.rows, t.cols)       # slots P + 1 .. P + span
    inside.copy_(maps[0])
    moved = tdt.Tables(fx, [inside] + maps[1:], masks)
    before = raw(pool).copy()
    dests = [(p % 2, p) for p in range(t.P)]
    L.lib.c.simq_launch_counts_reset()
    assert pooled(L, moved, [pool, other], dests[:-1] + [(0, t.P + span)]) != 0                 # a written slot is the map's last one
    assert 'slot %d of pool 0 overlaps map 0' % (t.P + span) in L.last_error(), L.last_error()
    assert L.launch_counts() == {} and np.array_equal(raw(pool), before) and untouched(other, [])
    dests = dests[:-1] + [(0, n_slots - 1)]                                                     # ... the pool's last slot instead
    assert pooled(L, moved, [pool, other], dests) == 0, L.last_error()
    for p, (k, s) in enumerate(dests):
        q = (pool, other)[k]
        assert np.array_equal(raw(q[s]), rounded_like(q, f32[p])), (p, k, s)
    rest = sorted(set(range(n_slots)) - {s for k, s in dests if k == 0})
    assert np.array_equal(raw(pool)[rest], before[rest]) and untouched(other, [s for k, s in dests if k == 1])


def test_a_listed_pool_that_receives_nothing_is_not_touched(S, L, fixtures, monkeypatch):
    from simq import learner
    from simq.local_maps import RobotStamp
    name, fx, maps, masks, f32 = fixtures[0]
    envs = {e: [RobotStamp(*r) for r in rs] for e, rs in fx['robot_poses'].items()}
    poses, stamps = [(s['position'], s['heading']) for s in fx['states']], [envs[s['env']] for s in fx['states']]
    P, C = len(poses), len(fx['channels'])
    a = S.AliasedDeviceReplayBuffer(8, C, pool_slots=P + 3)
    b = S.AliasedDeviceReplayBuffer(8, C, pool_slots=P + 3, dtype='bf16')
    idle = S.AliasedDeviceReplayBuffer(8, C, pool_slots=4)
    for r in (a, b, idle):
        r.pool.view(torch.int16).fill_(SENT16) if r.pool.dtype == torch.bfloat16 else r.pool.view(torch.int32).fill_(SENT32)
    torch.cuda.synchronize()
    hs = [(a, b)[p % 2].reserve(1)[0] for p in range(P)]
    names = []
    real = L.Lib.call
    monkeypatch.setattr(L.Lib, 'call', staticmethod(lambda name, *x, **k: names.append(name) or real(name, *x, **k)))
    got = S.local_state_images(torch.stack(maps), fx['channels'], poses, robots=stamps, masks=fx['masks'], into=hs, pools=[idle, a, b])
    assert names == ['simq_local_state_images_pools'] and all(g is h for g, h in zip(got, hs))
    torch.cuda.synchronize()
    for p, h in enumerate(hs):
        assert np.array_equal(raw(h.pool.pool[h.slot]), rounded_like(h.pool.pool, f32[p])), p
    for r in (a, b):
        assert untouched(r.pool, [h.slot for h in hs if h.pool is r]) and len(r._write_events) == 1
    assert untouched(idle.pool, []) and idle._write_events is learner.DeviceReplayBuffer._write_events and not idle._write_events
    # one listed pool is the same entry
    del names[:]
    S.local_state_images(torch.stack(maps), fx['channels'], poses[:1], robots=stamps[:1], masks=fx['masks'], into=a.reserve(1), pools=[a])
    assert names == ['simq_local_state_images_pools']


# ---- 3. the mapper, end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def episodes(golden_dir):
    import glob
    import os
    files = sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))
    assert len(files) == 2, files
    return [mapper_oracle.load_fixture(f) for f in files]


@pytest.fixture(scope='module')
def updated(S, episodes):
    """{configuration name: (the object after the update of round 0, the robots of round 0)}, made once and only read."""
    made = {}

    def get(name):
        if name not in made:
            bm = tdt.build_mapper(S, episodes, mapper_oracle.configurations()[name])
            frames, robots = tdt.round_inputs(S, episodes, 0)
            bm.update(*frames)
            made[name] = (bm, robots)
        return made[name]
    return get


def group_of(episodes, m):
    return episodes[m // 3]['groups'][m % 3]


def group_rings(S, episodes, C, dtypes=('fp32', 'bf16'), slots=12, capacity=8, **kw):
    """{group: its ring}, in the order of the groups: fp32 for the first group, bf16 for the second; every pool filled with its sentinel."""
    groups = sorted({g for ep in episodes for g in ep['groups']})
    assert len(groups) == 2, groups
    rings = {g: S.AliasedDeviceReplayBuffer(capacity, C, pool_slots=slots, dtype=d, **kw) for g, d in zip(groups, dtypes)}
    for r in rings.values():
        r.pool.view(torch.int16).fill_(SENT16) if r.pool.dtype == torch.bfloat16 else r.pool.view(torch.int32).fill_(SENT32)
        r.reserve(3)                                                            # (dropped at once: the free list is no longer in slot order)
    torch.cuda.synchronize()
    return rings


def expected(episodes, name, mappers, t=0):
    cfg = mapper_oracle.configurations()[name]
    return np.stack([mapper_oracle.expected_state(cfg, episodes[m // 3]['rounds'][t]['images'], m % 3, 3) for m in mappers])


def table_bytes(arg):
    return bytes(arg) if isinstance(arg, ctypes.Array) else arg.tobytes() if hasattr(arg, 'tobytes') else None


def test_mapper_writes_the_states_of_both_groups_in_one_launch(S, L, episodes, updated, monkeypatch):
    bm, robots = updated(CFG)
    C = len(bm.channels)
    want = expected(episodes, CFG, SHUFFLED)
    assert len({group_of(episodes, m) for m in SHUFFLED}) == 2
    calls = []
    real = L.Lib.call
    monkeypatch.setattr(L.Lib, 'call', staticmethod(lambda name, *a, **k: calls.append((name, a)) or real(name, *a, **k)))
    seen = []
    for form in (robots, S.RobotArrays.from_states(bm, robots)):
        rings = group_rings(S, episodes, C)
        hs = [rings[group_of(episodes, m)].reserve(1)[0] for m in SHUFFLED]
        del calls[:]
        L.lib.c.simq_launch_counts_reset()
        got = bm.get_states(form, mappers=SHUFFLED, into=hs, pools=list(rings.values()))
        assert len(got) == 4 and all(g is h for g, h in zip(got, hs))
        state_calls = [(n, a) for n, a in calls if n.startswith('simq_local_state')]
        assert [n for n, _ in state_calls] == ['simq_local_state_images_pools']
        counts = L.launch_counts()
        assert counts.get('local_state_pools') == 1 and not [k for k in counts if k.startswith('local_state') and k != 'local_state_pools']
        torch.cuda.synchronize()
        for p, h in enumerate(hs):
            assert h.pool is rings[group_of(episodes, SHUFFLED[p])]
            assert np.array_equal(raw(h.pool.pool[h.slot]), rounded_like(h.pool.pool, want[p])), p
            assert np.array_equal(tb.bits32(np.asarray(h)), tb.bits32(want[p] if h.pool.pool.dtype == torch.float32 else tb.rounded(want[p]))), p
        for r in rings.values():
            assert untouched(r.pool, [h.slot for h in hs if h.pool is r])
        seen.append((state_calls[0][1], rings, hs))
    # both forms hand the library the same descriptors (section 19): counts, robots, problems, channels, pool types and destinations
    (a, _, ha), (b, _, hb) = seen
    assert [(h.slot, group_of(episodes, m)) for h, m in zip(ha, SHUFFLED)] == [(h.slot, group_of(episodes, m)) for h, m in zip(hb, SHUFFLED)]
    for k in (1, 3, 5, 7, 9, 11):
        assert a[k] == b[k], k
    for k in (4, 6, 8, 12):
        assert table_bytes(a[k]) == table_bytes(b[k]) and table_bytes(a[k]), k
    assert [(q.pool_slots, q.bf16) for q in a[10]] == [(q.pool_slots, q.bf16) for q in b[10]] == [(12, 0), (12, 1)]
    # ... and the per-group into= calls on a second pair of rings give the same rows
    monkeypatch.undo()
    rings2 = group_rings(S, episodes, C)
    row = {}
    for g, ring in rings2.items():
        mine = [m for m in SHUFFLED if group_of(episodes, m) == g]
        for m, h in zip(mine, bm.get_states(robots, mappers=mine, into=ring.reserve(len(mine)))):
            row[m] = h
    torch.cuda.synchronize()
    _, rings, hs = seen[0]
    for m, h in zip(SHUFFLED, hs):
        assert h.slot == row[m].slot and np.array_equal(raw(h.pool.pool[h.slot]), raw(row[m].pool.pool[row[m].slot])), m
    for g in rings:
        assert np.array_equal(raw(rings[g].pool), raw(rings2[g].pool)), g


# ---- 4. stream order ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [True, 'index', False], ids=['upload_stream', 'index', 'consuming_stream'])
def test_stream_order_of_a_pools_write_and_the_gathers_of_both_rings(S, episodes, updated, mode):
    name = 'use_intention_map_ramp'                                          # (no distance images: the call ends without a read-back)
    bm, robots = updated(name)
    ra = S.RobotArrays.from_states(bm, robots)
    C = len(bm.channels)
    order, flipped = list(range(6)), list(range(5, -1, -1))
    want = expected(episodes, name, order)
    rings = group_rings(S, episodes, C, slots=8, capacity=4, upload_stream=mode)
    pools = list(rings.values())
    side = torch.cuda.Stream()

    def reserve(mappers):
        return [rings[group_of(episodes, m)].reserve(1)[0] for m in mappers]

    # 1: the write behind a long kernel on a side stream, both rings sampled at once from the default stream
    with torch.cuda.stream(side):
        if hasattr(torch.cuda, '_sleep'):                                   # tens of milliseconds of work ahead of the write
            torch.cuda._sleep(60_000_000)
        else:
            big = torch.empty(1 << 28, device='cuda')
            for _ in range(40):
                big.fill_(1.0)
        hs = bm.get_states(ra, mappers=order, into=reserve(order), pools=pools)
    mine = {g: [m for m in order if group_of(episodes, m) == g] for g in rings}
    batches = {}
    for g, ring in rings.items():
        of = [hs[m] for m in mine[g]]
        n = len(of)
        assert 2 <= n <= 4                                                   # (every transition is sampled: one with a next state among them)
        for k in range(n):
            ring.push(of[k], k, 0.5 * k, of[(k + 1) % n] if k % 2 else None)
    for g, ring in rings.items():
        random.seed(5)
        idx = ring.sample_indices(len(mine[g]))
        random.seed(5)
        batches[g] = (ring.sample(len(mine[g])), idx)
    # 2: the slots released (other transitions overwrite the rings, the handles go) and rewritten with other states right behind the
    #    gathers, on the side stream again: the batches gathered before keep their values
    before = {g: sorted(hs[m].slot for m in mine[g]) for g in rings}
    del hs, of
    later = [np.full((W, W, C), 0.25 * k, np.float32) for k in range(2)]
    for ring in rings.values():
        for k in range(4):
            ring.push(later[k % 2], 0, 0.0, None)
    gc.collect()
    assert all(r.observations_resident == 2 for r in rings.values())
    with torch.cuda.stream(side):
        again = bm.get_states(robots, mappers=flipped, into=reserve(flipped), pools=pools)
    assert all(set(h.slot for h in again if h.pool is rings[g]) & set(before[g]) for g in rings)
    torch.cuda.synchronize()
    for g, ring in rings.items():
        batch, idx = batches[g]
        n = len(mine[g])
        rows = want[mine[g]]
        assert np.array_equal(raw(batch.state), rounded_like(ring.pool, np.stack([rows[i] for i in idx]))), (mode, g)
        assert np.array_equal(raw(batch.next_state), rounded_like(ring.pool, np.stack([rows[(i + 1) % n] for i in idx if i % 2]))), (mode, g)
    for m, h in zip(flipped, again):
        assert np.array_equal(raw(h.pool.pool[h.slot]), rounded_like(h.pool.pool, want[m])), m


# ---- 5. a TransitionTracker episode over two groups ---------------------------------------------------------------------------------
def collect(S, episodes, bm, policy, one_call):
    """A scripted episode of both environments: per round get_states for the robots that decide, step_many on the handles, push of the
    transitions the trackers complete.  one_call: one get_states(pools=) per round; else one get_states(into=) per group."""
    C = len(bm.channels)
    groups = sorted({g for ep in episodes for g in ep['groups']})
    rings = {g: S.AliasedDeviceReplayBuffer(16, C, pool_slots=40) for g in groups}
    members = [{g: [r for r, x in enumerate(ep['groups']) if x == g] for g in groups} for ep in episodes]
    trackers, actions_seen = None, []
    rounds = min(4, min(len(ep['rounds']) for ep in episodes))
    for t in range(rounds):
        robots = tdt.round_inputs(S, episodes, t)[1]
        deciding = [m for m in range(6) if t == 0 or (m + t) % 3 != 0]          # (a robot that does not decide keeps its state: None)
        if one_call:
            hs = [rings[group_of(episodes, m)].reserve(1)[0] for m in deciding]
            of = dict(zip(deciding, bm.get_states(robots, mappers=deciding, into=hs, pools=list(rings.values()))))
        else:
            of = {}
            for g in groups:
                mine = [m for m in deciding if group_of(episodes, m) == g]
                if mine:                                                        # (round 1: nobody of the second group decides)
                    of.update(zip(mine, bm.get_states(robots, mappers=mine, into=rings[g].reserve(len(mine)))))
        states = [[[of.get(3 * e + r) for r in members[e][g]] for g in groups] for e in range(2)]
        random.seed(300 + t)
        actions = policy.step_many(states, exploration_eps=0.2)
        actions_seen.append(actions)
        if trackers is None:
            trackers = [S.TransitionTracker(st) for st in states]
        else:
            for e, tracker in enumerate(trackers):
                reward = [[0.25 * (t + 1) for _ in g] for g in states[e]]
                for i, transitions in enumerate(tracker.update_step_completed(reward, states[e], t == rounds - 1)):
                    for transition in transitions:
                        rings[groups[i]].push(*transition)
        for e, tracker in enumerate(trackers):
            tracker.update_action(actions[e])
    return rings, actions_seen


def test_a_two_group_episode_collects_the_same_with_one_call_per_round(S, episodes, updated):
    bm, _ = updated(CFG)
    fx = episodes[0]
    groups = sorted(set(fx['groups']))
    cfg = types.SimpleNamespace(robot_config=[{fx['types'][fx['groups'].index(g)]: fx['groups'].count(g)} for g in groups],
                                num_input_channels=len(bm.channels), final_exploration=0.01, checkpoint_path=None)
    policy = S.DQNPolicy(cfg, train=False, random_seed=1)
    for net in policy.policy_nets:
        net.eval()
    per_group, want_actions = collect(S, episodes, bm, policy, False)
    one_call, got_actions = collect(S, episodes, bm, policy, True)
    assert got_actions == want_actions
    assert sum(len(r) for r in per_group.values()) > 0
    for g in per_group:
        a, b = per_group[g], one_call[g]
        assert len(a) == len(b) and a.position == b.position and a.observations_resident == b.observations_resident, g
        tdt.same_records(b, a)
        if len(a) >= 2 and any(x.next_state is not None for x in a.buffer):
            for seed in (1, 2, 3):
                random.seed(seed)
                idx = a.sample_indices(2)
                if all(a.buffer[i].next_state is None for i in idx):
                    continue
                random.seed(seed)
                want = a.sample(2)
                random.seed(seed)
                got = b.sample(2)
                torch.cuda.synchronize()
                tdt.same_batch(got, want)
