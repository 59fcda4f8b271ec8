"""GPU: a replay pool of bf16 states.  The contract is stated without a tolerance: a bf16 state is the round-to-
nearest-even bf16 of the fp32 state the existing code produces; every consumer given bf16 states returns what it returns today on those
rounded values as fp32; and a plan whose first convolution runs stem_conv_bf16 returns that on the UNROUNDED fp32 states as well.  Every
comparison below is bit for bit, except the BatchNorm sums of the first convolution (fp64 atomics in arbitrary order in both forms).
The host reference of the rounding -- torch's conversion on the CPU -- is pinned by tests/test_bf16_states_cpu.py."""
import ctypes
import os
import random
import types

import numpy as np
import pytest
import torch

import mapper_oracle
import test_gpu_device_transitions as tdt
from test_bf16_states_cpu import crafted_values

pytestmark = pytest.mark.gpu

W = 96
SENT16 = 0x7FD5                      # a bf16 NaN with a payload: any element written, or left unwritten, shows
SENT32 = 0x7FC0BEEF


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


@pytest.fixture(scope='module')
def L(S):
    from simq import _lib
    return _lib


def host_bf16(a):
    """The reference rounding: torch's float32 -> bfloat16 on the host (a CPU bfloat16 tensor)."""
    a = a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return a.to(torch.bfloat16)


def bits16(t):
    """bf16 tensor (any device) -> uint16 ndarray."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bits32(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def widen(b16):
    """uint16 bf16 bits -> the float32 they are exactly."""
    return (np.asarray(b16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def same_bf16(got, want, what=''):
    """Equal bits wherever the reference is not a NaN; NaN at the same places (a NaN's payload is not part of the contract)."""
    got, want = bits16(got), bits16(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(widen(got)), np.isnan(widen(want))
    assert np.array_equal(nan_g, nan_w), what
    assert np.array_equal(got[~nan_w], want[~nan_w]), what


def sentinel16(*shape):
    t = torch.empty(shape, dtype=torch.bfloat16, device='cuda')
    t.view(torch.int16).fill_(SENT16)
    return t


def sentinel32(*shape):
    t = torch.empty(shape, dtype=torch.float32, device='cuda')
    t.view(torch.int32).fill_(SENT32)
    return t


def scratch(nbytes):
    return torch.full((int(nbytes),), 0xA5, dtype=torch.uint8, device='cuda')


# ---- 1. the conversions ---------------------------------------------------------------------------------------------------------------
def conversion_values():
    rng = np.random.RandomState(11)
    rand = rng.randint(0, 1 << 32, size=10000, dtype=np.uint64).astype(np.uint32).view(np.float32)    # every exponent, NaNs among them
    return np.concatenate([crafted_values(), rand])


@pytest.mark.parametrize('offsets', [(0, 0), (1, 1), (1, 0), (0, 1)], ids=['aligned', 'both+1', 'src+1', 'dst+1'])
def test_conversions_round_to_nearest_even_and_widen_exactly(L, offsets):
    values = conversion_values()
    so, do = offsets
    for n in (1, 7, 8, 9, 4097, values.size):
        v = values[:n]
        src = torch.zeros(n + 24, dtype=torch.float32, device='cuda')           # (torch allocations start on 256-byte boundaries)
        src[so:so + n] = torch.from_numpy(v).cuda()
        dst = sentinel16(n + 24)
        L.lib.c.simq_launch_counts_reset()
        L.lib.call('simq_states_to_bf16', L.ptr(src[so:]), L.ptr(dst[do:]), n, L.stream_ptr())
        assert L.launch_counts() == {'states_to_bf16': 1}
        same_bf16(dst[do:do + n], host_bf16(v), ('to_bf16', n, offsets))
        rest = np.concatenate([bits16(dst[:do]), bits16(dst[do + n:])])
        assert (rest == SENT16).all(), ('to_bf16 wrote outside', n, offsets)
        # the round trip: widening what was just made, at the mirrored offsets, gives exactly those bits as the high halves
        back = sentinel32(n + 24)
        L.lib.call('simq_states_to_f32', L.ptr(dst[do:]), L.ptr(back[so:]), n, L.stream_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(bits32(back[so:so + n]), bits16(dst[do:do + n]).astype(np.uint32) << 16), ('to_f32', n, offsets)
        assert (np.concatenate([bits32(back[:so]), bits32(back[so + n:])]) == SENT32).all(), ('to_f32 wrote outside', n, offsets)
        again = sentinel16(n + 24)
        L.lib.call('simq_states_to_bf16', L.ptr(back[so:]), L.ptr(again[do:]), n, L.stream_ptr())
        ok = ~np.isnan(widen(bits16(dst[do:do + n])))
        assert np.array_equal(bits16(again[do:do + n])[ok], bits16(dst[do:do + n])[ok])       # rounding is the identity on bf16 values


# ---- 2, 3. the first convolution and its weight gradient over bf16 input ----------------------------------------------------------------
def stem_inputs(cin, B, seed):
    rng = np.random.RandomState(seed)
    x = (rng.randn(B, W, W, cin) * np.exp(rng.uniform(-3, 3, (B, W, W, cin)))).astype(np.float32)
    w = (rng.randn(64, 7, 7, cin) * 0.1).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()


def stem_fwd(L, entry, x, w, B, cin, stats=True):
    y = sentinel16(B, 48, 48, 64)
    st = torch.zeros(128, dtype=torch.float64, device='cuda') if stats else None
    L.lib.call(entry, L.ptr(x), L.ptr(w), L.ptr(y), B, W, W, cin, L.ptr(st), L.ptr(scratch(58368)), L.stream_ptr())
    torch.cuda.synchronize()
    return y, st


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('cin', [3, 4, 5, 9])
def test_stem_forward_over_bf16_states(S, L, cin, B):
    from simq.fcn import to_bf16, to_f32
    x, w = stem_inputs(cin, B, 100 + 10 * cin + B)
    x16 = to_bf16(x)
    same_bf16(x16, host_bf16(x), 'states')
    assert not torch.equal(to_f32(x16), x)                                       # (the inputs are not bf16 values to begin with)
    L.lib.c.simq_launch_counts_reset()
    y16, s16 = stem_fwd(L, 'simq_conv2d_fwd_stem_bf16_x16', x16, w, B, cin)
    assert L.launch_counts().get('stem_conv_bf16_x16') == 1 and 'stem_conv_bf16' not in L.launch_counts()
    y_r, s_r = stem_fwd(L, 'simq_conv2d_fwd_stem_bf16', to_f32(x16), w, B, cin)  # the fp32-input operator on the widened rounded states
    y_u, s_u = stem_fwd(L, 'simq_conv2d_fwd_stem_bf16', x, w, B, cin)            # ... and on the unrounded ones
    assert np.isfinite(widen(bits16(y_u))).all() and (bits16(y_u) != SENT16).all()
    assert np.array_equal(bits16(y16), bits16(y_r)) and np.array_equal(bits16(y16), bits16(y_u))
    for other in (s_r, s_u):                                                     # fp64 atomics in arbitrary order in both forms
        a, b = s16.cpu().numpy(), other.cpu().numpy()
        assert (np.abs(a - b) <= 1e-12 * np.maximum(np.abs(a), np.abs(b))).all(), np.abs(a - b).max()
    # a NaN and an Inf at image corners: the first element of the tensor and the last (both tensor-edge rows, left and right padding)
    xn = x.clone()
    xn[0, 0, 0, 0] = float('nan')
    xn[B - 1, W - 1, W - 1, cin - 1] = float('inf')
    if B > 1:
        xn[1, 0, W - 1, 0] = float('-inf')
    yn16, _ = stem_fwd(L, 'simq_conv2d_fwd_stem_bf16_x16', to_bf16(xn), w, B, cin, stats=False)
    yn_u, _ = stem_fwd(L, 'simq_conv2d_fwd_stem_bf16', xn, w, B, cin, stats=False)
    assert np.isnan(widen(bits16(yn_u)))[0, 0, 0].all() and not np.isfinite(widen(bits16(yn_u)))[B - 1, 47, 47].all()
    same_bf16(yn16, yn_u, 'non-finite inputs')


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('cin', [3, 4, 5, 9])
def test_stem_weight_gradient_over_bf16_states(S, L, cin, B):
    from simq.fcn import to_bf16
    x, _ = stem_inputs(cin, B, 200 + 10 * cin + B)
    dy = host_bf16(np.random.RandomState(300 + cin + B).randn(B, 48, 48, 64).astype(np.float32)).cuda()
    slabs = min(512, -(-(B * 48 * 3) // 16))
    dws = []
    for entry, xin in (('simq_conv2d_wgrad_stem_bf16_x16', to_bf16(x)), ('simq_conv2d_wgrad_stem_bf16', x)):
        dw = sentinel32(64, 7, 7, cin)
        L.lib.c.simq_launch_counts_reset()
        L.lib.call(entry, L.ptr(xin), L.ptr(dy), L.ptr(dw), B, W, W, cin, L.ptr(scratch(slabs * 64 * 49 * cin * 4)), L.stream_ptr())
        torch.cuda.synchronize()
        assert L.launch_counts() == {'stem_wgrad_bf16_x16' if entry.endswith('x16') else 'stem_wgrad_bf16': 1}
        dws.append(bits32(dw))
    assert np.isfinite(dws[1].view(np.float32)).all() and np.abs(dws[1].view(np.float32)).max() > 0
    assert np.array_equal(dws[0], dws[1])                                        # the slabs are summed in a fixed order


# ---- 4. mapper states written as bf16 -----------------------------------------------------------------------------------------------------
def dense16(L, t):
    need = L.lib.c.simq_local_state_desc_bytes(t.G, t.n_robots, t.P, t.C)
    out = sentinel16(t.P, W, W, t.C)
    L.lib.call('simq_local_state_images_bf16', *t.head(), L.ptr(scratch(need)), ctypes.c_int64(need), L.ptr(out), ctypes.c_int64(out.numel()),
               L.stream_ptr())
    torch.cuda.synchronize()
    return out


def slotted16(L, t, slots, pool):
    need = L.lib.c.simq_local_state_slots_desc_bytes(t.G, t.n_robots, t.P, t.C)
    L.lib.call('simq_local_state_images_slots_bf16', *t.head(), tdt.slots_array(slots), L.ptr(scratch(need)), ctypes.c_int64(need), L.ptr(pool),
               ctypes.c_int64(pool.shape[0]), L.stream_ptr())
    torch.cuda.synchronize()


def test_mapper_states_are_the_rounded_fp32_states(L, golden_dir):
    for name, fx in tdt.local_fixtures(golden_dir):
        maps, masks = tdt.device_inputs(fx)
        for poisoned in (False, True):
            if poisoned:                                                         # a map with a NaN cell: NaN at the same pixels
                maps = [m.clone() for m in maps]
                maps[0][fx['states'][0]['pixel'][0], fx['states'][0]['pixel'][1]] = float('nan')
            t = tdt.Tables(fx, maps, masks)
            f32 = t.dense(L)                                                     # what the fp32 entry gives
            if not poisoned:
                assert np.array_equal(bits32(f32), bits32(fx['want']))           # ... which is what tests/local_maps_oracle.py gives
            else:
                assert np.isnan(f32.cpu().numpy()).any()
            L.lib.c.simq_launch_counts_reset()
            d16 = dense16(L, t)
            assert L.launch_counts() == {'local_state_bf16': 1}
            same_bf16(d16, host_bf16(f32), (name, 'dense', poisoned))
            rng = np.random.RandomState(t.P)
            slots = tdt.shuffled_slots(rng, t.P, t.P + 5)                        # not consecutive, slot 0 and the last among them
            pool = sentinel16(t.P + 5, W, W, t.C)
            L.lib.c.simq_launch_counts_reset()
            slotted16(L, t, slots, pool)
            assert L.launch_counts() == {'local_state_slots_bf16': 1}
            for p, s in enumerate(slots):
                same_bf16(pool[s], host_bf16(f32[p]), (name, 'slot', p, s, poisoned))
            assert (bits16(pool)[sorted(set(range(t.P + 5)) - set(slots))] == SENT16).all(), name


# ---- 5. the rings -----------------------------------------------------------------------------------------------------------------------
def rounded(a):
    """float32 ndarray -> the float32 ndarray of its bf16 rounding (host reference)."""
    return host_bf16(a).float().numpy()


def test_bf16_pool_push_adopt_reserve_gather_and_sample(S, L, golden_dir):
    C = 5
    transitions = tdt.scripted_transitions(C, 90, 41)                           # 90 pushes into 64 records: the ring wraps, slots are released
    ref = S.AliasedDeviceReplayBuffer(64, C)
    ring = S.AliasedDeviceReplayBuffer(64, C, dtype='bf16')
    assert ring.pool.dtype == torch.bfloat16 and ring.pool.shape == ref.pool.shape
    ring.pool.view(torch.int16).fill_(SENT16)
    for k, (s, a, r, ns) in enumerate(transitions):
        ref.push(s, a, r, ns)
        ring.push(s, a, r, ns)
        assert ring.observations_resident == ref.observations_resident and ring.position == ref.position
    assert len(ring) == 64 and ring.observations_resident < 128
    torch.cuda.synchronize()
    for x, y in zip(ring.buffer, ref.buffer):
        assert (x.action, x.reward, x.next_state is None) == (y.action, y.reward, y.next_state is None) and int(x.state) == int(y.state)
    rec = ring.buffer[7]
    got = np.asarray(rec.state)
    assert got.dtype == np.float32 and np.array_equal(bits32(got), bits32(rounded(np.asarray(ref.buffer[7].state))))
    assert rec.state.copy().dtype == np.float32 and rec.state[3, 4].dtype == np.float32 and rec.state.device_row().dtype == torch.bfloat16
    free = sorted(ring._free)
    assert (bits16(ring.pool[free[-1]]) == SENT16).all()                         # a slot never handed out was never written
    # sample: the picks of the reference's rule (tests/golden/sampler.npz: random.sample(range(len), B)) -- those of the fp32 pool
    random.seed(12)
    picks = random.sample(range(64), 8)
    random.seed(12)
    assert ring.sample_indices(8) == picks
    random.seed(12)
    want = ref.sample(8)
    random.seed(12)
    got = ring.sample(8)
    torch.cuda.synchronize()
    assert got.state.dtype == torch.bfloat16 and got.next_state.dtype == torch.bfloat16 and got.non_final_mask == want.non_final_mask
    assert np.array_equal(bits16(got.state), bits16(host_bf16(want.state))) and np.array_equal(bits16(got.next_state), bits16(host_bf16(want.next_state)))
    for k in ('action', 'reward', 'nonfinal_pos'):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    # adopt: an fp32 tensor is rounded, a bf16 tensor scattered as it is; gather_handles reads them back
    from simq import synth
    x = torch.from_numpy(synth.make_states(3, C, 43)).cuda()
    h32 = ring.adopt(x)
    x16 = host_bf16(x).cuda()
    h16 = ring.adopt(x16)
    back = ring.gather_handles(h32 + h16)
    torch.cuda.synchronize()
    assert back.dtype == torch.bfloat16 and np.array_equal(bits16(back), bits16(torch.cat([x16, x16])))
    a = np.asarray(h32[1])
    assert a.dtype == np.float32 and np.array_equal(bits32(a), bits32(x16[1].float()))
    ring.push(h32[0], 1, 0.5, h16[0])
    ring.discard(h32 + h16)                                                      # slot release: the pushed pair stays, the other four go back
    assert [ring._ref[h.slot] for h in h32 + h16] == [1, 0, 0, 1, 0, 0] and all(h.slot in ring._free for h in h32[1:] + h16[1:])
    # refusals of adopt: a wrong dtype, a wrong shape -- and a bf16 tensor into an fp32 pool
    for bad in (x.double(), x.half(), x[:, :, :, :4].contiguous(), x[0]):
        with pytest.raises(L.SimqError, match='adopt takes'):
            ring.adopt(bad)
    with pytest.raises(L.SimqError, match='adopt takes a contiguous float32 tensor'):
        ref.adopt(x16)


def test_mapper_writes_rounded_states_into_a_bf16_pool(S, L, golden_dir, monkeypatch):
    import glob
    episodes = [mapper_oracle.load_fixture(f) for f in sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))]
    cfg = mapper_oracle.configurations()['full_spatial']
    bm = tdt.build_mapper(S, episodes, cfg)
    frames, robots = tdt.round_inputs(S, episodes, 0)
    bm.update(*frames)
    C = len(bm.channels)
    shuffled = [4, 1, 5, 0]
    ring = S.AliasedDeviceReplayBuffer(8, C, pool_slots=12, dtype='bf16')
    other = S.AliasedDeviceReplayBuffer(8, C, pool_slots=12)
    ring.pool.view(torch.int16).fill_(SENT16)
    ring.reserve(3)                                                              # (dropped at once: the free list is no longer in slot order)
    names = []
    real = L.Lib.call
    monkeypatch.setattr(L.Lib, 'call', staticmethod(lambda name, *a, **k: names.append(name) or real(name, *a, **k)))
    hs = ring.reserve(4)
    got = bm.get_states(robots, mappers=shuffled, into=hs)
    assert all(g is h for g, h in zip(got, hs)) and names.count('simq_local_state_images_slots_bf16') == 1
    assert 'simq_local_state_images_slots' not in names and 'simq_local_state_images' not in names
    dense = bm.get_states(robots, mappers=shuffled)                              # the fp32 states of the same call
    torch.cuda.synchronize()
    want = host_bf16(dense)
    for p, h in enumerate(hs):
        assert np.array_equal(bits16(ring.pool[h.slot]), bits16(want[p])), p
        assert np.array_equal(bits32(np.asarray(h)), bits32(want[p].float()))
    assert (bits16(ring.pool)[sorted(set(range(12)) - {h.slot for h in hs})] == SENT16).all()
    # handles of two pools of different type are refused, before anything is launched
    del names[:]
    with pytest.raises(ValueError, match='more than one pool'):
        bm.get_states(robots, mappers=shuffled, into=hs[:3] + other.reserve(1))
    assert not [n for n in names if n.startswith('simq_local_state')]


def test_two_ring_buffer_of_bf16_states(S):
    C = 4
    transitions = tdt.scripted_transitions(C, 21, 47)
    ref, ring = S.DeviceReplayBuffer(16, C), S.DeviceReplayBuffer(16, C, dtype='bf16')
    assert ring.states.dtype == torch.bfloat16 and ring.next_states.dtype == torch.bfloat16
    for k, (s, a, r, ns) in enumerate(transitions):
        ref.push(s, a, r, ns)
        if k % 3 == 0:                                                           # device tensors: fp32 (rounded on the way in) ...
            ring.push(torch.from_numpy(s).cuda(), a, r, None if ns is None else torch.from_numpy(ns)[None].cuda())
        elif k % 3 == 1:                                                         # ... bf16 (copied) ...
            ring.push(host_bf16(s).cuda(), a, r, None if ns is None else host_bf16(ns).cuda())
        else:                                                                    # ... and ndarrays through the staging ring
            ring.push(s, a, r, ns)
    random.seed(3)
    want = ref.sample(6)
    random.seed(3)
    got = ring.sample(6)
    torch.cuda.synchronize()
    assert got.state.dtype == torch.bfloat16 and got.non_final_mask == want.non_final_mask
    assert np.array_equal(bits16(got.state), bits16(host_bf16(want.state))) and np.array_equal(bits16(got.next_state), bits16(host_bf16(want.next_state)))
    a = np.asarray(ring.buffer[2].state)
    assert a.dtype == np.float32 and np.array_equal(bits32(a), bits32(rounded(np.asarray(ref.buffer[2].state))))
    # the bulk fill
    from simq import synth
    st, ns = synth.make_states(5, C, 48), synth.make_states(5, C, 49)
    bulk = S.DeviceReplayBuffer(8, C, dtype='bf16')
    bulk.push_many(st, np.arange(5), np.zeros(5, np.float32), ns, np.array([False, True, False, False, False]))
    torch.cuda.synchronize()
    assert np.array_equal(bits16(bulk.states[:5]), bits16(host_bf16(st))) and np.array_equal(bits16(bulk.next_states[:5]), bits16(host_bf16(ns)))
    assert bulk.buffer[1].next_state is None and len(bulk) == 5


# ---- 6. the whole step --------------------------------------------------------------------------------------------------------------------
def step_transitions(cin, cout, B, seed):
    from simq import synth
    trs = synth.make_transitions(B, cin, cout, seed, terminal_frac=0.0)
    return [(s, a, r, None if k in (1, 3) else ns) for k, (s, a, r, ns) in enumerate(trs)]       # two terminal transitions


def learner(S, cin, cout, options, dtype, transitions):
    from oracle import fcn as ofcn
    from simq import synth
    nets = []
    for seed in (3, 4):
        net = S.FCN(cin, cout, precision='bf16', options=options)
        net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, seed)))
        nets.append(net)
    nets[0].train(); nets[1].eval()
    ring = S.AliasedDeviceReplayBuffer(8, cin, pool_slots=16, dtype=dtype)
    for t in transitions:
        ring.push(*t)
    return nets[0], nets[1], ring


@pytest.mark.parametrize('double_dqn,fused', [(True, True), (False, True), (True, False)], ids=['double', 'vanilla', 'composed'])
def test_whole_step_from_a_bf16_pool_equals_the_step_from_the_fp32_pool(S, double_dqn, fused):
    import simq.learner as sl
    from oracle import cases as c
    cin, cout, B = 5, 2, 5
    transitions = step_transitions(cin, cout, B, 7)
    A = learner(S, cin, cout, {'deterministic': 1}, 'fp32', transitions)
    Bb = learner(S, cin, cout, {'deterministic': 1, 'bf16_states': 1}, 'bf16', transitions)
    assert A[0].plan.bf16_states == 0 and Bb[0].plan.bf16_states == 1 and Bb[0].state_dtype == torch.bfloat16
    out = []
    for policy, target, ring in (A, Bb):
        steps = []
        for idx in ([3, 0, 4, 1, 2], [1, 2, 0, 4, 3]):
            batch = ring.gather(idx)
            assert batch.state.dtype == ring.dtype and sum(batch.non_final_mask) == 3
            info = sl.train_step(policy, target, batch, c.GAMMA, B, c.LR, c.MOMENTUM, c.WEIGHT_DECAY, c.CLIP, use_double_dqn=double_dqn,
                                 options=sl.StepOptions(fused=fused))
            torch.cuda.synchronize()
            steps.append((info['loss'], info['td_error'], policy._last['q_sa'].clone(), policy._last['td'].clone()))
        out.append(dict(steps=steps, params=policy.flat_params.clone(), grads=policy.flat_grads.clone(), bn=policy.bn_buffers.clone(),
                        momentum=policy._simq_opt_state.momentum.clone(), tracked=dict(policy.num_batches_tracked)))
    a, b = out
    for (la, ta, qa, tda), (lb, tb, qb, tdb) in zip(a['steps'], b['steps']):
        assert la == la and abs(la) < 1e6 and (la, ta) == (lb, tb)
        assert np.array_equal(bits32(qa), bits32(qb)) and np.array_equal(bits32(tda), bits32(tdb))
    for k in ('params', 'grads', 'momentum', 'bn'):
        assert np.array_equal(bits32(a[k]), bits32(b[k])), k
    assert a['tracked'] == b['tracked']
    # an fp32 batch handed to the bf16_states learner is rounded on the device and gives the same step as its own bf16 batch would
    pol, tgt, ring16 = learner(S, cin, cout, {'deterministic': 1, 'bf16_states': 1}, 'bf16', transitions)
    for idx in ([3, 0, 4, 1, 2], [1, 2, 0, 4, 3]):
        info = sl.train_step(pol, tgt, A[2].gather(idx), c.GAMMA, B, c.LR, c.MOMENTUM, c.WEIGHT_DECAY, c.CLIP, use_double_dqn=double_dqn,
                             options=sl.StepOptions(fused=fused))
    torch.cuda.synchronize()
    assert (info['loss'], info['td_error']) == a['steps'][1][:2] and np.array_equal(bits32(pol.flat_params), bits32(a['params']))


# ---- 7. acting ------------------------------------------------------------------------------------------------------------------------------
def test_policy_acts_on_handles_of_a_bf16_pool_as_on_the_fp32_pool(S):
    C = 4
    base = dict(robot_config=[{'lifting_robot': 3}, {'pushing_robot': 1}], num_input_channels=C, final_exploration=0.01, checkpoint_path=None,
                simq_precision='bf16')
    ref = S.DQNPolicy(types.SimpleNamespace(**base), train=False, random_seed=3)
    pol = S.DQNPolicy(types.SimpleNamespace(simq_plan_options={'bf16_states': 1}, **base), train=False, random_seed=3)
    for a, b in zip(ref.policy_nets, pol.policy_nets):
        assert a.plan.bf16_states == 0 and b.plan.bf16_states == 1
        b.load_state_dict(a.state_dict())
        a.eval(); b.eval()
    envs = tdt.policy_envs(C, 51)
    ring32 = S.AliasedDeviceReplayBuffer(8, C, pool_slots=24)
    ring16 = S.AliasedDeviceReplayBuffer(8, C, pool_slots=24, dtype='bf16')
    for keep_host in ((), (1, 4, 7)):                                            # every state a handle; handles and ndarrays mixed
        h32, h16 = tdt.adopt_structure(ring32, envs, set(keep_host)), tdt.adopt_structure(ring16, envs, set(keep_host))
        for eps in (0.0, 0.5):
            random.seed(17)
            want = [ref.step(st, exploration_eps=eps) for st in h32]
            random.seed(17)
            assert [pol.step(st, exploration_eps=eps) for st in h16] == want, (keep_host, eps)
            random.seed(17)
            assert pol.step_many(h16, exploration_eps=eps) == want, (keep_host, eps)
            random.seed(17)
            assert [pol.step(st, exploration_eps=eps) for st in envs] == want    # ndarrays: rounded on the device, one launch
        random.seed(23)
        want_a, want_info = ref.step(h32[0], exploration_eps=0.0, debug=True)
        random.seed(23)
        got_a, got_info = pol.step(h16[0], exploration_eps=0.0, debug=True)
        assert got_a == want_a
        tdt.same_info(got_info, want_info)                                       # the Q-maps, bit for bit


# ---- 8. the consumers that need fp32 ------------------------------------------------------------------------------------------------------
def test_fp32_consumers_give_their_results_on_the_rounded_states(S):
    import simq.learner as sl
    from oracle import cases as c, fcn as ofcn
    from simq import synth
    C, B = 5, 4
    states = synth.make_states(B, C, 81)
    ring16 = S.AliasedDeviceReplayBuffer(8, C, pool_slots=16, dtype='bf16')
    ring32 = S.AliasedDeviceReplayBuffer(8, C, pool_slots=16)
    for k in range(B):
        ring16.push(states[k], k, 0.0, None if k else states[1])
        ring32.push(rounded(states[k]), k, 0.0, None if k else rounded(states[1]))
    # train_intention_step: the BCE target is the last channel of the state
    res = []
    for ring in (ring32, ring16):
        net = S.FCN(C - 1, 1, precision='fp32', options={'deterministic': 1})
        net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(C - 1, 1, 5)))
        net.train()
        info = sl.train_intention_step(net, ring.gather([2, 0, 3, 1]), c.LR, c.MOMENTUM, c.WEIGHT_DECAY)
        torch.cuda.synchronize()
        res.append((info['loss_intention'], net.flat_params.clone(), net._last['target'].clone()))
    assert res[0][0] == res[1][0] and np.array_equal(bits32(res[0][1]), bits32(res[1][1])) and np.array_equal(bits32(res[0][2]), bits32(res[1][2]))
    # DQNIntentionPolicy.step_many on handles of a bf16 pool == on the rounded arrays
    cfg = types.SimpleNamespace(robot_config=[{'lifting_robot': 3}, {'pushing_robot': 1}], num_input_channels=5, final_exploration=0.01,
                                checkpoint_path=None)
    pol = S.DQNIntentionPolicy(cfg, train=False, random_seed=3)
    for n in pol.policy_nets + pol.intention_nets:
        n.eval()
    envs = tdt.policy_envs(4, 52)
    round_envs = [[[None if s is None else rounded(s) for s in g] for g in st] for st in envs]
    pool = S.AliasedDeviceReplayBuffer(8, 4, pool_slots=24, dtype='bf16')
    handles = tdt.adopt_structure(pool, envs, set())
    random.seed(17)
    want = pol.step_many(round_envs, exploration_eps=0.5)
    random.seed(17)
    assert pol.step_many(handles, exploration_eps=0.5) == want
    random.seed(17)
    assert [pol.step(st, exploration_eps=0.5) for st in handles] == want
    # state_output_visualizations reading rows of a bf16 pool
    outputs = np.random.RandomState(72).randn(2, 2, W, W).astype(np.float32)
    vs = synth.make_states(2, 4, 71)
    hs = pool.adopt(torch.from_numpy(vs).cuda())
    want = S.state_output_visualizations([rounded(v) for v in vs], list(outputs))
    got = S.state_output_visualizations(hs, list(outputs))
    torch.cuda.synchronize()
    assert np.array_equal(bits32(got), bits32(want))


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_a_bf16_batch_into_a_plan_without_the_option_is_refused_before_any_launch(S, L, precision):
    import simq.learner as sl
    from oracle import cases as c
    cin, cout, B = 5, 2, 5
    policy, target = S.FCN(cin, cout, precision=precision), S.FCN(cin, cout, precision=precision)
    policy.train(); target.eval()
    ring = S.AliasedDeviceReplayBuffer(8, cin, pool_slots=16, dtype='bf16')
    for t in step_transitions(cin, cout, B, 9):
        ring.push(*t)
    batch = ring.gather([0, 1, 2, 3, 4])
    torch.cuda.synchronize()
    params = policy.flat_params.clone()
    for fused in (True, False):
        L.lib.c.simq_launch_counts_reset()
        with pytest.raises(L.SimqError, match=r'bf16_states.*\.float\(\)'):
            sl.train_step(policy, target, batch, c.GAMMA, B, c.LR, c.MOMENTUM, c.WEIGHT_DECAY, c.CLIP, options=sl.StepOptions(fused=fused))
        assert L.launch_counts() == {}
    L.lib.c.simq_launch_counts_reset()
    policy.eval()
    with pytest.raises(L.SimqError, match='bf16_states'):
        policy.forward_nhwc(batch.state)
    with pytest.raises(L.SimqError, match='bf16_states'):
        policy.infer_argmax(batch.state[:1])
    assert L.launch_counts() == {} and torch.equal(policy.flat_params, params)
    # nets that disagree on the option are refused as well
    if precision == 'bf16':
        odd = S.FCN(cin, cout, precision='bf16', options={'bf16_states': 1})
        with pytest.raises(L.SimqError, match='agree on the plan option bf16_states'):
            sl.train_step(policy.train(), odd.eval(), batch, c.GAMMA, B, c.LR, c.MOMENTUM, c.WEIGHT_DECAY, c.CLIP)
        assert L.launch_counts() == {}


# ---- 10. checkpoints -----------------------------------------------------------------------------------------------------------------------
def test_a_bf16_ring_saves_float32_and_loads_bit_identical(S, tmp_path):
    from simq import checkpoint
    C = 4
    ring = S.AliasedDeviceReplayBuffer(8, C, pool_slots=12, dtype='bf16')
    for t in tdt.scripted_transitions(C, 11, 61):
        ring.push(*t)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9)
    path = S.save_checkpoint(tmp_path, 7, 2, [opt], [ring])
    host = S.load_checkpoint(path)['replay_buffers'][0]
    assert all(isinstance(r.state, np.ndarray) and r.state.dtype == np.float32 and (r.next_state is None or r.next_state.dtype == np.float32)
               for r in host.buffer)
    t, e, rings = checkpoint.resume(path, [opt], device='cuda', dtype='bf16')
    back = rings[0]
    torch.cuda.synchronize()
    assert (t, e) == (7, 2) and back.dtype == torch.bfloat16 and back.position == ring.position and len(back) == len(ring)
    for x, y in zip(ring.buffer, back.buffer):
        assert (x.action, x.reward, x.next_state is None) == (y.action, y.reward, y.next_state is None)
        assert np.array_equal(bits16(ring.pool[int(x.state)]), bits16(back.pool[int(y.state)]))
        if x.next_state is not None:
            assert np.array_equal(bits16(ring.pool[int(x.next_state)]), bits16(back.pool[int(y.next_state)]))
    random.seed(9)
    want = ring.sample(4)
    random.seed(9)
    got = back.sample(4)
    torch.cuda.synchronize()
    assert np.array_equal(bits16(got.state), bits16(want.state)) and np.array_equal(bits16(got.next_state), bits16(want.next_state))
