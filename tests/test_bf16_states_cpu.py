"""CPU: what a replay pool of bf16 states checks before it needs a device -- the plan option bf16_states (default,
round trip, the plans that may carry it, the workspace it must not enlarge), the host refusals of the bf16 mapper entries and of the two
conversions (fake device pointers, never dereferenced), the dtype= keyword of the rings, and the reference every GPU test of the
feature rests on: torch's float32 -> bfloat16 conversion on the host is round-to-nearest-even, shown here against an integer restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('simq_states_to_bf16', 'simq_states_to_f32', 'simq_conv2d_fwd_stem_bf16_x16', 'simq_conv2d_wgrad_stem_bf16_x16',
       'simq_local_state_images_bf16', 'simq_local_state_images_slots_bf16')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def crafted_values():
    """float32 values whose rounding to bf16 takes every branch: ties with an even and with an odd kept mantissa, just below / above a
    tie, the largest finite float32 (rounds to +Inf), the largest value that stays finite, the smallest normal, denormals (one that
    rounds up into the normals' neighbourhood, ties among denormals, the smallest), +-0, +-Inf and NaNs."""
    bits = [0x3F808000,              # 1 + 2^-8: a tie, kept mantissa even (0x3F80) -> stays
            0x3F818000,              # a tie, kept mantissa odd (0x3F81) -> up to 0x3F82
            0x3F807FFF, 0x3F808001,  # just below / just above a tie
            0xBF808000, 0xBF818000,  # the same ties, negative
            0x7F7FFFFF,              # the largest finite float32 -> +Inf
            0xFF7FFFFF,              # ... -> -Inf
            0x7F7F7FFF,              # the largest float32 that stays finite (below the tie under bf16's largest, 0x7F7F)
            0x7F7F8000,              # that tie: kept mantissa odd -> up, to +Inf
            0x00800000,              # the smallest normal
            0x007FFFFF,              # the largest denormal -> the smallest normal
            0x00008000,              # a tie among the denormals, kept mantissa even (0) -> +0
            0x00018000,              # ... odd -> 0x0002
            0x00000001, 0x80000001,  # the smallest denormals -> +-0
            0x00010000, 0x80010000,  # denormals that bf16 holds exactly
            0x00000000, 0x80000000,  # +-0
            0x7F800000, 0xFF800000,  # +-Inf
            0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF]   # NaNs: quiet, negative with payload, signalling, all ones
    return np.array(bits, dtype=np.uint32).view(np.float32)


def rne_bits(a):
    """float32 ndarray -> bf16 bits (uint16), round to nearest even, in integers; a NaN gives a quiet NaN of its sign."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x0040).astype(np.uint16), r)


def host_bf16_bits(a):
    """The CPU reference of the GPU tests: torch's conversion on the host, as bits."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_the_host_reference_is_round_to_nearest_even():
    v = crafted_values()
    got, want = host_bf16_bits(v), rne_bits(v)
    nan = np.isnan(v)
    assert nan.sum() == 4
    assert np.array_equal(got[~nan], want[~nan]), [(hex(a), hex(b), hex(c)) for a, b, c in zip(v.view(np.uint32), got, want) if b != c]
    wide = (got.astype(np.uint32) << 16).view(np.float32)
    assert np.isnan(wide[nan]).all()                                      # a NaN stays a NaN; its payload is not part of the contract
    # what the crafted values are there for, spelled out
    by = {int(b): int(g) for b, g in zip(v.view(np.uint32), got)}
    assert by[0x3F808000] == 0x3F80 and by[0x3F818000] == 0x3F82 and by[0x3F807FFF] == 0x3F80 and by[0x3F808001] == 0x3F81
    assert by[0x7F7FFFFF] == 0x7F80 and by[0xFF7FFFFF] == 0xFF80 and by[0x7F7F7FFF] == 0x7F7F and by[0x7F7F8000] == 0x7F80
    assert by[0x00800000] == 0x0080 and by[0x007FFFFF] == 0x0080 and by[0x00008000] == 0x0000 and by[0x00018000] == 0x0002
    assert by[0x00000001] == 0x0000 and by[0x80000001] == 0x8000 and by[0x00010000] == 0x0001 and by[0x80000000] == 0x8000
    assert by[0x7F800000] == 0x7F80 and by[0xFF800000] == 0xFF80
    # and on random values of every magnitude
    rng = np.random.RandomState(5)
    r = rng.randint(0, 1 << 32, size=20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    ok = ~np.isnan(r)
    assert np.array_equal(host_bf16_bits(r)[ok], rne_bits(r)[ok])


def test_new_entry_points_are_declared_exported_and_bound(L):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'simq.h')).read(), flags=re.S)
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        proto = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, header)
        assert proto, '%s is not declared in include/simq.h' % name
        assert hasattr(raw, name), 'libsimq.so does not export %s' % name
        assert name in L.EXPORTS and len(L._SIGS[name][1]) == proto.group(1).count(',') + 1, name
    # the bf16 entries take what the fp32 entries take
    for a, b in (('simq_local_state_images', 'simq_local_state_images_bf16'), ('simq_local_state_images_slots', 'simq_local_state_images_slots_bf16'),
                 ('simq_conv2d_fwd_stem_bf16', 'simq_conv2d_fwd_stem_bf16_x16'), ('simq_conv2d_wgrad_stem_bf16', 'simq_conv2d_wgrad_stem_bf16_x16')):
        assert L._SIGS[a] == L._SIGS[b]
    assert re.search(r'int\s+bf16_states\s*;[^}]*}\s*simq_plan_options\s*;', header, flags=re.S), 'bf16_states must be the last field'
    assert L.PlanOptions._fields_[-1][0] == 'bf16_states'


def test_the_option_defaults_to_zero_and_round_trips(L):
    c = L.lib.c
    o = L.PlanOptions()
    c.simq_plan_options_default(ctypes.byref(o))
    assert o.bf16_states == 0 and o.struct_bytes == ctypes.sizeof(L.PlanOptions)
    assert L.Plan(5, 2, 'bf16').bf16_states == 0 and L.Plan(5, 2).bf16_states == 0
    plan = L.Plan(5, 2, 'bf16', options={'bf16_states': 1})
    assert plan.bf16_states == 1
    got = L.PlanOptions()
    assert c.simq_plan_get_options(plan.handle, ctypes.byref(got)) == 0 and got.bf16_states == 1 and got.stem_bf16 == 1
    # every other option is what it was
    assert plan.options == L.Plan(5, 2, 'bf16').options


def test_only_plans_whose_first_convolution_runs_stem_conv_bf16_take_the_option(L):
    for cin in range(3, 10):
        assert L.Plan(cin, 2, 'bf16', options={'bf16_states': 1}).bf16_states == 1
    for kw in (dict(cin=5, precision='fp32'), dict(cin=5, precision='bf16x3'), dict(cin=5, precision='bf16', extra={'stem_bf16': 0}),
               dict(cin=10, precision='bf16')):
        with pytest.raises(L.SimqError) as e:
            L.Plan(kw['cin'], 2, kw['precision'], options=dict(kw.get('extra', {}), bf16_states=1))
        msg = str(e.value)
        assert 'bf16_states' in msg and 'SIMQ_PREC_BF16' in msg and 'stem_bf16 = 1' in msg and '7 * num_input_channels <= 63' in msg, msg
    with pytest.raises(L.SimqError, match='bf16_states = 2'):
        L.Plan(5, 2, 'bf16', options={'bf16_states': 2})
    # ... and without the option all of them are created as before
    for cin, prec, extra in ((5, 'fp32', {}), (5, 'bf16x3', {}), (5, 'bf16', {'stem_bf16': 0}), (10, 'bf16', {})):
        assert L.Plan(cin, 2, prec, options=extra).bf16_states == 0


def test_the_option_never_enlarges_a_workspace(L):
    for cin in (3, 5, 9):
        for det in (0, 1):
            a = L.Plan(cin, 2, 'bf16', options={'deterministic': det})
            b = L.Plan(cin, 2, 'bf16', options={'deterministic': det, 'bf16_states': 1})
            for batch in (1, 5, 128):
                for fwd in (False, True):
                    wa, wb = a.workspace_bytes(batch, forward_only=fwd), b.workspace_bytes(batch, forward_only=fwd)
                    assert 0 < wb <= wa, (cin, batch, fwd, wa, wb)
                    # what is saved is the grad-mode forward's copy of the minibatch: half of it, up to the 256-byte alignment of the slots
                    assert wa - wb >= batch * 96 * 96 * cin * 2 - 256, (cin, batch, wa, wb)
            assert L._c.simq_wcache_bytes(a.handle) == L._c.simq_wcache_bytes(b.handle)


def test_conversions_refuse_bad_arguments_before_any_device_call(L):
    c = L.lib.c
    SRC, DST = 0x10000000, 0x20000000
    for name, src_align, dst_align, src_elem, dst_elem in (('simq_states_to_bf16', 4, 2, 4, 2), ('simq_states_to_f32', 2, 4, 2, 4)):
        fn = getattr(c, name)

        def refused(word, src=SRC, dst=DST, n=64):
            assert fn(ctypes.c_void_p(src) if src else None, ctypes.c_void_p(dst) if dst else None, n, None) == -1, (name, src, dst, n)
            assert word in L.last_error(), (word, L.last_error())

        refused('NULL', src=0)
        refused('NULL', dst=0)
        refused('n < 1', n=0)
        refused('aligned', src=SRC + src_align // 2)
        refused('aligned', dst=DST + dst_align // 2)
        refused('overlaps', dst=SRC + 64 * src_elem - dst_align)                 # the destination's first element is the source's last bytes
        refused('overlaps', src=DST + 64 * dst_elem - src_align)
        if not torch.cuda.is_available():
            assert fn(ctypes.c_void_p(SRC), ctypes.c_void_p(SRC + 64 * src_elem), 64, None) == -2, L.last_error()   # adjacent: every check passed


def test_bf16_mapper_entries_refuse_what_the_fp32_entries_refuse(L):
    """Every refusal of the two new entry points with fake pointers, one at a time; sizes and overlaps count 2-byte elements."""
    from simq import local_maps as lm
    c = L.lib.c
    MAPS, MASKS, DESC, POOL, OUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    item = 96 * 96 * 2                                                              # one channel: BYTES of a bf16 slot
    rot = lm.Rotation((ctypes.c_double * 4)(1, 0, -0.0, 1), (ctypes.c_double * 2)(0, 0), (ctypes.c_int32 * 2)(136, 136))

    def tables(n, kind, maps):
        probs = (lm.LocalProblem * max(n, 1))(*[lm.LocalProblem(rot, 92, 116, 184, 232, 0, 0)] * max(n, 1))
        chans = (lm.LocalChannel * max(n, 1))(*[lm.LocalChannel(kind, 0, 0.0, 0)] * max(n, 1))
        return (lm.LocalMap * 1)(lm.LocalMap(maps, 184, 232)), probs, chans

    def slots_call(slots, n=None, maps=MAPS, desc=DESC, desc_bytes=1 << 20, pool=POOL, pool_slots=8, kind=0, problems=True):
        n = len(slots) if n is None else n
        a_maps, probs, chans = tables(n, kind, maps)
        return c.simq_local_state_images_slots_bf16(a_maps, 1, ctypes.c_void_p(MASKS), 2, None, 0, probs if problems else None, n, chans, 1,
                                                    (ctypes.c_int64 * max(len(slots), 1))(*slots), ctypes.c_void_p(desc) if desc else None,
                                                    desc_bytes, ctypes.c_void_p(pool) if pool else None, pool_slots, None)

    def dense_call(n=2, maps=MAPS, desc=DESC, desc_bytes=1 << 20, out=OUT, out_elems=None, kind=0):
        a_maps, probs, chans = tables(n, kind, maps)
        return c.simq_local_state_images_bf16(a_maps, 1, ctypes.c_void_p(MASKS), 2, None, 0, probs, n, chans, 1, ctypes.c_void_p(desc) if desc else None,
                                              desc_bytes, ctypes.c_void_p(out) if out else None, n * 96 * 96 if out_elems is None else out_elems, None)

    def refused(call, word, *a, **kw):
        assert call(*a, **kw) == -1, (a, kw)
        assert word in L.last_error(), (word, L.last_error())

    # ---- the slots form
    refused(slots_call, 'local_state_images_slots_bf16: NULL', [1], pool=None)
    refused(slots_call, 'NULL', [1], desc=None)
    refused(slots_call, 'NULL', [1], problems=False)
    refused(slots_call, 'n = 0', [1], n=0)
    refused(slots_call, 'pool_slots = 0', [0], pool_slots=0)
    refused(slots_call, 'd_pool 2-byte aligned', [1], pool=POOL + 1)
    refused(slots_call, 'd_desc must be 8-byte', [1], desc=DESC + 4)
    refused(slots_call, 'slot -1 outside the pool of 8', [-1, 2])
    refused(slots_call, 'slot 8 outside the pool of 8', [2, 8])
    refused(slots_call, 'slot 2 is named twice', [2, 5, 2])
    need = c.simq_local_state_slots_desc_bytes(1, 0, 2, 1)
    refused(slots_call, 'd_desc holds %d bytes, the descriptors and the slot table take %d' % (need - 1, need), [1, 2], desc_bytes=need - 1)
    # a 184 x 232 fp32 map placed in the pool from slot 3 on covers 170 752 bytes = slots 3 .. 12 of 18 432 bytes each
    assert -(-184 * 232 * 4 // item) == 10
    for s in (3, 12):
        refused(slots_call, 'slot %d overlaps map 0' % s, [0, s], maps=POOL + 3 * item, pool_slots=16)
    refused(slots_call, 'slot 1 overlaps d_desc', [1], desc=POOL + item + 64)
    refused(slots_call, 'slot 0 overlaps the mask bank', [0], pool=MASKS)
    refused(slots_call, 'local_state_images_slots_bf16: problem 0 channel 0: kind 5', [1], kind=5)
    # ---- the dense form
    refused(dense_call, 'local_state_images_bf16: NULL', out=None)
    refused(dense_call, 'NULL', desc=None)
    refused(dense_call, 'n = 0', n=0)
    refused(dense_call, 'd_out 2-byte aligned', out=OUT + 1)
    refused(dense_call, 'd_desc must be 8-byte', desc=DESC + 2)
    refused(dense_call, 'd_out holds %d bf16 elements' % (2 * 96 * 96 - 1), out_elems=2 * 96 * 96 - 1)
    need = c.simq_local_state_desc_bytes(1, 0, 2, 1)
    refused(dense_call, 'd_desc holds %d bytes' % (need - 1), desc_bytes=need - 1)
    refused(dense_call, 'd_out overlaps d_desc', desc=OUT + 2 * item - 8)           # the last 8 bytes of the second image
    refused(dense_call, 'd_out overlaps map 0', maps=OUT + 2 * item - 4)
    refused(dense_call, 'd_out overlaps the mask bank', out=MASKS + 4)
    refused(dense_call, 'local_state_images_bf16: problem 0 channel 0: kind 7', kind=7)
    if not torch.cuda.is_available():
        # every check passed: refused by the missing device.  The scratch right behind the bf16 images -- inside them, were they fp32
        assert dense_call(desc=OUT + 2 * item) == -2, L.last_error()
        assert slots_call([0, 2, 1], maps=POOL + 3 * item) == -2, L.last_error()
        assert slots_call([1], pool=POOL + 2) == -2, L.last_error()                 # 2-byte alignment is all a bf16 pool needs


def test_dtype_keyword_of_the_rings():
    from simq import learner
    for cls in (learner.DeviceReplayBuffer, learner.AliasedDeviceReplayBuffer):
        assert cls(4, 3, device='cpu').dtype == torch.float32 and cls(4, 3, device='cpu', dtype='fp32').item == 96 * 96 * 3
        ring = cls(4, 3, device='cpu', dtype='bf16')
        assert ring.dtype == torch.bfloat16 and ring.states.dtype == torch.bfloat16 and ring.next_states.dtype == torch.bfloat16
        assert ring.item * 4 == 96 * 96 * 3 * 2                            # the gathers move 4-byte words
        for bad in ('fp16', 'float32', torch.bfloat16, None, 16):
            with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
                cls(4, 3, device='cpu', dtype=bad)
    # without a device the ring still holds the rounded state, and a record's state is a float32 array: the exact widening
    v = np.resize(crafted_values()[:22], (96, 96, 3)).astype(np.float32)    # (no NaN among the first 22)
    ring = learner.AliasedDeviceReplayBuffer(4, 3, device='cpu', pool_slots=6, dtype='bf16')
    ring.push(v, 1, 0.5, None)
    got = np.asarray(ring.buffer[0].state)
    assert got.dtype == np.float32 and got.shape == (96, 96, 3)
    assert np.array_equal(got.view(np.uint32), rne_bits(v).astype(np.uint32) << 16)
    assert ring.buffer[0].state.copy().dtype == np.float32 and ring.buffer[0].state[0, 0].dtype == np.float32
    h = ring.reserve(1)[0]
    assert h.device_row().dtype == torch.bfloat16 and np.asarray(h).dtype == np.float32


def test_checkpoint_of_a_bf16_ring_holds_float32_and_comes_back_bit_identical(tmp_path):
    """(host rings: the device path of the same round trip is in tests/test_gpu_bf16_states.py)"""
    import simq
    from simq import checkpoint, learner
    rng = np.random.RandomState(3)
    ring = learner.AliasedDeviceReplayBuffer(3, 4, device='cpu', pool_slots=8, dtype='bf16')
    obs = [rng.randn(96, 96, 4).astype(np.float32) * 10.0 ** rng.randint(-3, 4) for _ in range(4)]
    for k in range(4):                                                     # wraps once
        ring.push(obs[k], k, 0.25 * k, obs[k + 1] if k < 3 else None)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9)
    path = simq.save_checkpoint(tmp_path, 5, 1, [opt], [ring])
    host = simq.load_checkpoint(path)['replay_buffers'][0]
    assert type(host) is learner.ReplayBuffer and all(r.state.dtype == np.float32 for r in host.buffer)
    assert host.buffer[1].next_state is host.buffer[2].state                # one array, pickled once
    back = checkpoint.to_device_ring(host, 4, device='cpu', pool_slots=8, dtype='bf16')
    assert back.dtype == torch.bfloat16 and back.position == ring.position and len(back) == len(ring)
    for a, b in zip(ring.buffer, back.buffer):
        assert (a.action, a.reward, a.next_state is None) == (b.action, b.reward, b.next_state is None)
        assert torch.equal(ring.pool[int(a.state)].view(torch.int16), back.pool[int(b.state)].view(torch.int16))
    # a reference-format ring of unrounded float32 states loaded into a bf16 ring is rounded
    plain = learner.ReplayBuffer(3)
    plain.push(obs[0], 0, 0.0, None)
    dev = checkpoint.to_device_ring(plain, 4, device='cpu', pool_slots=8, dtype='bf16')
    assert np.array_equal(np.asarray(dev.buffer[0].state).view(np.uint32), rne_bits(obs[0]).astype(np.uint32) << 16)
