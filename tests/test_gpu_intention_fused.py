"""GPU: the intention supervision step as one library call and bf16 states end to end on the predicted-intention path (DESIGN
section 27): simq_intention_split, simq_bce_with_logits_state and simq_sigmoid_concat_x against the entries they stand beside,
simq_train_intention_step against the separate calls and the golden fixtures, its loss copy against a full synchronise, and
DQNIntentionPolicy on handles of a bf16 pool against the same policy on the widened arrays."""
import random
import types

import numpy as np
import pytest
import torch

from oracle import cases
from oracle import fcn as ofcn
from oracle import learner as olearner
from simq import arch, synth

pytestmark = pytest.mark.gpu

W = 96
SENT = {torch.bfloat16: 0x7FD5, torch.float32: 0x7FC0BEEF}      # NaNs with a payload: an element written, or left unwritten, shows
BF, F32 = torch.bfloat16, torch.float32
# fp32 bit patterns: two NaNs with payloads (one signalling), +-Inf, -0, a denormal, the largest value below 2 (rounds up to the next
# bf16 binade), the largest finite value (rounds to +Inf as bf16)
SPECIALS = np.array([0x7FC0BEEF, 0xFFA5A5A5, 0x7F800000, 0xFF800000, 0x80000000, 0x00012345, 0x3FFFFFFF, 0x7F7FFFFF], np.uint32)
CHANNELS = [2, 4, 5, 10, 14]


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


@pytest.fixture(scope='module')
def L(S):
    from simq import _lib
    return _lib


def bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == BF:
        return t.view(torch.int16).numpy().view(np.uint16)
    if t.dtype == torch.float64:
        return t.view(torch.int64).numpy().view(np.uint64)
    return t.view(torch.int32).numpy().view(np.uint32)


def isnan_bits(b):
    wide = b.astype(np.uint32) << 16 if b.dtype == np.uint16 else b
    return np.isnan(wide.view(np.float32))


def same(got, want, exact, what=''):
    """exact: equal bits.  Otherwise (a conversion): equal bits wherever the reference is not a NaN, and NaN where it is."""
    got, want = bits(got).reshape(-1), bits(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if exact:
        assert np.array_equal(got, want), what
        return
    nan_g, nan_w = isnan_bits(got), isnan_bits(want)
    assert np.array_equal(nan_g, nan_w), what
    assert np.array_equal(got[~nan_w], want[~nan_w]), what


def rel(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()
    b = torch.as_tensor(np.asarray(b.detach().cpu() if torch.is_tensor(b) else b)).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class Guarded:
    """n elements of `dtype` that start `off` elements behind the start of an allocation (torch allocations start on 256-byte boundaries),
    inside a buffer of sentinels: `off` in front, 16 behind."""

    def __init__(self, dtype, n, off):
        self.n, self.off, self.dtype = n, off, dtype
        self.base = torch.empty(off + n + 16, dtype=dtype, device='cuda')
        assert self.base.data_ptr() % 256 == 0
        self.base.view(torch.int16 if dtype == BF else torch.int32).fill_(SENT[dtype])
        self.view = self.base[off:off + n]

    def untouched(self):
        b = bits(self.base)
        return bool((b[:self.off] == SENT[self.dtype]).all() and (b[self.off + self.n:] == SENT[self.dtype]).all())


def recorded_calls(L, fn):
    """The names of every lib.call made while fn() runs, and fn's result."""
    names = []
    orig = L.Lib.__dict__['call']

    def wrapper(name, *args, **kwargs):
        names.append(name)
        return orig.__func__(name, *args, **kwargs)

    L.Lib.call = staticmethod(wrapper)
    try:
        out = fn()
    finally:
        L.Lib.call = orig
    return names, out


# ---- 1. the split ------------------------------------------------------------------------------------------------------------------------
def split_state(B, C, rot):
    """[pixels][C] fp32: normal values, with the specials (rotated by `rot`, so that over the runs of a case the first and the last pixel
    see every one of them) in the first, an interior and the last run of pixels, in channel 0 and, reversed, in channel C-1."""
    P = B * W * W
    s = np.random.RandomState(100 * B + C).standard_normal((P, C)).astype(np.float32)
    u = s.view(np.uint32)
    sp = np.roll(SPECIALS, rot)
    for start in (0, P // 2 + 3, P - len(sp)):
        u[start:start + len(sp), 0] = sp
        u[start:start + len(sp), C - 1] = sp[::-1]
    return s


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', CHANNELS)
def test_split_moves_bits_and_converts_as_the_state_conversions_do(S, L, C, B):
    from simq.fcn import to_bf16, to_f32
    P, run = B * W * W, 0
    for in16 in (0, 1):
        for out16 in (0, 1):
            # (state, head, last) element offsets from a 256-byte boundary: all 16-byte aligned; each array in turn 4 bytes (fp32) or 2 bytes
            # (bf16) off, which sends every tile down the element-wise path; all three off
            for offs in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                x32 = torch.from_numpy(split_state(B, C, run)).cuda()
                run += 1
                src = to_bf16(x32) if in16 else x32
                piece = src[:, :C - 1].contiguous()
                want_head = piece if in16 == out16 else to_bf16(piece) if out16 else to_f32(piece)
                want_last = to_f32(src[:, C - 1].contiguous()) if in16 else src[:, C - 1].contiguous()
                for with_last in ((True, False) if offs in ((0, 0, 0), (1, 1, 1)) else (True,)):
                    st = Guarded(BF if in16 else F32, P * C, offs[0])
                    st.view.copy_(src.reshape(-1))
                    head = Guarded(BF if out16 else F32, P * (C - 1), offs[1])
                    last = Guarded(F32, P, offs[2])
                    L.lib.c.simq_launch_counts_reset()
                    L.lib.call('simq_intention_split', L.ptr(st.view), in16, L.ptr(head.view), out16, L.ptr(last.view) if with_last else None,
                               P, C, L.stream_ptr())
                    assert L.launch_counts() == {'intention_split': 1}
                    what = (in16, out16, offs, with_last)
                    same(head.view, want_head, in16 == out16, what)
                    assert head.untouched() and st.untouched(), what
                    same(st.view, src, True, what)                                  # the state itself is only read
                    if with_last:
                        same(last.view, want_last, True, what)                       # fp32 bits moved, bf16 widened exactly: no rounding either way
                        assert last.untouched(), what
                    else:
                        assert (bits(last.base) == SENT[F32]).all(), what            # last = NULL: nothing of it is written
    x = torch.zeros(P, 2, device='cuda')
    with pytest.raises(L.SimqError, match='channels'):
        L.lib.call('simq_intention_split', L.ptr(x), 0, L.ptr(torch.empty(P, 1, device='cuda')), 0, None, P, 1, L.stream_ptr())


# ---- 2. BCE against the last state channel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pixels', [1, 255, 3 * 9216 + 5])
@pytest.mark.parametrize('C', [2, 5])
def test_bce_on_the_state_is_the_bce_on_the_split_off_target(S, L, C, pixels):
    from simq.fcn import to_bf16, to_f32
    g = torch.Generator().manual_seed(3 + C)
    x = (torch.randn(pixels, generator=g) * 6).float()
    x[0] = 0.0
    if pixels > 2:
        x[1], x[2] = 60.0, -60.0                                                     # saturated logits: the stable form must not overflow
    state32 = torch.rand(pixels, C, generator=g).cuda()
    xd = x.cuda()
    scratch = torch.empty(int(L.lib.c.simq_bce_state_scratch_bytes()), dtype=torch.uint8, device='cuda')
    for in16 in (0, 1):
        state = to_bf16(state32) if in16 else state32
        target = (to_f32(state) if in16 else state)[:, C - 1].contiguous()
        dx_old, ls_old = torch.empty_like(xd), torch.zeros(1, dtype=torch.float64, device='cuda')
        L.lib.call('simq_bce_with_logits', L.ptr(xd), L.ptr(target), pixels, L.ptr(dx_old), L.ptr(ls_old), L.stream_ptr())
        runs = []
        for _ in range(2):
            dx, ls = torch.full_like(xd, 7.0), torch.full((1,), -1.0, dtype=torch.float64, device='cuda')
            scratch.fill_(0xA5)
            L.lib.c.simq_launch_counts_reset()
            L.lib.call('simq_bce_with_logits_state', L.ptr(xd), L.ptr(state), in16, pixels, C, L.ptr(dx), L.ptr(ls), L.ptr(scratch), L.stream_ptr())
            assert L.launch_counts() == {'bce_state': 1}
            runs.append((dx, ls))
        (dx, ls), (dx2, ls2) = runs
        print('bce_state C=%d pixels=%d bf16=%d: loss sum %.17g, the atomic entry %.17g' % (C, pixels, in16, float(ls.item()), float(ls_old.item())))
        same(dx, dx_old, True, 'dlogits')                                             # the same expression, element for element
        same(dx2, dx, True)
        assert np.array_equal(bits(ls), bits(ls2)), 'two runs of the ordered sum differ'
        # both are fp64 sums of the same <= 2.8e4 fp32 terms, in another order
        assert abs(float(ls.item()) - float(ls_old.item())) <= 1e-12 * abs(float(ls_old.item()))
        x64 = x.double().requires_grad_(True)
        ref = torch.nn.functional.binary_cross_entropy_with_logits(x64, target.cpu().double())
        ref.backward()
        assert abs(float(ls.item()) / pixels - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
        assert rel(dx, x64.grad) < 1e-5
        L.lib.call('simq_bce_with_logits_state', L.ptr(xd), L.ptr(state), in16, pixels, C, None, L.ptr(ls2), L.ptr(scratch), L.stream_ptr())   # loss only
        assert np.array_equal(bits(ls), bits(ls2))


# ---- 3. sigmoid + concat -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', CHANNELS)
def test_concat_in_every_type_pair_is_the_fp32_concat_rounded(S, L, C, B):
    from simq.fcn import to_bf16, to_f32
    P, Cs = B * W * W, C - 1
    x32 = torch.from_numpy(np.ascontiguousarray(split_state(B, C, C)[:, :Cs])).cuda()
    logit = (torch.randn(P, generator=torch.Generator().manual_seed(C)) * 6).cuda()
    logit[0], logit[1], logit[2] = 0.0, 60.0, -60.0
    x16 = to_bf16(x32)

    def old(x):
        out, prob = torch.empty(P, Cs + 1, device='cuda'), torch.empty(P, device='cuda')
        L.lib.call('simq_sigmoid_concat', L.ptr(x), L.ptr(logit), L.ptr(out), L.ptr(prob), P, Cs, L.stream_ptr())
        return out, prob

    out_a, prob_a = old(x32)                  # on the fp32 state
    out_b, _ = old(to_f32(x16))               # on the widened bf16 state
    for in16 in (0, 1):
        for out16 in (0, 1):
            for offs in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 1, 0)):       # state, logit, out, prob
                src = x16 if in16 else x32
                st = Guarded(BF if in16 else F32, P * Cs, offs[0])
                st.view.copy_(src.reshape(-1))
                lg = Guarded(F32, P, offs[1])
                lg.view.copy_(logit)
                out = Guarded(BF if out16 else F32, P * (Cs + 1), offs[2])
                prob = Guarded(F32, P, offs[3])
                for with_prob in (True, False):
                    L.lib.c.simq_launch_counts_reset()
                    L.lib.call('simq_sigmoid_concat_x', L.ptr(st.view), in16, L.ptr(lg.view), L.ptr(out.view), out16,
                               L.ptr(prob.view) if with_prob else None, P, Cs, L.stream_ptr())
                    assert L.launch_counts() == {'sigmoid_concat_x': 1}
                    what = (in16, out16, offs, with_prob)
                    want32 = out_b if in16 else out_a                               # a bf16 state in gives what its widening gives
                    if out16:
                        same(out.view, to_bf16(want32), False, what)
                    else:
                        same(out.view, want32, True, what)                          # fp32 -> fp32: simq_sigmoid_concat, bit for bit
                    same(prob.view, prob_a, True, what)                              # (first pass: written; second pass: left as it was)
                    assert out.untouched() and prob.untouched() and st.untouched() and lg.untouched(), what


# ---- 4. the fused step, fp32 -----------------------------------------------------------------------------------------------------------------
def intention_net(S, cin, wseed, precision='fp32', options=None, fused=False):
    net = S.FCN(cin, 1, precision=precision, options=options)
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, 1, wseed)))
    net.train()
    net.fused_step = fused
    return net


@pytest.mark.parametrize('case', cases.INTENTION_CASES, ids=[c[0] for c in cases.INTENTION_CASES])
def test_fused_step_vs_golden_and_oracle(S, L, case, golden_dir):
    """test_train_intention_vs_golden_and_oracle (tests/test_gpu_intention.py) with net.fused_step = True, under its bars."""
    name, cin_full, B, wseed, dseed = case
    cin = cin_full - 1
    g = np.load('%s/%s.npz' % (golden_dir, name))
    batch = cases.make_batch(cin_full, 1, B, dseed)
    spec = ofcn.state_spec(cin, 1)
    net = intention_net(S, cin, wseed, fused=True)
    opt = torch.optim.SGD(net.parameters(), lr=cases.LR, momentum=cases.MOMENTUM, weight_decay=cases.WEIGHT_DECAY)
    st64 = cases.oracle_state(cin, 1, wseed, torch.float64)
    ex64 = {}
    olearner.train_intention_step(st64, spec, [None] * len(olearner.grad_keys(spec)), batch, cases.LR, cases.MOMENTUM,
                                  cases.WEIGHT_DECAY, dtype=torch.float64, extras=ex64)
    names, info1 = recorded_calls(L, lambda: S.train_intention(net, opt, batch, olearner.apply_transform))
    assert names == ['simq_weights_prepare', 'simq_train_intention_step', 'simq_train_loss_wait'], names
    assert set(info1) == {'loss_intention'} and isinstance(info1['loss_intention'], float)
    print('%s fused: loss %.9g (golden %.9g)' % (name, info1['loss_intention'], float(g['loss_intention'][0])))
    assert rel(info1['loss_intention'], g['loss_intention'][0]) < 1e-4
    assert rel(net._last['logits'], g['output_step1']) < 1e-4
    assert 'target' not in net._last
    got = {}
    gflat = net.flat_grads.detach().cpu()
    for (pname, _, kind), (off, n, shape) in zip(net._param_names, net._grad_views):
        t = gflat[off:off + n].view(shape)
        got[arch.PREFIX + pname] = t.permute(0, 3, 1, 2).contiguous() if len(shape) == 4 else t
    num = sum(float((got[k].double() - ex64['grads'][k]).pow(2).sum()) for k in ex64['grads'])
    den = sum(float(ex64['grads'][k].pow(2).sum()) for k in ex64['grads'])
    err = (num / den) ** 0.5
    print('%s fused: gradient rel-L2 %.3g vs fp64' % (name, err))
    assert err <= 5e-2, 'gradient rel-L2 error %.3g vs fp64 (reference fp32 itself: %.3g)' % (err, float(g['ref_fp32_grad_relerr']))
    p0 = next(iter(net.parameters()))
    assert opt.state[p0]['momentum_buffer'].data_ptr() == net._simq_opt_state.momentum.data_ptr()
    info2 = S.train_intention(net, opt, batch, olearner.apply_transform)
    assert rel(info2['loss_intention'], g['loss_intention'][1]) < 2e-2
    sd = net.state_dict()
    assert all(int(sd[k]) == 2 for k in sd if k.endswith('num_batches_tracked'))
    rows = np.asarray([[float(sd[k].double().sum()), float(sd[k].double().norm())] for k, _, kind in spec if ofcn.is_parameter(kind)])
    assert np.abs(rows[:, 1] - g['param_summary_after2'][:, 1]).max() <= 1e-4 * g['param_summary_after2'][:, 1].max()
    # the target on request, and the refusals of the entry with a device behind it
    from simq.learner import train_intention_step
    train_intention_step(net, batch, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, keep_target=True)
    want = torch.from_numpy(np.stack(batch.state))[..., cin]
    assert torch.equal(net._last['target'].cpu(), want)
    with pytest.raises(L.SimqError, match='single-process'):
        train_intention_step(net, batch, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, comm=object())
    with pytest.raises(Exception):
        S.train_intention(intention_net(S, cin + 1, wseed, fused=True), opt, batch, None)      # channel mismatch
    with pytest.raises(Exception):
        net._backward_raw(torch.zeros(B, 1, W, W, device='cuda'), B)                           # the head was convolved in place: no stale backward


def two_steps(S, net, batches):
    from simq.learner import train_intention_step
    losses = [train_intention_step(net, b, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY)['loss_intention'] for b in batches]
    torch.cuda.synchronize()
    return dict(losses=losses, params=net.flat_params.clone(), grads=net.flat_grads.clone(), momentum=net._simq_opt_state.momentum.clone(),
                bn=net.bn_buffers.clone(), logits=net._last['logits'].clone(), tracked=dict(net.num_batches_tracked))


def test_fused_step_equals_the_separate_calls_on_a_deterministic_plan(S, L):
    """Two steps fused against two steps unfused from equal weights, on a plan with deterministic = 1.  The unfused path runs twice first:
    where its own two runs are bit-equal (they were, on every tensor below, when this test was written) the fused run must be bit-equal to
    them; a tensor on which they differ would be compared at their spread.  The losses are fp64 sums of the same fp32 terms in another
    order (the unfused sum is made with atomics): 1e-12 relative."""
    C, B = 5, 4
    ring = S.DeviceReplayBuffer(8, C)
    for t in synth.make_transitions(6, C, 1, 44, terminal_frac=0.0):
        ring.push(*t)
    batches = lambda: [ring.gather([3, 0, 4, 1]), ring.gather([5, 2, 0, 4])]
    u1, u2 = (two_steps(S, intention_net(S, C - 1, 34, options={'deterministic': 1}), batches()) for _ in range(2))
    names, f = recorded_calls(L, lambda: two_steps(S, intention_net(S, C - 1, 34, options={'deterministic': 1}, fused=True), batches()))
    assert names.count('simq_train_intention_step') == 2 and 'simq_split_last_channel' not in names, names
    for k in ('logits', 'params', 'grads', 'momentum', 'bn'):
        spread = float((u1[k].double() - u2[k].double()).abs().max())
        print('%s: spread of the unfused path %.3g, fused - unfused %.3g' % (k, spread, float((f[k].double() - u1[k].double()).abs().max())))
        if np.array_equal(bits(u1[k]), bits(u2[k])):
            assert np.array_equal(bits(f[k]), bits(u1[k])), k
        else:
            assert float((f[k].double() - u1[k].double()).abs().max()) <= spread, k
    for a, b in zip(f['losses'], u1['losses']):
        print('loss fused %.17g unfused %.17g' % (a, b))
        assert a == a and abs(a - b) <= 1e-12 * abs(b)
    assert f['tracked'] == u1['tracked'] and set(f['tracked'].values()) == {2}


# ---- 5. the fused step on bf16 pools ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,extra', [(5, {}), (10, {}), (11, {'stem_bf16': 2})], ids=['c5', 'c10', 'c11_wide'])
def test_fused_step_from_a_bf16_ring_equals_the_widening_path(S, L, C, extra):
    """A plain-bf16 intention net with bf16_states = 1 steps on the minibatch of a bf16 ring as it is: no widening pass, the head rounded
    nowhere (bf16 bits moved), the target read in place.  Compared as tests/test_gpu_bf16_states.py compares its fp32-pool and bf16-pool
    learners -- deterministic plans, bit for bit -- with the widening path of a net without the option; the loss, whose unfused sum is
    made with atomics in arbitrary order, at 1e-12 relative."""
    from simq.fcn import to_bf16, to_f32
    B = 3
    ring = S.DeviceReplayBuffer(8, C, dtype='bf16')
    for t in synth.make_transitions(5, C, 1, 40 + C, terminal_frac=0.0):
        ring.push(*t)
    picks = ([3, 0, 4], [1, 2, 0])
    ref = intention_net(S, C - 1, 21, 'bf16', dict(extra, deterministic=1))
    net = intention_net(S, C - 1, 21, 'bf16', dict(extra, deterministic=1, bf16_states=1), fused=True)
    assert ref.state_dtype == F32 and net.state_dtype == BF and not ref.fused_step
    want = two_steps(S, ref, [ring.gather(p) for p in picks])
    batches = [ring.gather(p) for p in picks]
    assert batches[0].state.dtype == BF
    names, got = recorded_calls(L, lambda: two_steps(S, net, batches))
    assert 'simq_states_to_f32' not in names and 'simq_states_to_bf16' not in names and 'simq_split_last_channel' not in names, names
    assert names.count('simq_train_intention_step') == 2
    head = to_bf16(to_f32(batches[1].state)[..., :C - 1].contiguous())
    same(net._last['head'], head, True, 'the head the step convolved')
    for k in ('logits', 'params', 'grads', 'momentum', 'bn'):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    for a, b in zip(got['losses'], want['losses']):
        print('C=%d loss fused %.17g widening path %.17g' % (C, a, b))
        assert a == a and abs(a - b) <= 1e-12 * abs(b)
    # a bf16 batch into a plan WITHOUT bf16_states is allowed on the fused path: the split widens it
    ref2 = intention_net(S, C - 1, 21, 'bf16', dict(extra, deterministic=1), fused=True)
    names, got2 = recorded_calls(L, lambda: two_steps(S, ref2, [ring.gather(p) for p in picks]))
    assert 'simq_states_to_f32' not in names
    assert ref2._last['head'].dtype == F32
    for k in ('logits', 'params', 'grads', 'momentum', 'bn'):
        assert np.array_equal(bits(got2[k]), bits(want[k])), k


# ---- 6. run-ahead ----------------------------------------------------------------------------------------------------------------------------
def test_deferred_loss_and_two_plans_waiting_side_by_side(S, L):
    import simq.learner as sl
    C, B = 5, 4
    trs = synth.make_transitions(B, C, 2, 9, terminal_frac=0.0)
    ring = S.DeviceReplayBuffer(8, C)
    for t in trs:
        ring.push(*t)

    def nets():
        policy, target = S.FCN(C, 2, options={'deterministic': 1}), S.FCN(C, 2, options={'deterministic': 1})
        policy.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(C, 2, 3)))
        target.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(C, 2, 4)))
        policy.train(); target.eval()
        return policy, target, intention_net(S, C - 1, 34, options={'deterministic': 1}, fused=True)

    def td(policy, target, batch, sync):
        return sl.train_step(policy, target, batch, cases.GAMMA, B, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, cases.CLIP, sync=sync)

    def intention(inet, batch, sync):
        return sl.train_intention_step(inet, batch, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, sync=sync)

    # one at a time, each waited for at once
    policy, target, inet = nets()
    batch = ring.gather([2, 0, 3, 1])
    want_td = td(policy, target, batch, True)
    want_int = intention(inet, batch, True)
    torch.cuda.synchronize()
    assert float(inet._last['loss_sum'].item()) / (B * W * W) == want_int['loss_intention']
    with pytest.raises(L.SimqError, match='train_loss_wait'):                      # the copy was waited for: none is pending on that plan
        L.lib.call('simq_train_loss_wait', inet.plan.handle)
    # both enqueued back to back, both waited for afterwards: each plan keeps its own copy state
    policy, target, inet = nets()
    batch = ring.gather([2, 0, 3, 1])
    with pytest.raises(L.SimqError, match='train_loss_wait'):
        L.lib.call('simq_train_loss_wait', inet.plan.handle)                       # a plan that never stepped
    p_td = td(policy, target, batch, 'defer')
    p_int = intention(inet, batch, 'defer')
    assert isinstance(p_int, sl.PendingIntentionStep)
    got_int = p_int.result()                                                        # (the later step first)
    got_td = p_td.result()
    assert p_int.result() is got_int
    torch.cuda.synchronize()
    assert float(inet._last['loss_sum'].item()) / (B * W * W) == got_int['loss_intention']      # the value read after a full synchronise
    assert got_td == want_td and got_int == want_int
    # train_groups works unchanged on fused intention nets
    policy, target, inet = nets()
    opt = torch.optim.SGD(policy.parameters(), lr=cases.LR, momentum=cases.MOMENTUM, weight_decay=cases.WEIGHT_DECAY)
    opt_i = torch.optim.SGD(inet.parameters(), lr=cases.LR, momentum=cases.MOMENTUM, weight_decay=cases.WEIGHT_DECAY)
    infos = sl.train_groups(cases.make_cfg(B), [policy], [target], [opt], [ring.gather([2, 0, 3, 1])], None, [cases.GAMMA], intention_nets=[inet],
                            optimizers_intention=[opt_i])
    assert infos == [dict(want_td, **want_int)]


# ---- 7. the policy ---------------------------------------------------------------------------------------------------------------------------
def rounded(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(BF).float().numpy()


@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
def test_policy_on_handles_of_a_bf16_pool_widens_nothing(S, L, train):
    import test_gpu_device_transitions as tdt
    base = dict(robot_config=[{'lifting_robot': 3}, {'pushing_robot': 1}], num_input_channels=5, final_exploration=0.01, checkpoint_path=None,
                simq_precision='bf16')
    ref = S.DQNIntentionPolicy(types.SimpleNamespace(**base), train=train, random_seed=3)
    pol = S.DQNIntentionPolicy(types.SimpleNamespace(simq_plan_options={'bf16_states': 1}, simq_intention_plan_options={'bf16_states': 1},
                                                     simq_intention_fused=True, **base), train=train, random_seed=3)
    for a, b in zip(ref.policy_nets + ref.intention_nets, pol.policy_nets + pol.intention_nets):
        assert a.plan.bf16_states == 0 and b.plan.bf16_states == 1
        b.load_state_dict(a.state_dict())
        for n in (a, b):
            n.train() if train else n.eval()
    assert all(n.fused_step for n in pol.intention_nets) and not any(n.fused_step for n in ref.intention_nets)
    C = 5 if train else 4                                                           # (train mode: the state carries the ground-truth map)
    envs = tdt.policy_envs(C, 51)
    wide = [[[None if s is None else rounded(s) for s in g] for g in st] for st in envs]
    pool = S.AliasedDeviceReplayBuffer(8, C, pool_slots=24, dtype='bf16')
    handles = tdt.adopt_structure(pool, envs, set())

    def act():
        out = []
        for eps in (0.0, 0.5):
            random.seed(17)
            out.append([pol.step(st, exploration_eps=eps) for st in handles])
            random.seed(17)
            out.append(pol.step_many(handles, exploration_eps=eps))
        random.seed(23)
        out.append(pol.step(handles[0], exploration_eps=0.0, debug=True))
        return out

    names, got = recorded_calls(L, act)
    assert 'simq_states_to_f32' not in names, names
    assert ('simq_intention_split' in names) == train and 'simq_sigmoid_concat_x' in names and 'simq_sigmoid_concat' not in names
    k = 0
    for eps in (0.0, 0.5):
        random.seed(17)
        want = [ref.step(st, exploration_eps=eps) for st in wide]
        assert got[k] == want and got[k + 1] == want, (train, eps)
        k += 2
    random.seed(23)
    want_a, want_info = ref.step(wide[0], exploration_eps=0.0, debug=True)
    got_a, got_info = got[k]
    assert got_a == want_a
    for ga, gb in zip(got_info['output_intention'], want_info['output_intention']):
        for xa, xb in zip(ga, gb):
            assert (xa is None) == (xb is None)
            if xa is not None:
                assert np.array_equal(np.asarray(xa, np.float32).view(np.uint32), np.asarray(xb, np.float32).view(np.uint32))
    assert all(n.training == train for n in pol.policy_nets + pol.intention_nets)


def legacy_scenario(S):
    """Everything a DQNIntentionPolicy WITHOUT the new cfg keys and a train_intention_step without fused_step do on fp32 states: ndarrays and
    handles of an fp32 pool, step / step_many / debug, eval and train mode, then one supervision step."""
    import simq.learner as sl
    cfg = types.SimpleNamespace(robot_config=[{'lifting_robot': 2}, {'pushing_robot': 1}], num_input_channels=5, final_exploration=0.01,
                                checkpoint_path=None)
    pol = S.DQNIntentionPolicy(cfg, train=False, random_seed=3)
    for n in pol.policy_nets + pol.intention_nets:
        n.eval()
    s = list(synth.make_states(4, 4, 61))
    pol.step([[s[0], None], [s[1]]], exploration_eps=0.0)
    pol.step([[s[0], s[2]], [None]], exploration_eps=0.0, debug=True)
    pol.step_many([[[s[0], s[1]], [s[2]]], [[None, s[3]], [None]]], exploration_eps=0.0)
    pool = S.AliasedDeviceReplayBuffer(8, 4, pool_slots=16)
    h = pool.adopt(torch.from_numpy(np.stack(s)).cuda())
    pol.step([[h[0], None], [h[1]]], exploration_eps=0.0)
    pol.step_many([[[h[0], s[1]], [h[2]]]], exploration_eps=0.0)
    pol.train = True
    for n in pol.policy_nets + pol.intention_nets:
        n.train()
    f = list(synth.make_states(3, 5, 62))
    pool5 = S.AliasedDeviceReplayBuffer(8, 5, pool_slots=16)
    h5 = pool5.adopt(torch.from_numpy(np.stack(f)).cuda())
    pol.step([[f[0], None], [f[1]]], exploration_eps=0.0)
    pol.step([[h5[0], None], [h5[1]]], exploration_eps=0.0)
    pol.step_many([[[h5[0], f[1]], [h5[2]]]], exploration_eps=0.0)
    pol.step([[f[0], None], [None]], exploration_eps=0.0, use_ground_truth_intention=True)
    ring = S.DeviceReplayBuffer(8, 5)
    for t in synth.make_transitions(4, 5, 1, 63, terminal_frac=0.0):
        ring.push(*t)
    sl.train_intention_step(pol.intention_nets[0], ring.gather([2, 0, 3, 1]), cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY)
    sl.train_intention_step(pol.intention_nets[0], ring.gather([1, 3, 0, 2]), cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, sync='defer').result()
    torch.cuda.synchronize()


# what legacy_scenario issued on the parent of the change that added the typed path (recorded there with recorded_calls, the parent's
# Python package on this library): 122 calls.  PRED: one forward of an intention net + the fp32 concat; ACT: one forward of a Q-network +
# the argmax (forward_nhwc refreshes the weight cache every time)
PRED = ['simq_weights_prepare', 'simq_forward', 'simq_sigmoid_concat']
ACT = ['simq_weights_prepare', 'simq_forward', 'simq_q_argmax']
GATHER, SCATTER = ['simq_replay_gather'], ['simq_replay_scatter']
LEGACY_CALLS = sum([
    PRED, PRED, ACT, ACT,                                            # step on ndarrays
    PRED, PRED, ACT,                                                 # ... with debug
    PRED, PRED, ACT, ACT,                                            # step_many
    SCATTER, GATHER, PRED, GATHER, PRED, ACT, ACT,                   # adopt; step on handles of an fp32 pool
    GATHER, PRED, GATHER, PRED, ACT, ACT,                            # step_many on handles and an ndarray
    SCATTER, PRED, PRED, ACT, ACT,                                   # train mode: adopt; step on ndarrays
    GATHER, GATHER, PRED, PRED, ACT, ACT,                            # ... on handles
    GATHER, PRED, GATHER, PRED, ACT, ACT,                            # ... step_many
    ACT,                                                             # ground-truth intention: the Q-network alone
    GATHER, GATHER, ['simq_split_last_channel', 'simq_forward', 'simq_bce_with_logits', 'simq_plan_adopt_side_stream', 'simq_backward_phase',
                     'simq_clip_sgd_step'],                           # train_intention_step, unfused
    GATHER, GATHER, ['simq_split_last_channel', 'simq_weights_prepare', 'simq_forward', 'simq_bce_with_logits', 'simq_backward_phase',
                     'simq_clip_sgd_step'],
], [])


def test_a_policy_without_the_new_keys_issues_the_calls_it_issued(S, L):
    names, _ = recorded_calls(L, lambda: legacy_scenario(S))
    assert len(LEGACY_CALLS) == 122
    assert names == LEGACY_CALLS, [(k, a, b) for k, (a, b) in enumerate(zip(names, LEGACY_CALLS)) if a != b][:5]
