"""GPU: the wide-row bf16 stem -- the first convolution and its weight gradient on the bf16 matrix cores for 10..13
input channels (64 <= 7 * Cin <= 95: three k-steps per filter row), as standalone operators, inside a plan created with the option
stem_bf16 = 2, under the whole TD step, and fed from a replay pool of bf16 states.  The bars are those of the narrow kernels' tests
(tests/test_gpu_ops.py, test_gpu_bf16_states.py, test_gpu_nonfinite.py, test_gpu_fcn.py); shapes are the smallest that reach both
tensor-edge rows, more than one block, the odd 2-byte-aligned channel counts and the slab-capacity case (Cin = 13 at B = 1)."""
import random
import types

import numpy as np
import pytest
import torch

import nonfinite_cases as nc
import test_gpu_device_transitions as tdt
import test_gpu_fcn as tfcn
from test_gpu_bf16_states import (SENT32, W, bits16, bits32, learner, same_bf16, scratch, sentinel16, sentinel32, stem_inputs,
                                  step_transitions, widen)

pytestmark = pytest.mark.gpu

OPT = {'stem_bf16': 2}


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


@pytest.fixture(scope='module')
def L(S):
    from simq import _lib
    return _lib


def wide_bytes(L):
    return int(L.lib.c.simq_conv2d_fwd_stem_bf16_wide_scratch_bytes())


def edge_case(B, C, seed):
    """The operands of test_stem_conv_bf16_matches_a_bf16_operand_convolution: a large offset on every image edge, so that a wrong
    padding mask cannot hide."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 96, 96, C, generator=g)
    x[:, 0, :, :] += 3.0; x[:, -1, :, :] -= 3.0; x[:, :, 0, :] += 5.0; x[:, :, -1, :] -= 5.0
    w = torch.randn(64, 7, 7, C, generator=g) * (2.0 / (49 * C)) ** 0.5
    return x, w


def conv64(x, w):
    """fp64 convolution of the bf16-rounded operands, NHWC"""
    return nc.conv_ref(x.bfloat16(), w.bfloat16(), stride=2, pad=3)


def wgrad64(x, dy, C):
    """fp64 weight gradient of the bf16-rounded input and the bf16 dy, OHWI"""
    return torch.nn.grad.conv2d_weight(x.bfloat16().double().permute(0, 3, 1, 2), (64, C, 7, 7), dy.double().permute(0, 3, 1, 2), stride=2,
                                       padding=3).permute(0, 2, 3, 1)


def wide_fwd(L, entry, x, w, B, C, stats=True, prefill_nan=False):
    y = torch.full((B, 48, 48, 64), float('nan'), dtype=torch.bfloat16, device='cuda') if prefill_nan else sentinel16(B, 48, 48, 64)
    st = torch.zeros(128, dtype=torch.float64, device='cuda') if stats else None
    L.lib.call(entry, L.ptr(x), L.ptr(w), L.ptr(y), B, W, W, C, L.ptr(st), L.ptr(scratch(wide_bytes(L))), L.stream_ptr())
    torch.cuda.synchronize()
    return y, st


# ---- 1. the forward operator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C', [(1, 10), (2, 11), (2, 12), (3, 13)], ids=['b1_cin10', 'b2_cin11', 'b2_cin12', 'b3_cin13'])
def test_wide_stem_forward_matches_a_bf16_operand_convolution(L, B, C):
    """Against an fp64 convolution of the bf16-ROUNDED operands the only error left is the accumulation order and the one bf16 rounding of
    the stored output (2^-8 of the range); the statistics come from the unrounded accumulators (1e-5).  B = 1 puts both tensor-edge rows
    into one image."""
    x, w = edge_case(B, C, 41 + 7 * C + B)
    xd, wd = x.cuda(), w.cuda()
    L.lib.c.simq_launch_counts_reset()
    y, stats = wide_fwd(L, 'simq_conv2d_fwd_stem_bf16_wide', xd, wd, B, C, prefill_nan=True)
    assert L.launch_counts().get('stem_conv_bf16_wide') == 1 and 'stem_conv_bf16' not in L.launch_counts(), L.launch_counts()
    ref = conv64(x, w)
    got = y.double().cpu()
    assert torch.isfinite(got).all()                                            # every element of the NaN-filled output was written
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    sref = torch.cat([ref.reshape(-1, 64).sum(0), (ref * ref).reshape(-1, 64).sum(0)])
    serr = tfcn.rel(stats, sref)
    print('\nwide stem C=%d B=%d: max error vs fp64 conv of the rounded operands %.3g of the output range, statistics %.3g' % (C, B, err, serr))
    assert err < 2.0 ** -8
    assert serr < 1e-5
    y2, _ = wide_fwd(L, 'simq_conv2d_fwd_stem_bf16_wide', xd, wd, B, C, stats=False, prefill_nan=True)   # eval mode: no statistics, same outputs
    assert np.array_equal(bits16(y), bits16(y2))


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', [10, 11, 13])
def test_wide_stem_forward_over_bf16_states(L, C, B):
    """The _x16 entry on RNE(x) is bit for bit the fp32-input entry on the widened rounded input and on the unrounded input; the BatchNorm
    sums are fp64 atomics in arbitrary order in both (1e-12 relative).  C = 11 and 13: fragments start on odd elements."""
    from simq.fcn import to_bf16, to_f32
    x, w = stem_inputs(C, B, 100 + 10 * C + B)
    x16 = to_bf16(x)
    assert not torch.equal(to_f32(x16), x)
    L.lib.c.simq_launch_counts_reset()
    y16, s16 = wide_fwd(L, 'simq_conv2d_fwd_stem_bf16_wide_x16', x16, w, B, C)
    assert L.launch_counts().get('stem_conv_bf16_wide_x16') == 1 and 'stem_conv_bf16_wide' not in L.launch_counts(), L.launch_counts()
    y_r, s_r = wide_fwd(L, 'simq_conv2d_fwd_stem_bf16_wide', to_f32(x16), w, B, C)
    y_u, s_u = wide_fwd(L, 'simq_conv2d_fwd_stem_bf16_wide', x, w, B, C)
    assert np.isfinite(widen(bits16(y_u))).all()
    assert np.array_equal(bits16(y16), bits16(y_r)) and np.array_equal(bits16(y16), bits16(y_u))
    for other in (s_r, s_u):
        a, b = s16.cpu().numpy(), other.cpu().numpy()
        assert (np.abs(a - b) <= 1e-12 * np.maximum(np.abs(a), np.abs(b))).all(), np.abs(a - b).max()
    # NaN / Inf at the first and the last element of the tensor: both tensor-edge rows, left and right padding
    xn = x.clone()
    xn[0, 0, 0, 0] = float('nan')
    xn[B - 1, W - 1, W - 1, C - 1] = float('inf')
    yn16, _ = wide_fwd(L, 'simq_conv2d_fwd_stem_bf16_wide_x16', to_bf16(xn), w, B, C, stats=False)
    yn_u, _ = wide_fwd(L, 'simq_conv2d_fwd_stem_bf16_wide', xn, w, B, C, stats=False)
    assert np.isnan(widen(bits16(yn_u)))[0, 0, 0].all() and not np.isfinite(widen(bits16(yn_u)))[B - 1, 47, 47].all()
    same_bf16(yn16, yn_u, 'non-finite inputs')


# ---- 2. the weight gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C', [(1, 10), (2, 11), (3, 13), (19, 10)], ids=['b1_cin10', 'b2_cin11', 'b3_cin13', 'b19_cin10'])
def test_wide_stem_weight_gradient(L, B, C):
    """Against the fp64 weight gradient of the bf16-rounded operands only the fp32 accumulation order is left (the existing bar, 1e-4 of the
    range); two runs are bit-identical (slabs added in a fixed order); the scratch is exactly the exported slab count, the region behind it
    is untouched; the _x16 entry on RNE(x) gives the same bits.  B = 19: more chunks than one block takes in a trip."""
    from simq.fcn import to_bf16
    x, _ = edge_case(B, C, 43 + 7 * C + B)
    dy = torch.randn(B, 48, 48, 64, generator=torch.Generator().manual_seed(300 + C + B)).bfloat16()
    xd, dyd = x.cuda(), dy.cuda()
    slabs = L.lib.c.simq_conv2d_wgrad_stem_bf16_slabs(B, W, W, C, -1)
    assert slabs == min(512, 9 * B)
    n, tail = slabs * 64 * 49 * C, 4096
    runs = []
    for entry, xin in (('simq_conv2d_wgrad_stem_bf16_wide', xd), ('simq_conv2d_wgrad_stem_bf16_wide', xd), ('simq_conv2d_wgrad_stem_bf16_wide_x16', to_bf16(xd))):
        dw = sentinel32(64, 7, 7, C)
        buf = sentinel32(n + tail)
        L.lib.c.simq_launch_counts_reset()
        L.lib.call(entry, L.ptr(xin), L.ptr(dyd), L.ptr(dw), B, W, W, C, L.ptr(buf), L.stream_ptr())
        torch.cuda.synchronize()
        assert L.launch_counts() == {entry[len('simq_conv2d_'):].replace('wgrad_stem', 'stem_wgrad'): 1}, L.launch_counts()
        assert (bits32(buf[n:]) == SENT32).all(), 'the weight gradient wrote behind the scratch it asks for'
        runs.append(bits32(dw))
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    got = torch.from_numpy(runs[0].view(np.float32)).double()
    ref = wgrad64(x, dy, C)
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    print('\nwide stem wgrad C=%d B=%d: max error vs fp64 gradient of the rounded operands %.3g of the range' % (C, B, err))
    assert err < 1e-4


# ---- 3. NaN and Inf (rules 1 and 2) ------------------------------------------------------------------------------------------------
# At Cin = 10 a filter row holds 70 real values; elements 70 and 71 of the third k-step's first k-group are channels 0 and 1 of the pixel
# in column 2 ox + 4, one column right of output ox's window: 'tail' puts the value there (ox = 20), where only outputs 21..23 may see it
WIDE_SITES = {'corner': (0, 95, 2), 'interior': (41, 53, 2), 'tail': (40, 44, 0)}


@pytest.mark.parametrize('site', sorted(WIDE_SITES))
@pytest.mark.parametrize('what', sorted(nc.VALUES))
def test_wide_stem_forward_nonfinite(L, what, site):
    from simq.fcn import to_bf16
    B, C = 2, 10
    x, w = edge_case(B, C, 43)
    r, c, ch = WIDE_SITES[site]
    x[1, r, c, ch] = nc.VALUES[what]
    ref = conv64(x, w)
    bad = nc.nonfinite(ref)
    # the reference on the CPU is not vacuous: exactly the outputs whose 7 x 7 window holds the pixel, in image 1 alone
    oys, oxs = [o for o in range(48) if abs(2 * o - r) <= 3], [o for o in range(48) if abs(2 * o - c) <= 3]
    want = torch.zeros_like(bad)
    want[1, oys[0]:oys[-1] + 1, oxs[0]:oxs[-1] + 1, :] = True
    assert torch.equal(bad, want) and int(bad.sum()) == len(oys) * len(oxs) * 64 > 0
    if site == 'tail':
        assert (c - 4) // 2 == 20 and 20 not in oxs and not bool(bad[:, :, 20].any())   # output 20 reads it behind its real values only
    xd, wd = x.cuda(), w.cuda()
    for entry, xin in (('simq_conv2d_fwd_stem_bf16_wide', xd), ('simq_conv2d_fwd_stem_bf16_wide_x16', to_bf16(xd))):
        y, _ = wide_fwd(L, entry, xin, wd, B, C, stats=False)
        nc.check_against_reference(y.float(), ref, 2.0 ** -8, None, '%s %s %s' % (entry, what, site))


# ---- 4. inside a plan, teacher-forced -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,B', [(10, 2), (13, 1), (11, 3)], ids=['cin10_b2', 'cin13_b1', 'cin11_b3'])
def test_plan_with_the_wide_stem_teacher_forced(S, L, C, B):
    """FCN(C, 1, 'bf16', {'stem_bf16': 2}): every forward mode launches the wide kernel once and no generic gather kernel; stem.y0 is the
    fp64 convolution of the rounded input and weights at 2^-8; the 7x7 weight gradient is the fp64 gradient of the STORED dy0 plane and the
    rounded input at 1e-4; both bit-identical over two runs.  C = 13 at B = 1: nine slabs asked for, seven fit the workspace slot."""
    from oracle import cases, fcn as ofcn, learner as olearner
    from simq import synth
    net = S.FCN(C, 1, precision='bf16', options=OPT)
    assert net.plan.options['stem_bf16'] == 2
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(C, 1, 91)))
    net.train()
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, C, 92)]).permute(0, 2, 3, 1).contiguous().cuda()
    dq = torch.from_numpy(cases.dense_upstream(1, B, 95)).cuda().contiguous()
    net._ensure_weights()
    for mode, slot in ((L.MODE_EVAL, None), (L.MODE_TRAIN_NOGRAD, 'tmp')):
        L.lib.call('simq_launch_counts_reset')
        net._forward_raw(x, mode)
        torch.cuda.synchronize()
        ran = L.launch_counts()
        assert ran.get('stem_conv_bf16_wide', 0) == 1 and ran.get('igemm_f32_gather', 0) == 0 and ran.get('stem_conv_bf16', 0) == 0, (mode, ran)
    runs = []
    for _ in range(2):
        L.lib.call('simq_launch_counts_reset')
        net._forward_raw(x, L.MODE_TRAIN)
        torch.cuda.synchronize()
        ran = L.launch_counts()
        assert ran.get('stem_conv_bf16_wide', 0) == 1 and ran.get('igemm_f32_gather', 0) == 0, ran
        L.lib.call('simq_launch_counts_reset')
        grads_flat, traced = net.backward_traced(dq, B)
        torch.cuda.synchronize()
        ran = L.launch_counts()
        assert ran.get('stem_wgrad_bf16_wide', 0) == 1 and ran.get('stem_wgrad_bf16', 0) == 0, ran
        gw = {k: v.detach().cpu().clone() for (k, _, _), v in zip(net._param_names, net.reference_views(grads_flat))}['resnet18.conv1.weight']
        runs.append((net.stored_tensor('stem.y0', B, 'train').cpu().clone(), traced('stem.dy0').cpu().clone(), gw))
    (y0, dy0, gw), (y0b, dy0b, gwb) = runs
    assert y0.dtype == torch.bfloat16 and tuple(y0.shape) == (B, 48, 48, 64) and dy0.dtype == torch.bfloat16
    assert np.array_equal(bits16(y0), bits16(y0b))
    assert np.array_equal(bits16(dy0), bits16(dy0b)) and np.array_equal(bits32(gw), bits32(gwb))
    sd = {k[len('module.'):]: v.detach().cpu() for k, v in net.state_dict().items()}
    w_ohwi = sd['resnet18.conv1.weight'].permute(0, 2, 3, 1)
    ref = conv64(x.cpu(), w_ohwi)
    err = float((y0.double() - ref).abs().max()) / float(ref.abs().max())
    want = wgrad64(x.cpu(), dy0, C).permute(0, 3, 1, 2)                          # (OIHW, the reference's layout)
    gerr = float((gw.double() - want).abs().max()) / float(want.abs().max())
    print('\nplan C=%d B=%d: stem.y0 %.3g of the range, 7x7 weight gradient %.3g of the range' % (C, B, err, gerr))
    assert err < 2.0 ** -8
    assert float(want.abs().max()) > 0 and gerr < 1e-4


# ---- 5. the network ---------------------------------------------------------------------------------------------------------------------------
def test_train_c10o1_b4_with_the_wide_stem_meets_the_bf16_bars(S, golden_dir):
    """test_precision_fused_train's bf16 leg for the ten-channel case, with the option: the calibrated bars of bf16_calibration_cin.npz."""
    from oracle import cases, fcn as ofcn, learner as olearner
    case = [c for c in cases.TRAIN_CASES_CIN if c[0] == 'train_c10o1_b4'][0]
    name, cin, cout, B, wseed, dseed = case
    g = np.load('%s/%s.npz' % (golden_dir, name))
    cal = np.load('%s/bf16_calibration_cin.npz' % golden_dir)
    cfg = cases.make_cfg(B)
    batch = cases.make_batch(cin, cout, B, dseed)
    spec = ofcn.state_spec(cin, cout)
    policy = tfcn.make_net(S, cin, cout, wseed, training=True, precision='bf16', options=OPT)
    target = tfcn.make_net(S, cin, cout, wseed + 1000, training=False, precision='bf16', options=OPT)
    opt = torch.optim.SGD(policy.parameters(), lr=cases.LR, momentum=cases.MOMENTUM, weight_decay=cases.WEIGHT_DECAY)
    st64, tg64 = cases.oracle_state(cin, cout, wseed, torch.float64), cases.oracle_state(cin, cout, wseed + 1000, torch.float64)
    ex64 = {}
    olearner.train_step(cfg, st64, tg64, spec, [None] * len(olearner.grad_keys(spec)), batch, cases.GAMMA, cases.LR, cases.MOMENTUM,
                        cases.WEIGHT_DECAY, dtype=torch.float64, extras=ex64)
    from simq import _lib
    _lib.lib.call('simq_launch_counts_reset')
    info = S.train(cfg, policy, target, opt, batch, None, cases.GAMMA)
    torch.cuda.synchronize()
    ran = _lib.launch_counts()
    assert ran.get('stem_conv_bf16_wide', 0) == 3 and ran.get('stem_wgrad_bf16_wide', 0) == 1 and ran.get('igemm_f32_gather', 0) == 0, ran
    tn = float(policy._simq_opt_state.total_norm.item())
    coef = min(1.0, cases.CLIP / (tn + 1e-6))
    got = {k: v / coef for k, v in tfcn.grads_to_reference_layout(policy).items()}
    err = tfcn.global_rel_l2(got, ex64['grads'])
    print('\n[%s bf16 wide stem] loss %.6f (ref %.6f) td %.6f (ref %.6f) grad rel-L2 err vs fp64 %.3g; calibration loss %.3g td %.3g grad %.3g' % (
        name, info['loss'], float(g['loss'][0]), info['td_error'], float(g['td_error'][0]), err, float(cal[name + '.loss']),
        float(cal[name + '.td_error']), float(cal[name + '.grad'])))
    assert tfcn.rel(info['loss'], g['loss'][0]) < max(0.15, 2 * float(cal[name + '.loss']))
    assert tfcn.rel(info['td_error'], g['td_error'][0]) < max(0.15, 2 * float(cal[name + '.td_error']))
    assert err <= max(0.5, 1.2 * float(cal[name + '.grad']))
    info2 = S.train(cfg, policy, target, opt, batch, None, cases.GAMMA)
    assert np.isfinite(info2['loss'])
    sd = policy.state_dict()
    assert all(int(sd[k]) == 4 for k in sd if k.endswith('num_batches_tracked'))


# ---- 6. narrow plans are what they were ---------------------------------------------------------------------------------------------------
def two_steps(S, L, cin, cout, B, options, dtype, transitions, order, double_dqn=True):
    import simq.learner as sl
    from oracle import cases as c
    policy, target, ring = learner(S, cin, cout, options, dtype, transitions)
    steps, families = [], {}
    for idx in order:
        batch = ring.gather(idx)
        L.lib.c.simq_launch_counts_reset()
        info = sl.train_step(policy, target, batch, c.GAMMA, B, c.LR, c.MOMENTUM, c.WEIGHT_DECAY, c.CLIP, use_double_dqn=double_dqn)
        torch.cuda.synchronize()
        families = L.launch_counts()
        steps.append((info['loss'], info['td_error'], policy._last['q_sa'].clone(), policy._last['td'].clone()))
    return dict(steps=steps, params=policy.flat_params.clone(), grads=policy.flat_grads.clone(), bn=policy.bn_buffers.clone(),
                momentum=policy._simq_opt_state.momentum.clone(), tracked=dict(policy.num_batches_tracked), families=families)


def assert_same_steps(a, b):
    for (la, ta, qa, tda), (lb, tb, qb, tdb) in zip(a['steps'], b['steps']):
        assert la == la and abs(la) < 1e6 and (la, ta) == (lb, tb)
        assert np.array_equal(bits32(qa), bits32(qb)) and np.array_equal(bits32(tda), bits32(tdb))
    for k in ('params', 'grads', 'momentum', 'bn'):
        assert np.array_equal(bits32(a[k]), bits32(b[k])), k
    assert a['tracked'] == b['tracked']


def test_narrow_plans_step_bit_for_bit_as_with_value_one(S, L):
    cin, cout, B = 5, 2, 4
    transitions = step_transitions(cin, cout, B, 7)
    order = ([3, 0, 1, 2], [1, 2, 0, 3])
    one = two_steps(S, L, cin, cout, B, {'deterministic': 1, 'stem_bf16': 1}, 'fp32', transitions, order)
    two = two_steps(S, L, cin, cout, B, {'deterministic': 1, 'stem_bf16': 2}, 'fp32', transitions, order)
    assert_same_steps(one, two)
    assert one['families'] == two['families']
    ran = two['families']
    assert ran.get('stem_conv_bf16', 0) >= 2 and ran.get('stem_wgrad_bf16', 0) == 1, ran
    assert not [k for k in ran if 'wide' in k], ran
    # ... on the grid they had: the workspace slot the slabs live in holds what the batch asks for
    assert L.lib.c.simq_conv2d_wgrad_stem_bf16_slabs(B, W, W, cin, B * 294912 * 4) == L.lib.c.simq_conv2d_wgrad_stem_bf16_slabs(B, W, W, cin, -1) == 9 * B


# ---- 7. a bf16 pool of ten-channel states ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('double_dqn', [True, False], ids=['double', 'vanilla'])
def test_whole_step_from_a_bf16_pool_of_ten_channel_states(S, L, double_dqn):
    cin, cout, B = 10, 1, 4
    transitions = step_transitions(cin, cout, B, 7)
    order = ([3, 0, 1, 2], [1, 2, 0, 3])
    a = two_steps(S, L, cin, cout, B, {'deterministic': 1, 'stem_bf16': 2}, 'fp32', transitions, order, double_dqn)
    b = two_steps(S, L, cin, cout, B, {'deterministic': 1, 'stem_bf16': 2, 'bf16_states': 1}, 'bf16', transitions, order, double_dqn)
    assert_same_steps(a, b)
    nfwd = a['families'].get('stem_conv_bf16_wide', 0)                          # (grad-mode, target and -- double DQN -- the no-grad policy forward)
    assert nfwd >= 2 and a['families'].get('stem_wgrad_bf16_wide', 0) == 1, a['families']
    assert b['families'].get('stem_conv_bf16_wide_x16', 0) == nfwd and b['families'].get('stem_wgrad_bf16_wide_x16', 0) == 1, b['families']
    assert not [k for k in b['families'] if k in ('stem_conv_bf16_wide', 'stem_wgrad_bf16_wide', 'stem_conv_bf16', 'stem_wgrad_bf16')], b['families']
    assert a['families'].get('igemm_f32_gather', 0) == 0 and b['families'].get('igemm_f32_gather', 0) == 0


def test_policy_acts_on_a_bf16_pool_of_ten_channel_states(S):
    C = 10
    base = dict(robot_config=[{'lifting_robot': 3}, {'pushing_robot': 1}], num_input_channels=C, final_exploration=0.01, checkpoint_path=None,
                simq_precision='bf16')
    ref = S.DQNPolicy(types.SimpleNamespace(simq_plan_options={'stem_bf16': 2}, **base), train=False, random_seed=3)
    pol = S.DQNPolicy(types.SimpleNamespace(simq_plan_options={'stem_bf16': 2, 'bf16_states': 1}, **base), train=False, random_seed=3)
    for a, b in zip(ref.policy_nets, pol.policy_nets):
        assert a.plan.bf16_states == 0 and b.plan.bf16_states == 1 and a.plan.options['stem_bf16'] == b.plan.options['stem_bf16'] == 2
        b.load_state_dict(a.state_dict())
        a.eval(); b.eval()
    envs = tdt.policy_envs(C, 51)
    ring32 = S.AliasedDeviceReplayBuffer(8, C, pool_slots=12)
    ring16 = S.AliasedDeviceReplayBuffer(8, C, pool_slots=12, dtype='bf16')
    h32, h16 = tdt.adopt_structure(ring32, envs, set()), tdt.adopt_structure(ring16, envs, set())
    random.seed(17)
    want = ref.step_many(h32, exploration_eps=0.0)
    random.seed(17)
    assert pol.step_many(h16, exploration_eps=0.0) == want
    assert any(a is not None for st in want for g in st for a in g)


def test_a_bf16_batch_of_ten_channel_states_needs_the_option(S, L):
    import simq.learner as sl
    from oracle import cases as c
    cin, cout, B = 10, 1, 4
    policy, target = S.FCN(cin, cout, precision='bf16', options=OPT), S.FCN(cin, cout, precision='bf16', options=OPT)
    policy.train(); target.eval()
    # (wide-stem nets: their weight cache holds the wide layout)
    assert L._c.simq_wcache_bytes(policy.plan.handle) - L._c.simq_wcache_bytes(L.Plan(cin, cout, 'bf16').handle) == wide_bytes(L)
    ring = S.AliasedDeviceReplayBuffer(8, cin, pool_slots=16, dtype='bf16')
    for t in step_transitions(cin, cout, B, 9):
        ring.push(*t)
    batch = ring.gather([0, 1, 2, 3])
    torch.cuda.synchronize()
    L.lib.c.simq_launch_counts_reset()
    with pytest.raises(L.SimqError, match=r'bf16_states.*\.float\(\)'):
        sl.train_step(policy, target, batch, c.GAMMA, B, c.LR, c.MOMENTUM, c.WEIGHT_DECAY, c.CLIP)
    assert L.launch_counts() == {}
