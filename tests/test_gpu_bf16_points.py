"""GPU: the plain-bf16 plan against its MODEL -- oracle/bf16_points.py: the reference network (networks.py:16-26, resnet.py:31-47,
train.py:108-141) in fp64 arithmetic with operands rounded to bf16 exactly where the plan rounds them.

The reference defines bf16 only through torch.autocast, whose own gradient is 0.4-0.6 off fp64 on these nets: the calibrated bars of
tests/test_gpu_sized.py / test_gpu_fcn.py (<= 1.5 x that) cannot see a wrong bf16 kernel at network level.  Against the model what is
left is the kernels' own: fp32 instead of fp64 between two rounding points and the accumulation order -- 1e-7 relative at the source.
It does not stay 1e-7, and it cannot: a value within fp32-accumulation distance (~1e-6 of the range) of a bf16 rounding boundary rounds the
other way -- measured 0.01-0.02 % of the elements of every stored convolution output (the teacher-forced test below), one bf16 ulp (0.4-0.8 %
of the value) each: storage in bf16 turns a 1e-6 round-off into differences 1e3 times its size on a few elements per ten thousand, whatever
computes it.  Through 20 layers that is 3e-3 (rel-L2) on an eval-mode Q-map, and the train-mode BatchNorm / ReLU chain amplifies it to 3e-2
on a train-mode Q-map and 0.2-0.3 on the gradient (tests/diag/diag_bf16_points.py: stem output 1e-5, eval Q 2.9e-3, train Q 2.7e-2 against the model; against plain
fp64 2.2e-3 / 3.6e-3 / 6.3e-2).  So the model halves the distance the autocast calibration leaves (gradient 0.23-0.28 instead of 0.41-0.58),
it cannot make a 1e-3 oracle out of a chaotic system -- the tight network-level check is the TEACHER-FORCED one at the end of this file, where
every stored tensor is recomputed from the stored tensors it was made from and a differing rounding cannot propagate (bars of a single
kernel: conv 1 % flips of one ulp, elementwise bit-exact).  Bars against the model, with what was measured at B = 64 / 128:
  q_sa                  <= 8e-2 of the range        (measured 1.5e-2 / 3.2e-2; model vs fp64 3-7e-2)
  loss, TD error        <= 1 %                       (5e-4 .. 2e-3)
  TD targets            <= 3e-2 (2e-3 typical), at most 5 % of the transitions beyond it (a flipped double-DQN greedy action)
  gradient              per-tensor norms <= 15 % (5-8 %), sampled elements rel-L2 <= 0.40 (0.23-0.28; HIP bf16 vs fp64: 0.41-0.58), total norm 3 %
The teacher-forced walks cover all three forwards of a bf16 TD step: the grad-mode forward and the backward here; the policy's no-grad
train-mode forward, the target net's folded eval forward (what DQNPolicy.step acts with) and the two unfolded eval forms in
tests/test_gpu_bf16_eval_points.py, which runs walk_blocks_forward / walk_stem_and_head_forward below in the other modes.
The fixtures (tests/golden/bf16pts_*.npz, oracle/gen_golden.py bf16_points) were validated in the build container: with the rounding
points off the model IS the fp64 oracle (1e-12), with them on it lands inside the reference's autocast calibration.
"""
import os

import numpy as np
import pytest
import torch

from oracle import bf16_points as bp
from oracle import cases
from oracle import fcn as ofcn
from oracle import learner as olearner
from simq import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def simq_mod():
    import simq
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return simq


def rl2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def hip_step(simq_mod, cin, cout, B, wseed, dseed):
    cfg, batch = cases.make_cfg(B), cases.make_batch(cin, cout, B, dseed)
    policy, target = simq_mod.FCN(cin, cout, precision='bf16'), simq_mod.FCN(cin, cout, precision='bf16')
    policy.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, wseed)))
    target.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, wseed + 1000)))
    policy.train(); target.eval()
    opt = torch.optim.SGD(policy.parameters(), lr=cases.LR, momentum=cases.MOMENTUM, weight_decay=cases.WEIGHT_DECAY)
    info = simq_mod.train(cfg, policy, target, opt, batch, olearner.apply_transform, cases.GAMMA)
    tn = float(policy._simq_opt_state.total_norm.item())
    coef = min(1.0, cases.CLIP / (tn + 1e-6))
    grads = [v.detach().cpu().double() / coef for v in policy.reference_views(policy.flat_grads)]
    gs = np.stack([t.reshape(-1)[torch.tensor(cases.sample_indices(t.numel()))].numpy() for t in grads])
    sd = policy.state_dict()
    bn = np.concatenate([sd[k].detach().double().cpu().numpy().ravel() for k in sd if k.endswith('running_mean') or k.endswith('running_var')])
    return dict(info=info, total_norm=tn, grad=gs, gnorm=np.array([float(t.norm()) for t in grads]), q=policy._last['q'].detach().cpu().double().numpy(),
                q_sa=policy._last['q_sa'].cpu().numpy(), y=policy._last['y'].cpu().numpy(), bn=bn)


def judge(tag, h, m):
    """h: HIP results; m: the model's (loss, td_error, q_sa, y, grad_norm, grad [, q])."""
    e = dict(loss=abs(h['info']['loss'] - float(m['loss'])) / abs(float(m['loss'])),
             td=abs(h['info']['td_error'] - float(m['td_error'])) / abs(float(m['td_error'])),
             q_sa=relmax(h['q_sa'], m['q_sa']), grad=rl2(h['grad'], m['grad']),
             tn=abs(h['total_norm'] - float(m['total_norm'])) / float(m['total_norm']))
    big = m['grad_norm'] > 1e-3 * m['grad_norm'].max()
    e['gnorm'] = float((np.abs(h['gnorm'] - m['grad_norm']) / m['grad_norm'])[big].max())
    dy = np.abs(np.asarray(h['y'], np.float64) - m['y'])
    flipped = dy > 3e-2 * np.abs(m['y']).max()
    e['y_close'] = float(dy[~flipped].max() / np.abs(m['y']).max()) if (~flipped).any() else 0.0
    e['y_flipped'] = int(flipped.sum())
    print('\n%s: HIP bf16 vs the bf16-points model -- loss %.3g, td %.3g, q_sa %.3g, TD targets %.3g (%d of %d on another greedy action), '
          'gradient: sampled rel-L2 %.3g, worst per-tensor norm %.3g, total norm %.3g' % (tag, e['loss'], e['td'], e['q_sa'], e['y_close'], e['y_flipped'],
                                                                                       len(dy), e['grad'], e['gnorm'], e['tn']))
    return e


def test_bf16_step_against_the_model_live_b8(simq_mod):
    """Small batch, model evaluated on this host: the full Q-map, q_sa, TD targets, loss, gradient and BatchNorm buffers of one TD step."""
    cin, cout, B, wseed, dseed = 5, 2, 8, 33, 43
    h = hip_step(simq_mod, cin, cout, B, wseed, dseed)
    cfg, batch, spec = cases.make_cfg(B), cases.make_batch(cin, cout, B, dseed), ofcn.state_spec(cin, cout)
    gk = olearner.grad_keys(spec)
    st, tg = cases.oracle_state(cin, cout, wseed, torch.float64), cases.oracle_state(cin, cout, wseed + 1000, torch.float64)
    ex = {}
    info = bp.train_step(cfg, st, tg, spec, [None] * len(gk), batch, cases.GAMMA, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, extras=ex)
    gs = np.stack([ex['grads'][k].reshape(-1)[torch.tensor(cases.sample_indices(ex['grads'][k].numel()))].numpy() for k in gk])
    m = dict(loss=info['loss'], td_error=info['td_error'], q_sa=ex['q'].numpy(), y=ex['y'].numpy(), total_norm=ex['total_norm'],
             grad_norm=np.array([float(ex['grads'][k].norm()) for k in gk]), grad=gs)
    e = judge('live B=8', h, m)
    qerr = relmax(h['q'], ex['output'].numpy())
    bnerr = relmax(h['bn'], cases.bn_buffer_vector(st))
    print('   full Q-map %.3g, BatchNorm buffers %.3g' % (qerr, bnerr))
    # (8 samples: train-mode BatchNorm over 8 x 576 rows -- the chaotic end of the range; measured Q 3.2e-2, q_sa 0.11, gradient 0.34)
    assert qerr < 0.1 and e['q_sa'] < 0.3 and bnerr < 5e-3
    assert e['y_close'] < 3e-2 and e['y_flipped'] <= 2
    if e['y_flipped'] == 0:
        assert e['loss'] < 5e-2 and e['grad'] < 0.7 and e['gnorm'] < 0.3


@pytest.mark.parametrize('case', cases.TRAIN_CASES_SIZED[:2], ids=[c[0] for c in cases.TRAIN_CASES_SIZED[:2]])
def test_bf16_step_against_the_model_at_config_sizes(simq_mod, case):
    """configs[2] / configs[4]'s per-GPU shape (128 transitions) and configs[3]'s (64): the committed model fixtures."""
    name, cin, cout, B, wseed, dseed = case
    path = os.path.join(cases.GOLDEN_DIR, 'bf16pts_' + name + '.npz')
    m = np.load(path)
    h = hip_step(simq_mod, cin, cout, B, wseed, dseed)
    e = judge(name, h, m)
    print('   (the model itself vs fp64 on this batch: q_sa %.3g, loss %.3g, sampled gradient %.3g)' % tuple(m['vs_fp64'][:3]))
    assert relmax(h['bn'], m['bn_buffers']) < 5e-3
    assert e['q_sa'] < 8e-2 and e['y_close'] < 3e-2 and e['y_flipped'] <= max(1, B // 20)
    assert e['loss'] < 1e-2 + 0.02 * e['y_flipped'] and e['td'] < 1e-2 + 0.02 * e['y_flipped']
    assert e['gnorm'] < 0.15 and e['grad'] < 0.40 and e['tn'] < 3e-2


def test_bf16_dense_gradient_against_the_model(simq_mod):
    """loss = sum(Q * R) for the dense R of cases.DENSE_GRAD_CASES[0] (the autograd path, simq_backward with a dense upstream
    gradient): no TD targets, no greedy actions -- forward and backward walk alone."""
    name, cin, cout, B, wseed, dseed = cases.DENSE_GRAD_CASES[0]
    m = np.load(os.path.join(cases.GOLDEN_DIR, 'bf16pts_' + name + '.npz'))
    net = simq_mod.FCN(cin, cout, precision='bf16')
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, wseed)))
    net.train()
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, cin, dseed)]).cuda()
    R = torch.from_numpy(cases.dense_upstream(cout, B, dseed)).cuda()
    q = net(x)
    (q * R).sum().backward()
    grads = [p.grad.detach().cpu().double() for p in net.parameters() if p.grad is not None]
    spec = ofcn.state_spec(cin, cout)
    assert len(grads) == len(olearner.grad_keys(spec))
    gs = np.stack([t.reshape(-1)[torch.tensor(cases.sample_indices(t.numel()))].numpy() for t in grads])
    qd = q.detach().cpu().double()
    qs = qd.reshape(-1)[torch.tensor(cases.sample_indices(qd.numel(), 4096))].numpy()
    gn = np.array([float(t.norm()) for t in grads])
    big = m['grad_norm'] > 1e-3 * m['grad_norm'].max()
    e_q, e_g, e_n = relmax(qs, m['q_sample']), rl2(gs, m['grad']), float((np.abs(gn - m['grad_norm']) / m['grad_norm'])[big].max())
    chk = abs(float((qd * R.cpu().double()).sum()) - m['q_checksum'][2]) / abs(m['q_checksum'][2])
    print('\n%s: HIP bf16 vs the model -- Q (4096 samples) %.3g, sum(Q*R) %.3g, gradient sampled rel-L2 %.3g, worst per-tensor norm %.3g '
          '(the model vs fp64: Q %.3g, gradient %.3g)' % (name, e_q, chk, e_g, e_n, m['vs_fp64'][0], m['vs_fp64'][1]))
    assert e_q < 8e-2 and chk < 6e-2              # (measured 2.8-2.9e-2 / 7e-3 .. 2.4e-2 -- sum(Q * R) cancels, it moves with any change of a summation order; the model vs fp64 7e-2)
    assert e_g < 0.40 and e_n < 0.15              # (measured 0.25 / 6.5e-2; HIP vs fp64 0.38-0.43, the reference under autocast 0.41-0.60)


def _fma32(y, sc, sh):
    """fp32 fma(y, sc[c], sh[c]) emulated through fp64 (exact product and sum, one rounding; double rounding only on exact half-way cases)."""
    return (y.double() * sc.double() + sh.double()).float()


def _host_threads():
    """fp64 reference convolutions on the host: capped (MKL's dgemm beyond ~32 threads gets SLOWER on the 256-CPU boxes)."""
    return max(1, min(32, os.cpu_count() or 1))


def _check_conv(name, got16, ref64, log):
    """stored bf16 value == bf16(fp64 convolution of the stored bf16 operands) except where fp32 accumulation crosses a rounding boundary:
    < 1 % of the elements, each one bf16 ulp."""
    want = ref64.to(torch.bfloat16)
    frac = float((got16 != want).double().mean())
    worst = float(((got16.double() - ref64).abs() / ref64.abs().clamp_min(1e-2 * float(ref64.abs().max()))).max())
    log.append('  %-22s %.4f %% of the stored elements differ from bf16(fp64), worst %.3g of the value' % (name, 100 * frac, worst))
    assert frac < 1e-2 and worst < 2 ** -7, (name, frac, worst)


# kernel families (include/simq.h: the launch log) the bench's batch size is meant to select, and must have selected, in these tests
_FWD_FAMILIES_B128 = ('igemm_bf16_img_whole', 'igemm_bf16_img_half', 'igemm_bf16_c64', 'stem_conv_bf16', 'bn_apply16')
_BWD_FAMILIES_B128 = ('igemm_bf16_img_whole', 'igemm_bf16_img_half', 'igemm_bf16_c64', 'wgrad_bf16_img', 'wgrad_bf16_reg', 'stem_wgrad_bf16',
                      'bn_bwd_apply16', 'bn_bwd_apply16_mask_from_y')


def _forward_mode(mode):
    from simq import _lib
    return {'train': _lib.MODE_TRAIN, 'nograd': _lib.MODE_TRAIN_NOGRAD, 'eval': _lib.MODE_EVAL}[mode]


def _eval_coeff32(sd, bnkey):
    """scale | shift of an eval-mode BatchNorm as the consuming kernel forms them (bn_coeff.h: fp64 from the running statistics, rounded once)"""
    sc = sd[bnkey + '.weight'].double() / torch.sqrt(sd[bnkey + '.running_var'].double() + 1e-5)
    return sc.float(), (sd[bnkey + '.bias'].double() - sd[bnkey + '.running_mean'].double() * sc).float()


def walk_blocks_forward(simq_mod, B, mode='train', options=None):
    """The body of test_bf16_forward_teacher_forced_block_by_block for ONE forward in `mode`: 'train' (workspace slot 'train'), 'nograd'
    (MODE_TRAIN_NOGRAD, slot 'tmp': the policy's forward over the next states) or 'eval' on a plan whose `options` switch the folded eval
    form off (fold_eval_bn_bf16 = 0 / keep_fp32_activations = 1: bn_apply16 / bn_apply with coefficients from the running statistics).
    Returns (Q, launch log)."""
    import torch.nn.functional as F
    from simq import _lib
    cin, cout = 5, 2
    slot = 'train' if mode == 'train' else 'tmp'
    net = simq_mod.FCN(cin, cout, precision='bf16', options=options)
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, 77)))
    net.train()
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, cin, 78)]).permute(0, 2, 3, 1).contiguous().cuda()
    net._ensure_weights()
    _lib.lib.call('simq_launch_counts_reset')
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    q = net._forward_raw(x, _forward_mode(mode))
    torch.cuda.synchronize()
    ran = _lib.launch_counts()
    print('\n  B = %d %s forward launch log: %s' % (B, mode, ', '.join('%s x %d' % kv for kv in sorted(ran.items()))))
    if B == 128 and mode != 'eval':
        missing = [f for f in _FWD_FAMILIES_B128 if ran.get(f, 0) == 0]
        assert not missing, 'B = 128 forward did not select %s (ran: %s)' % (missing, ran)
        assert ran.get('igemm_bf16_pp', 0) + ran.get('igemm_bf16_dma', 0) > 0          # the 1x1 downsample / head convolutions: large LDS-DMA tiles
    keep_threads = torch.get_num_threads()
    torch.set_num_threads(_host_threads())
    try:
        sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        nchw = lambda t: t.permute(0, 3, 1, 2)
        stored = lambda name: net.stored_tensor(name, B, slot).cpu()
        rnd = lambda t: t.to(torch.bfloat16)
        log = []

        def check_bn(name, aux, ref64, gamma, beta):
            if mode == 'eval':                                   # running statistics (bn_coeff: fp64, rounded once); nothing stores them, and they stay
                bnkey = gamma[:-len('.weight')]
                assert torch.equal(sd[bnkey + '.running_mean'], sd0[bnkey + '.running_mean']) and torch.equal(sd[bnkey + '.running_var'], sd0[bnkey + '.running_var']), name
                return _eval_coeff32(sd, bnkey)
            gamma, beta = sd[gamma], sd[beta]
            mean = ref64.mean(dim=(0, 2, 3))
            var = ref64.var(dim=(0, 2, 3), unbiased=False)
            invstd = 1.0 / torch.sqrt(var + 1e-5)
            rng = float(ref64.abs().max())
            assert float((aux[2].double() - mean).abs().max()) < 2e-5 * rng and relmax(aux[3], invstd) < 2e-5, name
            sc = gamma.double() * aux[3].double()
            assert relmax(aux[0], sc) < 1e-6 and float((aux[1].double() - (beta.double() - aux[2].double() * sc)).abs().max()) < 1e-5 * max(1.0, float(sc.abs().max()) * rng), name
            return aux[0], aux[1]

        def check_exact(name, got, want32):
            want = want32 if got.dtype == torch.float32 else want32.to(torch.bfloat16)      # (keep_fp32_activations = 1: the fp32 copy is what is stored)
            frac = float((got != want).double().mean())
            log.append('  %-22s %.5f %% of the elements differ from the bit-exact emulation' % (name, 100 * frac))
            assert frac < 1e-4, name
        cur16 = stored('stem.pool.plane')
        cur_id = net.saved_activation('stem.pool', B, slot).cpu()          # fp32: block 1's identity shortcut
        assert torch.equal(cur16, cur_id.to(torch.bfloat16))
        r = 'module.resnet18.'
        for li in range(1, 5):
            for bi in range(2):
                b, key = 'layer%d.%d' % (li, bi), '%slayer%d.%d.' % (r, li, bi)
                xin = nchw(cur16.double())
                y1 = stored(b + '.y1')
                y1ref = F.conv2d(xin, rnd(sd[key + 'conv1.weight']).double(), padding=1)
                _check_conv(b + '.conv1', nchw(y1), y1ref, log)
                a1x = check_bn(b + '.bn1', stored(b + '.bn1'), y1ref, key + 'bn1.weight', key + 'bn1.bias')
                a1 = stored(b + '.a1')
                check_exact(b + '.a1', a1, torch.relu(_fma32(y1.float(), a1x[0], a1x[1])))
                y2 = stored(b + '.y2')
                y2ref = F.conv2d(nchw(rnd(a1).double()), rnd(sd[key + 'conv2.weight']).double(), padding=1)
                _check_conv(b + '.conv2', nchw(y2), y2ref, log)
                a2x = check_bn(b + '.bn2', stored(b + '.bn2'), y2ref, key + 'bn2.weight', key + 'bn2.bias')
                if (key + 'downsample.0.weight') in sd:
                    yd = stored(b + '.yd')
                    ydref = F.conv2d(xin, rnd(sd[key + 'downsample.0.weight']).double())
                    _check_conv(b + '.downsample', nchw(yd), ydref, log)
                    adx = check_bn(b + '.bnd', stored(b + '.bnd'), ydref, key + 'downsample.1.weight', key + 'downsample.1.bias')
                    identity = _fma32(yd.float(), adx[0], adx[1])
                else:
                    identity = cur_id.float()
                out = stored(b + '.out')
                v = (_fma32(y2.float(), a2x[0], a2x[1]).double() + identity.double()).float()
                check_exact(b + '.out', out, torch.relu(v))
                cur16, cur_id = rnd(out), out.float()
        print('\n'.join(log))
    finally:
        torch.set_num_threads(keep_threads)
    return q.cpu(), ran


@pytest.mark.parametrize('B', [6, 29, 128], ids=['b6', 'b29', 'b128'])
def test_bf16_forward_teacher_forced_block_by_block(simq_mod, B):
    """Network-level and flip-free: after ONE train-mode forward of the bf16 plan every tensor the residual blocks STORE (pre-BatchNorm outputs,
    the activation between the two convolutions, the block output, the BatchNorm coefficients) is recomputed in fp64 from the stored tensors it
    was computed from (simq_workspace_tensor_ex) -- a rounding that differs from the model's cannot propagate, so the bars are those of a
    single kernel:
      convolutions   stored bf16 value == bf16(fp64 convolution of the stored bf16 operands) except where fp32 accumulation crosses a rounding
                     boundary: < 1 % of the elements, each one bf16 ulp;
      BatchNorm      mean / invstd against the statistics of the fp64 convolution output at 2e-5; scale / shift = their gamma / beta form;
      elementwise    a1 = bf16(relu(fma(y1, scale, shift))) and out = bf16(relu(fma(y2, scale2, shift2) + identity)) -- identity = the stored
                     plane, the fp32 pooled map (block 1) or fma(yd, scale_d, shift_d) -- BIT-EXACT up to a 1e-4 fraction of half-way cases.
    This is what would catch a wrong residual plane, mask / activation plane, or bn_apply16 at network level (resnet.py:31-47).
    B = 128 is the batch the bench's bf16 leg runs (configs[2], configs[4] per GPU): only there are the whole-map image tile, the half-map
    tile of the 128-channel layers, the LDS-resident kernel of the 64-input-channel layers and the large-tile 1x1 kernels selected -- asserted
    through the launch log (B = 6 / 29 run the register-staged and 288-row LDS-DMA tiles instead)."""
    walk_blocks_forward(simq_mod, B, 'train')


@pytest.mark.parametrize('B', [6, 29, 128], ids=['b6', 'b29', 'b128'])
def test_bf16_backward_teacher_forced_block_by_block(simq_mod, B):
    """The backward walk of the bf16 plan (loss.backward(), train.py:132, through resnet.py:31-47 reversed), network-level and flip-free: after
    ONE train-mode forward and ONE backward with a dense seeded upstream gradient every gradient tensor the walk produces inside a residual
    block (simq_backward_traced keeps them; the walk itself reuses four temporaries) and every parameter gradient of the block is recomputed
    in fp64 from the STORED tensors it was made from -- the forward's stored bf16 tensors (simq_workspace_tensor_ex) and the traced bf16
    gradients -- so that a rounding which differs from the recomputation's cannot propagate and every comparison has a single kernel's bar:
      g_out -> [out > 0] -> BatchNorm-2 backward (dy2; dz for the identity shortcut; dyd through the downsample BatchNorm) -> conv2's data
      gradient (da1) -> ReLU mask from the stored PRE-BatchNorm output y1 (bn1_mask_from_preact: fma(y1, scale, shift) > 0) -> BatchNorm-1
      backward (dy1) -> conv1's data gradient + shortcut (g_in), and each layer's weight gradient = conv2d_weight(stored bf16 x, stored bf16 dy).
    Bars:
      stored bf16 gradient planes == bf16(fp64 recomputation) on all but < 1 % of the elements, each within one bf16 ulp;
      convolution weight gradients 2e-5 (max-abs over max-abs) against fp64 on the stored operands;
      the BatchNorm backward sums [sum dz | sum dz*xhat] the fused dgrad epilogues leave (formed from the fp32 values BEFORE they are rounded
      to the stored bf16): within the rounding noise of that storage -- a bf16 rounding error is uniform within half an ulp, 0.6-1.2 x
      2^-9 |v| in standard deviation, so the sum over a channel's rows has sigma ~ 0.8 x 2^-9 ||dz||_2; measured 2.8-3.0 of that unit as the
      maximum over the 6 000 channel sums of the walk (3.7 sigma), bar 6 -- a wrong mask source / y plane / mean moves them by ~sqrt(rows) x
      512 of that unit --, and d gamma / d beta == (float)those sums.
    g_in of block k must equal g_out of block k - 1 bit for bit (same buffer).  B = 128 is the bench's batch: the image-tile dgrad / weight-
    gradient kernels, the LDS-resident 64-channel dgrad and bn_bwd_apply16<mask from y> are selected only there (asserted, launch log)."""
    import torch.nn.functional as F
    from simq import _lib
    from simq._lib import MODE_TRAIN
    cin, cout = 5, 2
    net = simq_mod.FCN(cin, cout, precision='bf16')
    assert net.plan.options['bn1_mask_from_preact'] == 1 and net.plan.options['bf16_act_grads'] == 1
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, 81)))
    net.train()
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, cin, 82)]).permute(0, 2, 3, 1).contiguous().cuda()
    q = net._forward_raw(x, MODE_TRAIN)
    dq = torch.from_numpy(cases.dense_upstream(cout, B, 83)).cuda().contiguous()
    assert dq.shape == q.shape
    _lib.lib.call('simq_launch_counts_reset')
    grads_flat, traced = net.backward_traced(dq, B)
    torch.cuda.synchronize()
    ran = _lib.launch_counts()
    print('\n  B = %d backward launch log: %s' % (B, ', '.join('%s x %d' % kv for kv in sorted(ran.items()))))
    if B == 128:
        missing = [f for f in _BWD_FAMILIES_B128 if ran.get(f, 0) == 0]
        assert not missing, 'B = 128 backward did not select %s (ran: %s)' % (missing, ran)
        assert ran['bn_bwd_apply16_mask_from_y'] == 8                                     # bn1 of every block: the mask recomputed from y1
    gview = {k: v.detach().cpu().double() for (k, _, _), v in zip(net._param_names, net.reference_views(grads_flat))}
    keep_threads = torch.get_num_threads()
    torch.set_num_threads(_host_threads())
    try:
        sd = {k[len('module.'):]: v.detach().cpu() for k, v in net.state_dict().items()}
        nchw = lambda t: t.permute(0, 3, 1, 2)
        stored = lambda name: net.stored_tensor(name, B, 'train').cpu()
        tr = lambda name: traced(name).cpu()
        w64 = lambda k: sd[k].to(torch.bfloat16).double()
        log = []
        M = B * 576

        def check_wgrad(key, x16, dy16, pad):
            want = torch.nn.grad.conv2d_weight(nchw(x16.double()), tuple(sd[key].shape), nchw(dy16.double()), padding=pad)
            err = float((gview[key] - want).abs().max() / want.abs().max())
            log.append('  %-38s weight gradient vs fp64 on the stored operands %.2e' % (key, err))
            assert err < 2e-5, (key, err)

        def check_sums(name, red, dz64, y16, aux, gkey, bkey):
            """red [2, C] fp64 as the dgrad epilogue left them; dz64 [B,24,24,C] = stored bf16 gradient x mask; xhat from the stored pre-BN output"""
            xhat = (y16.double() - aux[2].double()) * aux[3].double()
            s0, s1 = dz64.sum(dim=(0, 1, 2)), (dz64 * xhat).sum(dim=(0, 1, 2))
            n0 = 2.0 ** -9 * torch.sqrt((dz64 ** 2).sum(dim=(0, 1, 2))).clamp_min(1e-30)
            n1 = 2.0 ** -9 * torch.sqrt(((dz64 * xhat) ** 2).sum(dim=(0, 1, 2))).clamp_min(1e-30)
            e0, e1 = float(((red[0] - s0).abs() / n0).max()), float(((red[1] - s1).abs() / n1).max())
            l1 = float(((red[0] - s0).abs() / dz64.abs().sum(dim=(0, 1, 2)).clamp_min(1e-30)).max())
            log.append('  %-22s sums vs the stored tensors: %.2f / %.2f of the bf16-storage noise 2^-9 ||dz||_2 (%.1e of sum |dz|)' % (name, e0, e1, l1))
            assert e0 < 6.0 and e1 < 6.0, (name, e0, e1)
            assert float((gview[bkey] - red[0].float().double()).abs().max()) <= 1e-6 * float(red[0].abs().max()), bkey      # d beta = sum dz
            assert float((gview[gkey] - red[1].float().double()).abs().max()) <= 1e-6 * float(red[1].abs().max()), gkey      # d gamma = sum dz*xhat
            return xhat

        def bn_backward(dz64, xhat, red, gamma, aux):
            """dy = gamma * invstd * (dz - sum(dz) / M - xhat * sum(dz*xhat) / M) with the STORED sums (elementwise.hip bn_bwd_apply)"""
            return gamma.double() * aux[3].double() * (dz64 - red[0] / M - xhat * red[1] / M)
        prev_g_in = None
        for li in range(4, 0, -1):
            for bi in (1, 0):
                b, key = 'layer%d.%d' % (li, bi), 'resnet18.layer%d.%d.' % (li, bi)
                has_ds = (key + 'downsample.0.weight') in sd
                xin16 = stored('layer%d.%d.out' % ((li, 0) if bi == 1 else (li - 1, 1))) if (li, bi) != (1, 0) else stored('stem.pool.plane')
                y1, a1, y2, out = stored(b + '.y1'), stored(b + '.a1'), stored(b + '.y2'), stored(b + '.out')
                bn1, bn2 = stored(b + '.bn1'), stored(b + '.bn2')
                red1, red2 = stored(b + '.red1').cpu(), stored(b + '.red2').cpu()
                g_out = tr(b + '.g_out')
                if prev_g_in is not None:
                    assert torch.equal(g_out, prev_g_in), b + ': the gradient the block receives is not the one the block above produced'
                # out = relu(bn2(y2) + identity): dz = g_out * [out > 0]
                dz64 = g_out.double() * (out.float() > 0).double()
                xhat2 = check_sums(b + '.bn2', red2, dz64, y2, bn2, key + 'bn2.weight', key + 'bn2.bias')
                _check_conv(b + '.dy2', tr(b + '.dy2'), bn_backward(dz64, xhat2, red2, sd[key + 'bn2.weight'], bn2), log)
                if has_ds:
                    yd, bnd, redd = stored(b + '.yd'), stored(b + '.bnd'), stored(b + '.redd').cpu()
                    xhatd = check_sums(b + '.bnd', redd, dz64, yd, bnd, key + 'downsample.1.weight', key + 'downsample.1.bias')
                    _check_conv(b + '.dyd', tr(b + '.dyd'), bn_backward(dz64, xhatd, redd, sd[key + 'downsample.1.weight'], bnd), log)
                else:
                    assert torch.equal(tr(b + '.dz'), dz64.to(torch.bfloat16)), b + '.dz: the masked gradient of the identity shortcut is not exact'
                dy2 = tr(b + '.dy2')
                check_wgrad(key + 'conv2.weight', a1, dy2, 1)
                da1 = tr(b + '.da1')
                _check_conv(b + '.da1', nchw(da1), F.conv_transpose2d(nchw(dy2.double()), w64(key + 'conv2.weight'), padding=1), log)
                # a1 = relu(bn1(y1)): the mask is recomputed from the stored pre-BN output with the forward's own scale / shift
                mask1 = (_fma32(y1.float(), bn1[0], bn1[1]) > 0)
                assert float((mask1 != (a1.float() > 0)).double().mean()) < 1e-6, b + ': the recomputed ReLU mask is not the mask of the stored activation'
                dz1 = da1.double() * mask1.double()
                xhat1 = check_sums(b + '.bn1', red1, dz1, y1, bn1, key + 'bn1.weight', key + 'bn1.bias')
                _check_conv(b + '.dy1', tr(b + '.dy1'), bn_backward(dz1, xhat1, red1, sd[key + 'bn1.weight'], bn1), log)
                dy1 = tr(b + '.dy1')
                check_wgrad(key + 'conv1.weight', xin16, dy1, 1)
                gin = F.conv_transpose2d(nchw(dy1.double()), w64(key + 'conv1.weight'), padding=1)
                if has_ds:
                    dyd = tr(b + '.dyd')
                    check_wgrad(key + 'downsample.0.weight', xin16, dyd, 0)
                    g_ds = tr(b + '.g_ds')
                    _check_conv(b + '.g_ds', nchw(g_ds), F.conv_transpose2d(nchw(dyd.double()), w64(key + 'downsample.0.weight')), log)
                    gin = gin + nchw(g_ds.double())
                else:
                    gin = gin + nchw(tr(b + '.dz').double())
                prev_g_in = tr(b + '.g_in')
                _check_conv(b + '.g_in', nchw(prev_g_in), gin, log)
        print('\n'.join(log))
    finally:
        torch.set_num_threads(keep_threads)


def _ulp_close32(name, got, want64, frac_bar=1e-3, log=None):
    """fp32 elementwise results against the fp64 emulation of the same fma / max: equal except on half-way cases of the double rounding."""
    want = want64.float()
    frac = float((got != want).double().mean())
    worst = float(((got.double() - want64).abs() / want64.abs().clamp_min(1e-3 * float(want64.abs().max()))).max())
    if log is not None:
        log.append('  %-22s %.5f %% of the fp32 elements differ from the emulation, worst %.2e of the value' % (name, 100 * frac, worst))
    assert frac < frac_bar and worst < 4e-7, (name, frac, worst)


def walk_stem_and_head_forward(simq_mod, B, mode='train'):
    """The body of test_bf16_stem_and_head_teacher_forced_forward for ONE forward in `mode`: 'train' (workspace slot 'train') or 'nograd'
    (MODE_TRAIN_NOGRAD, slot 'tmp').  Returns (Q, the stored z3 [B,Cout,48,48], conv3's bias)."""
    import torch.nn.functional as F
    from simq import _lib
    cin, cout = 5, 2
    ws_slot = 'train' if mode == 'train' else 'tmp'
    net = simq_mod.FCN(cin, cout, precision='bf16')
    assert net.plan.options['stem_bf16'] == 1
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, 91)))
    net.train()
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, cin, 92)]).permute(0, 2, 3, 1).contiguous().cuda()
    net._ensure_weights()
    _lib.lib.call('simq_launch_counts_reset')
    q = net._forward_raw(x, _forward_mode(mode))
    torch.cuda.synchronize()
    ran = _lib.launch_counts()
    assert ran.get('stem_conv_bf16', 0) == 1, ran
    keep_threads = torch.get_num_threads()
    torch.set_num_threads(_host_threads())
    try:
        sd = {k[len('module.'):]: v.detach().cpu() for k, v in net.state_dict().items()}
        nchw = lambda t: t.permute(0, 3, 1, 2)
        nhwc = lambda t: t.permute(0, 2, 3, 1)
        stored = lambda name: net.stored_tensor(name, B, ws_slot).cpu()
        rnd = lambda t: t.to(torch.bfloat16)
        log = []

        def check_bn(name, aux, ref64, gamma, beta):
            mean, var = ref64.mean(dim=(0, 2, 3)), ref64.var(dim=(0, 2, 3), unbiased=False)
            invstd = 1.0 / torch.sqrt(var + 1e-5)
            rng = float(ref64.abs().max())
            assert float((aux[2].double() - mean).abs().max()) < 2e-5 * rng and relmax(aux[3], invstd) < 2e-5, name
            sc = gamma.double() * aux[3].double()
            assert relmax(aux[0], sc) < 1e-6 and float((aux[1].double() - (beta.double() - aux[2].double() * sc)).abs().max()) < 1e-5 * max(1.0, float(sc.abs().max()) * rng), name
        # ---- stem
        y0 = stored('stem.y0')
        assert y0.dtype == torch.bfloat16 and tuple(y0.shape) == (B, 48, 48, 64)
        y0ref = F.conv2d(nchw(rnd(x.cpu()).double()), rnd(sd['resnet18.conv1.weight']).double(), stride=2, padding=3)
        _check_conv('stem.conv', nchw(y0), y0ref, log)
        aux0 = stored('stem.bn')
        check_bn('stem.bn', aux0, y0ref, sd['resnet18.bn1.weight'], sd['resnet18.bn1.bias'])
        a0 = torch.relu(_fma32(y0.float(), aux0[0], aux0[1]))
        pooled_ref, idx_ref = F.max_pool2d(nchw(a0), 3, 2, 1, return_indices=True)
        pooled = net.saved_activation('stem.pool', B, ws_slot).cpu()
        assert torch.equal(nchw(pooled), pooled_ref), 'stem.pool is not maxpool(relu(fma(y0, scale, shift))) bit for bit'
        assert torch.equal(stored('stem.pool.plane'), rnd(pooled))
        slot = nchw(stored('stem.idx')).long()
        py, px = torch.meshgrid(torch.arange(24), torch.arange(24), indexing='ij')
        flat = (2 * py - 1 + slot // 3) * 48 + (2 * px - 1 + slot % 3)
        assert torch.equal(flat, idx_ref), 'stem.idx is not the first maximal window slot'
        # ---- head
        out7 = stored('layer4.1.out')
        y1 = stored('head.y1')
        assert y1.dtype == torch.bfloat16
        y1ref = F.conv2d(nchw(out7.double()), rnd(sd['conv1.weight']).double(), sd['conv1.bias'].double())
        _check_conv('head.conv1', nchw(y1), y1ref, log)
        aux1 = stored('head.bn1')
        check_bn('head.bn1', aux1, y1ref, sd['bn1.weight'], sd['bn1.bias'])
        a1p = stored('head.a1.plane')
        want = rnd(torch.relu(_fma32(y1.float(), aux1[0], aux1[1])))
        frac = float((a1p != want).double().mean())
        log.append('  %-22s %.5f %% of the elements differ from the bit-exact emulation' % ('head.a1', 100 * frac))
        assert frac < 1e-4
        z2 = stored('head.z2')
        z2ref = F.conv2d(nchw(a1p.double()), rnd(sd['conv2.weight']).double(), sd['conv2.bias'].double())
        e = relmax(nchw(z2), z2ref)
        log.append('  %-22s conv2 + bias at 24x24 vs fp64 on the stored plane %.2e' % ('head.z2', e))
        assert e < 2e-5
        y2 = stored('head.y2')
        assert tuple(y2.shape) == (B, 48, 48, 32)
        y2ref = F.interpolate(nchw(z2.double()), scale_factor=2, mode='bilinear', align_corners=True)
        assert relmax(nchw(y2), y2ref) < 2e-6
        aux2 = stored('head.bn2')
        check_bn('head.bn2', aux2, nchw(y2.double()), sd['bn2.weight'], sd['bn2.bias'])
        a2ref = torch.relu(y2.double() * aux2[0].double() + aux2[1].double())
        if mode == 'train':
            a2 = net.saved_activation('head.a2', B, 'train').cpu()
            _ulp_close32('head.a2', a2, a2ref, log=log)
        else:                                                        # the no-grad forward never stores it, and the accessor says so: the Q-map
            with pytest.raises(_lib.SimqError):                      # below is then what conv3 makes of the stored y2 / bn2 (same bars)
                net.saved_activation('head.a2', B, ws_slot)
            a2 = a2ref.float()
        z3 = stored('head.z3').reshape(B, cout, 48, 48)              # (stored channel-major, like the Q-map it becomes)
        z3ref = F.conv2d(nchw(a2.double()), sd['conv3.weight'].double())
        e = relmax(z3, z3ref)
        log.append('  %-22s conv3 (fp32) at 48x48 vs fp64 on the stored activation %.2e' % ('head.z3', e))
        assert e < 1e-5
        qref = F.interpolate(z3.double(), scale_factor=2, mode='bilinear', align_corners=True) + sd['conv3.bias'].double().view(1, -1, 1, 1)
        assert relmax(q.cpu(), qref) < 2e-6
        # ... and the order the REFERENCE runs the last two stages in (networks.py:23-26: upsample, then conv3) gives the same Q-map
        qorder = F.conv2d(F.interpolate(nchw(a2.double()), scale_factor=2, mode='bilinear', align_corners=True), sd['conv3.weight'].double(), sd['conv3.bias'].double())
        assert relmax(q.cpu(), qorder) < 1e-5
        print('\n'.join(log))
    finally:
        torch.set_num_threads(keep_threads)
    return q.cpu(), z3, sd['conv3.bias']


@pytest.mark.parametrize('B', [6, 128], ids=['b6', 'b128'])
def test_bf16_stem_and_head_teacher_forced_forward(simq_mod, B):
    """Round 6 (verdict: the two teacher-forced walks started behind the stem and stopped in front of the head): the SAME bar for the first and
    the last kernels of the bf16 plan's train-mode forward.  Every stored tensor of the stem (resnet.py:94-97: 7x7 / stride-2 convolution on the
    bf16 matrix cores -> BatchNorm -> ReLU -> 3x3 / stride-2 max-pool) and of the head (networks.py:18-26, in the order the plan runs it --
    conv1 -> bn1 -> relu -> conv2 at 24x24 -> bilinear x2 -> bn2 -> relu -> conv3 at 48x48 -> bilinear x2 + bias: conv2 / conv3 commute with
    the bilinear maps, whose weights sum to 1) is recomputed in fp64 from the stored tensors it was made from:
      stem.y0        == bf16(fp64 conv7x7(bf16(x), bf16(w))) except < 1 % one-ulp flips; its BatchNorm statistics at 2e-5 (they come from the
                     UNROUNDED fp32 outputs); stem.pool == maxpool(relu(fma(y0, scale, shift))) BIT-exact in fp32, its bf16 plane its rounding,
                     stem.idx == the first maximal window slot (what the backward pass routes through);
      head.y1        == bf16(fp64 conv1x1(stored layer4.1.out plane, bf16(w1)) + b1) (< 1 % flips), bn1 at 2e-5, a1 plane bit-exact;
      head.z2        fp32: conv1x1(a1 plane, bf16(w2)) + b2 at 2e-5 (fp32 accumulation of exact bf16 products over K = 128);
      head.y2        its bilinear x2 (align_corners) at 1e-6; bn2 statistics of THAT tensor at 2e-5; a2 = relu(fma(y2, scale, shift)) at fp32 ulp;
      head.z3, q     conv3 (exact fp32 arithmetic: 32 -> Cout) at 1e-5 and the final bilinear x2 + bias at 1e-6 -- q is what FCN.forward returns."""
    walk_stem_and_head_forward(simq_mod, B, 'train')


@pytest.mark.parametrize('B', [6, 128], ids=['b6', 'b128'])
def test_bf16_stem_and_head_teacher_forced_backward(simq_mod, B):
    """... and of the backward walk (loss.backward(), train.py:132): the head's chain in front of layer4 and the stem's behind layer1, every
    traced gradient tensor and every parameter gradient recomputed in fp64 from the STORED operands (simq_backward_traced, round 6 names):
      conv3 + second bilinear (reference order, autograd in fp64 on the stored a2): d conv3.weight / bias, head.da2 at 1e-5;
      BatchNorm 2 backward (mask a2 > 0, xhat from the stored y2): head.dy2, d gamma / d beta at 2e-5; first bilinear transposed: head.dz2 at 1e-5,
      d conv2.bias = its pixel sum; conv2: weight gradient (bf16(dz2) x the stored a1 plane) and data gradient head.da1 (bf16(dz2) x bf16(w2)) at 2e-5;
      BatchNorm 1 backward (mask from the stored plane): head.dy1 at 2e-5, d gamma / d beta; conv1: bias / weight gradient (bf16(dy1) x the stored
      layer4.1.out plane) at 2e-5 and layer4.1.g_out == bf16(bf16(dy1) x bf16(w1)) with < 1 % one-ulp flips;
      stem: stem.dz == max-pool + ReLU backward of the stored layer1.0.g_in through the stored pre-BN output (autograd in fp64: same first-maximum
      routing) at 1e-6; stem.dy0 (a bf16 plane) == bf16(BatchNorm backward) with < 1 % flips, d gamma / d beta at 2e-5; the 7x7 weight gradient
      == conv2d_weight(bf16(x), stored dy0 plane) at 2e-5."""
    import torch.nn.functional as F
    from simq import _lib
    from simq._lib import MODE_TRAIN
    cin, cout = 5, 2
    net = simq_mod.FCN(cin, cout, precision='bf16')
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, 93)))
    net.train()
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, cin, 94)]).permute(0, 2, 3, 1).contiguous().cuda()
    q = net._forward_raw(x, MODE_TRAIN)
    dq = torch.from_numpy(cases.dense_upstream(cout, B, 95)).cuda().contiguous()
    _lib.lib.call('simq_launch_counts_reset')
    grads_flat, traced = net.backward_traced(dq, B)
    torch.cuda.synchronize()
    ran = _lib.launch_counts()
    assert ran.get('stem_wgrad_bf16', 0) == 1, ran
    gview = {k: v.detach().cpu().double() for (k, _, _), v in zip(net._param_names, net.reference_views(grads_flat))}
    keep_threads = torch.get_num_threads()
    torch.set_num_threads(_host_threads())
    try:
        sd = {k[len('module.'):]: v.detach().cpu() for k, v in net.state_dict().items()}
        nchw = lambda t: t.permute(0, 3, 1, 2)
        nhwc = lambda t: t.permute(0, 2, 3, 1)
        stored = lambda name: net.stored_tensor(name, B, 'train').cpu()
        tr = lambda name: traced(name).cpu()
        rnd = lambda t: t.to(torch.bfloat16)
        log = []

        def close(name, got, want, bar, scale=None):
            """scale: what the error is measured against when `want` itself cancels (the biases in front of a BatchNorm have a gradient that is
            zero in exact arithmetic: the sum over rows of a BatchNorm backward output) -- the sum of the magnitudes that were added"""
            e = float((got.double() - want).abs().max() / (want.abs().max() if scale is None else scale))
            log.append('  %-26s %.2e (bar %.0e)' % (name, e, bar))
            assert e < bar, (name, e)

        def bn_backward(name, g64, mask, y, aux, gamma, gkey, bkey, rows):
            dz = g64 * mask.double()
            xhat = (y.double() - aux[2].double()) * aux[3].double()
            s0, s1 = dz.sum(dim=(0, 1, 2)), (dz * xhat).sum(dim=(0, 1, 2))
            close(name + ' d beta', gview[bkey], s0, 2e-5)
            close(name + ' d gamma', gview[gkey], s1, 2e-5)
            return gamma.double() * aux[3].double() * (dz - s0 / rows - xhat * s1 / rows)
        # ---- conv3 + the second bilinear map, in the reference's order, differentiated by autograd in fp64 on the stored activation
        a2 = net.saved_activation('head.a2', B, 'train').cpu()
        A2 = nchw(a2.double()).contiguous().requires_grad_()
        w3, b3 = sd['conv3.weight'].double().requires_grad_(), sd['conv3.bias'].double().requires_grad_()
        F.conv2d(F.interpolate(A2, scale_factor=2, mode='bilinear', align_corners=True), w3, b3).backward(dq.cpu().double())
        close('conv3.weight', gview['conv3.weight'], w3.grad, 2e-5)
        close('conv3.bias', gview['conv3.bias'], b3.grad, 2e-5)
        da2 = tr('head.da2')
        close('head.da2', nchw(da2), A2.grad, 1e-5)
        # ---- BatchNorm 2 backward at 48x48, the first bilinear map transposed
        y2, aux2 = stored('head.y2'), stored('head.bn2')
        dy2 = tr('head.dy2')
        close('head.dy2', dy2, bn_backward('bn2', da2.double(), a2 > 0, y2, aux2, sd['bn2.weight'], 'bn2.weight', 'bn2.bias', B * 2304), 2e-5)
        Z = torch.zeros(B, 32, 24, 24, dtype=torch.float64, requires_grad=True)
        F.interpolate(Z, scale_factor=2, mode='bilinear', align_corners=True).backward(nchw(dy2.double()).contiguous())
        dz2 = tr('head.dz2')
        close('head.dz2', nchw(dz2), Z.grad, 1e-5)
        close('conv2.bias', gview['conv2.bias'], dz2.double().sum(dim=(0, 1, 2)), 1e-6, scale=float(dz2.double().abs().sum(dim=(0, 1, 2)).max()))
        # ---- conv2 (1x1, 128 -> 32) on the bf16 matrix cores: operands = the stored a1 plane and bf16(dz2)
        a1p, dz2b = stored('head.a1.plane'), rnd(dz2)
        close('conv2.weight', gview['conv2.weight'].reshape(32, 128), dz2b.double().reshape(-1, 32).t() @ a1p.double().reshape(-1, 128), 2e-5)
        da1 = tr('head.da1')
        close('head.da1', da1.reshape(-1, 128), dz2b.double().reshape(-1, 32) @ rnd(sd['conv2.weight']).double().reshape(32, 128), 2e-5)
        # ---- BatchNorm 1 backward at 24x24
        y1, aux1 = stored('head.y1'), stored('head.bn1')
        dy1 = tr('head.dy1')
        close('head.dy1', dy1, bn_backward('bn1', da1.double(), a1p.float() > 0, y1, aux1, sd['bn1.weight'], 'bn1.weight', 'bn1.bias', B * 576), 2e-5)
        close('conv1.bias', gview['conv1.bias'], dy1.double().sum(dim=(0, 1, 2)), 1e-6, scale=float(dy1.double().abs().sum(dim=(0, 1, 2)).max()))
        out7, dy1b = stored('layer4.1.out'), rnd(dy1)
        close('conv1.weight', gview['conv1.weight'].reshape(128, 512), dy1b.double().reshape(-1, 128).t() @ out7.double().reshape(-1, 512), 2e-5)
        g7 = tr('layer4.1.g_out')
        _check_conv('layer4.1.g_out', g7.reshape(-1, 512), dy1b.double().reshape(-1, 128) @ rnd(sd['conv1.weight']).double().reshape(128, 512), log)
        # ---- stem: max-pool + ReLU backward through the stored pre-BN output, BatchNorm backward, the 7x7 weight gradient
        y0, aux0 = stored('stem.y0'), stored('stem.bn')
        g0 = tr('layer1.0.g_in')
        V = nchw(_fma32(y0.float(), aux0[0], aux0[1]).double()).contiguous().requires_grad_()
        F.max_pool2d(torch.relu(V), 3, 2, 1).backward(nchw(g0.double()).contiguous())
        dz0 = tr('stem.dz')
        close('stem.dz', nchw(dz0), V.grad, 1e-6)
        dy0 = tr('stem.dy0')
        assert dy0.dtype == torch.bfloat16
        ones = torch.ones_like(dz0, dtype=torch.bool)
        _check_conv('stem.dy0', dy0, bn_backward('resnet18.bn1', dz0.double(), ones, y0, aux0, sd['resnet18.bn1.weight'], 'resnet18.bn1.weight',
                                                 'resnet18.bn1.bias', B * 2304), log)
        want = torch.nn.grad.conv2d_weight(nchw(rnd(x.cpu()).double()), tuple(sd['resnet18.conv1.weight'].shape), nchw(dy0.double()), stride=2, padding=3)
        close('resnet18.conv1.weight', gview['resnet18.conv1.weight'], want, 2e-5)
        print('\n'.join(log))
    finally:
        torch.set_num_threads(keep_threads)
