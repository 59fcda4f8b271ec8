"""GPU: the fp32 plan (what bench.py times) TEACHER-FORCED, kernel by kernel -- the fp32 counterpart of the walks at the end of
tests/test_gpu_bf16_points.py.  After ONE forward (and one traced backward with the dense upstream gradient of cases.dense_upstream) every
tensor the plan stores (simq_workspace_tensor_ex, storage 0) and every gradient the walk produces (simq_backward_traced) is recomputed in
fp64 from the STORED tensors it was made from: an error cannot propagate, so every comparison carries the bar of a single kernel instead of
the network-level bars (Q 1e-4, gradient "worst case 10 x", 5e-3 between two options) under which a wrong ReLU-mask source, a BatchNorm sum
over the wrong plane, a residual addend from the wrong buffer, a dropped halo row or a max-pool tie broken the wrong way move nothing.

Bars (each one the project's existing per-kernel bar for that form, none fitted to this file):
  convolutions, data gradients      max-abs error over max-abs value (test_gpu_ops.rel) against fp64 on the stored operands: 1e-5 direct /
                                    image-tile / 1x1 / F(2x2,3x3), 2e-5 F(4x4,3x3); which form a layer runs is the plan's rule
                                    (forward.hip conv_fwd, backward.hip conv_dgrad / conv_wgrad), restated in _fwd_form / _dgrad_form /
                                    _wgrad_form below and PROVEN by the launch log: the number of winograd_f4 / winograd_f2 /
                                    winograd_f4_wgrad / winograd_f2_wgrad launches must be the number of layers the rule names
  weight gradients                  1e-5 direct and F(2x2,3x3), 1e-4 the F(4x4,3x3) transform-domain form (test_gpu_bnfuse); stem 7x7 1e-5;
                                    conv3 weight / bias 1e-5; the biases in front of a BatchNorm (zero in exact arithmetic) 1e-5 of the sum of
                                    the magnitudes added (the bf16 walk's metric)
  elementwise (fma / add / max)     _ulp_close32: equal to the fp64 emulation of the same fma sequence but for double-rounding half-way cases
  bilinear x2                       _ulp_close32 against the emulation of the kernels' own expression, head.hip lerp2x: weights formed in
                                    fp32 (scale = (n-1)/(2n-1) in fp32; i0 = (int)(scale*o); l1 = scale*o - i0; l0 = 1 - l1; the last output
                                    row / column has i0 == i1: coinciding taps) and v = ly0*(lx0*v00 + lx1*v01) + ly1*(lx0*v10 + lx1*v11)
                                    evaluated the way the compiler contracts it (the first product of each sum fused: fma(l0, a, rn(l1*b)));
                                    the Q-map's kernel forms l1 with one rounding or with two, column by column (see _check_head_forward);
                                    the transposes (head.dz2, head.da2) 5e-6 of the range against the fp64 transpose of the same weights
  BatchNorm coefficients            mean (2e-5 of the range) / invstd (2e-5) against the fp64 statistics of the STORED pre-BN tensor, scale /
                                    shift = their gamma / beta form at 1e-6, running statistics (momentum 0.1, unbiased variance) 1e-6; eval
                                    mode: bn_eval_coeff_kernel's scale / shift from the running statistics at 1e-6
  BatchNorm backward sums           per channel |stored - fp64 sum of the stored / traced fp32 terms| <= n 2^-24 sum|term|, n = the largest
                                    number of terms a producing kernel adds in fp32 before its fp64 atomic (see _N_FP32_TERMS: 128); d gamma /
                                    d beta = (float) of the sums at 1e-6; BatchNorm input gradients 5e-6 (test_bn_relu_backward_against_fp64)
  max-pool                          value exact, idx == the FIRST maximal slot in scan order in EVERY window (unique or tied); tied windows
                                    must be >= 1 % of all windows so that the tie rule is exercised (post-ReLU zeros)

Batch sizes: 5 (F(2x2,3x3) everywhere, F(2x2,3x3) weight gradients, ragged M = 720), 8 (the smallest that takes F(4x4,3x3): 288 tiles),
32 (the bench's own selection: the 128x256 split-bf16 GEMM tile and the whole-plane-per-XCD walk), once per stage.

Where each stored name of include/simq.h (simq_workspace_tensor_ex / simq_backward_trace_tensor, fp32 plans) is checked:
  stem.y0 stem.bn stem.pool stem.idx                      _check_stem_forward
  layer<l>.<b>.y1 .y2 .yd .out .a1(eval) .bn1 .bn2 .bnd   _check_blocks_forward
  head.y1 head.bn1 head.a1(eval) head.z2 head.y2 head.bn2 head.a2 head.z3, Q     _check_head_forward
  layer<l>.<b>.g_out .dy2 .dz .dyd .da1 .dy1 .g_ds .g_in .red1 .red2 .redd      _check_blocks_backward
  head.da2 .dy2 .dz2 .da1 .dy1 head.red1 head.red2        _check_head_backward
  stem.dz stem.dy0 stem.red                               _check_stem_backward

MEASURED (MI355X; the worst value of each class over the whole walk at B = 5 / 8 / 32; every test prints its own):
  convolutions          direct / 1x1 / stem 9.5e-7 / 1.2e-6 / 1.1e-6, F(2x2,3x3) 1.1e-6 / 5.3e-7 / 6.2e-7, F(4x4,3x3) - / 6.2e-6 / 5.9e-6
  data gradients        direct 9.6e-7 / 1.1e-6 / 1.1e-6, F(2x2,3x3) 9.9e-7 / - / -, F(4x4,3x3) - / 5.5e-6 / 5.6e-6
  weight gradients      direct 5.2e-7 / 7.3e-7 / 7.7e-7, F(2x2,3x3) 1.2e-6 / - / -, F(4x4,3x3) - / 9.5e-6 / 1.6e-5; conv3 weight / bias 9.7e-7 / 5.4e-7 / 1.6e-6;
                        bias column sums 3.2e-9 / 1.9e-9 / 1.1e-9 of sum|.|
  elementwise           0 elements differ from the emulation (worst 6.0e-8 of the value: the final rounding); stem.dz exact
  bilinear x2           head.y2 and Q: 0 elements differ (6.0e-8); the transposes 1.6e-7 / 1.7e-7 / 1.6e-7
  BatchNorm             mean 2.7e-8, invstd 1.0e-7, scale 9.8e-8, shift 1.2e-7, running statistics 5.2e-8, eval coefficients 5.0e-8
  BatchNorm backward    sums 0.16 / 0.16 / 0.07 x 2^-24 sum|term| (bound 128), d gamma / d beta exactly (float) of the sums, input gradients 1.4e-7
  max-pool              3.2-3.7 % of the windows tied in the train modes (30 % with the running statistics of eval mode), idx the first slot in all
The whole file: 27 s wall, the B = 32 cases 4-6 s each, every other case about 1 s.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases
from oracle import fcn as ofcn
from oracle import learner as olearner
from simq import synth
from test_gpu_bf16_points import _fma32, _host_threads, _ulp_close32, relmax

pytestmark = pytest.mark.gpu

CIN, COUT = 5, 2
U24 = 2.0 ** -24
PLANES = {1: 64, 2: 128, 3: 256, 4: 512}
FWD_BAR = {'direct': 1e-5, 'f2': 1e-5, 'f4': 2e-5}
WGRAD_BAR = {'direct': 1e-5, 'f2': 1e-5, 'f4': 1e-4}
BN_BWD_BAR = 5e-6
# BatchNorm backward sums [sum dz | sum dz*xhat]: fp32 terms a producing kernel adds before its fp64 atomic (the worst-case bound of a
# sum of n fp32 terms is (n - 1) 2^-24 sum|term|; each term dz * ((y - mean) * invstd) carries three roundings of its own):
#   igemm_epilogue.h (direct / 1x1 / image-tile dgrads)   4*TM rows per lane, then two shuffle adds: BM / WM = 64 rows of a BM = 128 tile
#   wino_output_kernel (F(2x2,3x3) dgrads)                4 outputs per tile x ceil(ceil(T / tpb) / 512) trips <= 20 at B = 32
#   wino4f_output_kernel (F(4x4,3x3) dgrads)              16 outputs per tile x <= 2 trips = 32
#   chan_reduce_kernel<0> (head.red2, replicated form)    8 rows per lane
#   stem_pool_bwd_kernel                                  ceil(B*48*48*16 / (256 * min(1024, ceil(B*48*48*16 / 256)))): 1 / 2 / 5 at B = 5 / 8 / 32
# the largest is the implicit-GEMM epilogue's: 63 additions + 3 roundings per term <= 128 = the rows of its block tile
_N_FP32_TERMS = 128

nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)


@pytest.fixture(scope='module')
def simq_mod():
    import simq
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return simq


class _Threads:
    """fp64 reference convolutions on at most 16 host threads"""

    def __enter__(self):
        self.keep = torch.get_num_threads()
        torch.set_num_threads(min(16, _host_threads()))

    def __exit__(self, *a):
        torch.set_num_threads(self.keep)


# ---------------------------------------------------------------------------------------------------------------- which form runs where
def _block_convs():
    """(state-dict key, cin, cout, k) of the residual blocks' convolutions, forward order"""
    out = []
    for li in range(1, 5):
        for bi in range(2):
            p = PLANES[li]
            cin = p if (bi == 1 or li == 1) else PLANES[li - 1]
            key = 'resnet18.layer%d.%d.' % (li, bi)
            out.append((key + 'conv1.weight', cin, p, 3))
            out.append((key + 'conv2.weight', p, p, 3))
            if cin != p:
                out.append((key + 'downsample.0.weight', cin, p, 1))
    return out


def _wino(cin, cout, k):
    return k == 3 and cin * cout >= 128 * 128            # simq_plan_options.winograd_min_cc; every such layer is winograd_eligible


def _fwd_form(cin, cout, k, B, mode):
    """forward.hip conv_fwd: F(4x4,3x3) from 256 tiles -- in the grad-mode forward only the 512 -> 512 layers (winograd_f4_fwd_grad_min_cc)"""
    if not _wino(cin, cout, k):
        return 'direct'
    return 'f4' if (B * 36 >= 256 and (mode != 'train' or cin * cout >= 512 * 512)) else 'f2'


def _dgrad_form(cin, cout, k, B):
    """backward.hip conv_dgrad (winograd_f4_grad = 2)"""
    if not _wino(cin, cout, k):
        return 'direct'
    return 'f4' if B * 36 >= 256 else 'f2'


def _wgrad_form(cin, cout, k, B):
    """backward.hip conv_wgrad: winograd_wgrad_eligible (channels % 128) and winograd_wgrad_pays"""
    if not _wino(cin, cout, k) or cin % 128 or cout % 128:
        return 'direct'
    f4 = (B * 36) % 16 == 0
    if cin * cout >= (128 * 256 if f4 else 256 * 256):
        return 'f4' if f4 else 'f2'
    return 'direct'


def _count(form_of, want):
    return sum(1 for (_, cin, cout, k) in _block_convs() if form_of(cin, cout, k) == want)


def _fmt(ran):
    return ', '.join('%s x %d' % kv for kv in sorted(ran.items()))


# ---------------------------------------------------------------------------------------------------------------- one pass, snapshotted
class _Snap:
    pass


def _run(simq_mod, B, mode, options=None, backward=False, q_only=False, wseed=111, dseed=112):
    """ONE forward of an fp32 plan in `mode` ('train' | 'nograd' | 'eval') -- and, backward=True, one traced backward -- with every stored
    tensor copied to the host: S.t[name] (q_only: the Q-map and the launch log alone)."""
    from simq import _lib
    modes = {'train': _lib.MODE_TRAIN, 'nograd': _lib.MODE_TRAIN_NOGRAD, 'eval': _lib.MODE_EVAL}
    S = _Snap()
    S.B, S.mode, S.options = B, mode, dict(options or {})
    net = simq_mod.FCN(CIN, COUT, precision='fp32', options=options)
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(CIN, COUT, wseed)))
    S.plan_options = dict(net.plan.options)
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, CIN, dseed)]).permute(0, 2, 3, 1).contiguous().cuda()
    strip = lambda sd: {k[len('module.'):]: v.detach().cpu().clone() for k, v in sd.items()}
    S.sd0 = strip(net.state_dict())
    net._ensure_weights()
    _lib.lib.call('simq_launch_counts_reset')
    q = net._forward_raw(x, modes[mode])
    torch.cuda.synchronize()
    S.ran_fwd = _lib.launch_counts()
    slot = 'train' if mode == 'train' else 'tmp'
    t = S.t = {'x': x.cpu(), 'q': q.cpu()}
    if q_only:
        return S
    stored = lambda name: net.stored_tensor(name, B, slot).cpu()
    for name in ('stem.y0', 'stem.idx', 'head.z2', 'head.z3', 'head.bn1', 'head.bn2'):
        t[name] = stored(name)
    t['stem.pool'] = net.saved_activation('stem.pool', B, slot).cpu()
    if mode == 'eval':
        t['head.a1'] = net.saved_activation('head.a1', B, slot).cpu()
    else:
        for name in ('stem.bn', 'head.y1', 'head.y2'):
            t[name] = stored(name)
    if mode == 'train':
        t['head.a2'] = net.saved_activation('head.a2', B, 'train').cpu()
    for li in range(1, 5):
        for bi in range(2):
            b = 'layer%d.%d' % (li, bi)
            ds = li > 1 and bi == 0
            for w in (('a1', 'out') if mode == 'eval' else ('y1', 'y2', 'out')) + ('bn1', 'bn2') + (('yd', 'bnd') if ds else ()):
                t[b + '.' + w] = stored(b + '.' + w)
    S.sd1 = strip(net.state_dict())
    if backward:
        assert mode == 'train'
        dq = torch.from_numpy(cases.dense_upstream(COUT, B, dseed + 1)).cuda().contiguous()
        assert dq.shape == q.shape
        t['dq'] = dq.cpu()
        _lib.lib.call('simq_launch_counts_reset')
        grads_flat, traced = net.backward_traced(dq, B)
        torch.cuda.synchronize()
        S.ran_bwd = _lib.launch_counts()
        S.param_names = [k for (k, _, _) in net._param_names]
        S.grads = {k: v.detach().cpu().clone() for (k, _, _), v in zip(net._param_names, net.reference_views(grads_flat))}
        flat1 = grads_flat.clone()
        for li in range(1, 5):
            for bi in range(2):
                b = 'layer%d.%d' % (li, bi)
                ds = li > 1 and bi == 0
                for w in ('g_out', 'dy2', 'da1', 'dy1', 'g_in') + (('dyd', 'g_ds') if ds else ('dz',)):
                    t['tr.' + b + '.' + w] = traced(b + '.' + w).cpu()
                for w in ('red1', 'red2') + (('redd',) if ds else ()):
                    t[b + '.' + w] = stored(b + '.' + w)
        for name in ('head.da2', 'head.dy2', 'head.dz2', 'head.da1', 'head.dy1', 'stem.dz', 'stem.dy0'):
            t['tr.' + name] = traced(name).cpu()
        for name in ('stem.red', 'head.red1', 'head.red2'):
            t[name] = stored(name)
        if S.plan_options['deterministic']:
            grads2, _ = net.backward_traced(dq, B)
            torch.cuda.synchronize()
            S.repeat_equal = bool(torch.equal(flat1, grads2))
    return S


@pytest.fixture(scope='module')
def walk_b8(simq_mod):
    """the default plan's grad-mode forward + traced backward at B = 8, shared by stage A (train, b8), stage B (default, b8) and stage C"""
    return _run(simq_mod, 8, 'train', None, backward=True)


# ---------------------------------------------------------------------------------------------------------------- metrics
class _Log:
    def __init__(self, tag):
        self.tag, self.lines, self.worst = tag, [], {}

    def note(self, cls, value, line=None):
        self.worst[cls] = max(self.worst.get(cls, 0.0), float(value))
        if line:
            self.lines.append('  ' + line)

    def dump(self):
        print('\n%s\n%s' % (self.tag, '\n'.join(self.lines)))
        print('  WORST per class [%s]: %s' % (self.tag, ', '.join('%s %.3g' % kv for kv in sorted(self.worst.items()))))


def _ulp_worst(got, want64):
    """the two figures _ulp_close32 asserts (fraction of elements that differ, worst error of the value) without asserting"""
    want = want64.float()
    frac = float((got != want).double().mean())
    worst = float(((got.double() - want64).abs() / want64.abs().clamp_min(1e-3 * float(want64.abs().max()))).max())
    return frac, worst


def _ulp(log, name, got, want64, cls='elementwise'):
    frac, worst = _ulp_worst(got, want64)
    log.note(cls + ' frac', frac)
    log.note(cls + ' worst', worst, '%-26s %.5f %% of the fp32 elements differ from the emulation, worst %.2e of the value' % (name, 100 * frac, worst))
    _ulp_close32(name, got, want64)


def _close(log, name, got, want64, bar, cls, scale=None):
    e = float((got.double() - want64).abs().max() / (want64.abs().max().clamp_min(1e-300) if scale is None else scale))
    log.note(cls, e, '%-38s %.2e (bar %.0e)' % (name, e, bar))
    assert e < bar, (name, e, bar)


def _bn_stats64(y):
    """fp64 batch statistics of a stored NHWC pre-BatchNorm tensor"""
    y64 = y.double().reshape(-1, y.shape[-1])
    mean = y64.mean(0)
    var = ((y64 - mean) ** 2).mean(0)
    return mean, var, y64.shape[0]


def _check_bn_train(log, S, name, aux, y, bnkey):
    """train modes: the coefficients the consuming kernel formed (scale | shift | mean | invstd) against the STORED pre-BN tensor, and the
    running-statistics update of the layer (momentum 0.1, unbiased variance)"""
    sd0, sd1 = S.sd0, S.sd1
    mean, var, rows = _bn_stats64(y)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    rng = float(y.abs().max())
    e_mean, e_inv = float((aux[2].double() - mean).abs().max()) / rng, relmax(aux[3], invstd)
    gamma, beta = sd0[bnkey + '.weight'].double(), sd0[bnkey + '.bias'].double()
    sc = gamma * aux[3].double()
    e_sc = relmax(aux[0], sc)
    msc = aux[2].double() * sc
    e_sh = float((aux[1].double() - (beta - msc)).abs().max() / max(float(beta.abs().max()), float(msc.abs().max())))
    e_rm = relmax(sd1[bnkey + '.running_mean'], 0.9 * sd0[bnkey + '.running_mean'].double() + 0.1 * mean)
    e_rv = relmax(sd1[bnkey + '.running_var'], 0.9 * sd0[bnkey + '.running_var'].double() + 0.1 * var * rows / (rows - 1))
    log.note('bn mean', e_mean); log.note('bn invstd', e_inv); log.note('bn scale', e_sc); log.note('bn shift', e_sh)
    log.note('bn running', max(e_rm, e_rv), '%-26s mean %.1e invstd %.1e scale %.1e shift %.1e running %.1e / %.1e' % (name, e_mean, e_inv, e_sc, e_sh, e_rm, e_rv))
    assert e_mean < 2e-5 and e_inv < 2e-5, (name, e_mean, e_inv)
    assert e_sc < 1e-6 and e_sh < 1e-6, (name, e_sc, e_sh)
    assert e_rm < 1e-6 and e_rv < 1e-6, (name, e_rm, e_rv)


def _eval_coeff64(sd, bnkey):
    invstd = 1.0 / torch.sqrt(sd[bnkey + '.running_var'].double() + 1e-5)
    sc = sd[bnkey + '.weight'].double() * invstd
    return sc, sd[bnkey + '.bias'].double() - sd[bnkey + '.running_mean'].double() * sc


def _check_bn_eval(log, S, name, aux, bnkey):
    """eval mode: bn_eval_coeff_kernel's scale | shift from the running statistics; and they must not have moved"""
    sc, sh = _eval_coeff64(S.sd0, bnkey)
    e_sc, e_sh = relmax(aux[0], sc), relmax(aux[1], sh)
    log.note('bn eval coeff', max(e_sc, e_sh), '%-26s scale %.1e shift %.1e' % (name, e_sc, e_sh))
    assert e_sc < 1e-6 and e_sh < 1e-6, (name, e_sc, e_sh)
    assert torch.equal(S.sd0[bnkey + '.running_mean'], S.sd1[bnkey + '.running_mean']) and torch.equal(S.sd0[bnkey + '.running_var'], S.sd1[bnkey + '.running_var'])


# ---------------------------------------------------------------------------------------------------------------- bilinear x2, as the kernels form it
def _lerp_tab(n_in, fused):
    """head.hip lerp2x / elementwise.hip lerp_coord for every output index of a 2x map: (i0, i1, l0, l1) with fp32 weights.
    fused: real - i0 was contracted with real = scale * o into one fma (head_upsample_q_kernel, upsample2x_bwd_kernel: l1 = rn(scale*o - i0));
    otherwise l1 = rn(rn(scale*o) - i0) (upsample2x_fwd_kernel)."""
    n_out = 2 * n_in
    scale = np.float32(n_in - 1) / np.float32(n_out - 1)
    o = np.arange(n_out, dtype=np.float32)
    real = (scale * o).astype(np.float32)
    i0 = np.minimum(real.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    if fused:
        l1 = (np.float64(scale) * o.astype(np.float64) - i0.astype(np.float64)).astype(np.float32)
    else:
        l1 = real - i0.astype(np.float32)
    l1 = np.clip(l1, np.float32(0), np.float32(1)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l0), torch.from_numpy(l1)


def _up2x_emul(z, fused, fused_y=None):
    """[B, n, n, C] fp32 -> the fp64 value in front of the last rounding of  ly0*(lx0*v00 + lx1*v01) + ly1*(lx0*v10 + lx1*v11)  as compiled:
    t(row) = fma(lx0, v0, rn(lx1*v1)) per source row, v = fma(ly0, t(y0), rn(ly1*t(y1))).  fused / fused_y: how l1 was formed along x / y"""
    x0, x1, lx0, lx1 = _lerp_tab(z.shape[2], fused)
    y0, y1, ly0, ly1 = _lerp_tab(z.shape[1], fused if fused_y is None else fused_y)
    zd = z.double()
    lx0, lx1 = lx0.double().view(1, 1, -1, 1), lx1.double().view(1, 1, -1, 1)
    t = (lx0 * zd[:, :, x0, :] + (lx1 * zd[:, :, x1, :]).float().double()).float().double()
    ly0, ly1 = ly0.double().view(1, -1, 1, 1), ly1.double().view(1, -1, 1, 1)
    return ly0 * t[:, y0] + (ly1 * t[:, y1]).float().double()


def _nearest_candidate(got, cands):
    """per element, the candidate closest to `got` (fp64 values in front of the last rounding)"""
    best = cands[0].clone()
    for c in cands[1:]:
        closer = (got.double() - c).abs() < (got.double() - best).abs()
        best = torch.where(closer, c, best)
    return best


def _lerp_matrix(n_in, fused):
    """[2n, n] fp64: row o holds l0 at i0 and l1 at i1 (ADDED where the two taps coincide: the last row)"""
    i0, i1, l0, l1 = _lerp_tab(n_in, fused)
    W = torch.zeros(2 * n_in, n_in, dtype=torch.float64)
    r = torch.arange(2 * n_in)
    W.index_put_((r, i0), l0.double(), accumulate=True)
    W.index_put_((r, i1), l1.double(), accumulate=True)
    return W


def _up2x_transpose64(d, fused):
    """[B, 2n, 2n, C] -> [B, n, n, C]: the transpose of the bilinear map with the kernel's fp32 weights, in fp64"""
    W = _lerp_matrix(d.shape[1] // 2, fused)
    return torch.einsum('pj,bipc->bijc', W, torch.einsum('oi,bopc->bipc', W, d.double()))


# ---------------------------------------------------------------------------------------------------------------- stage A: forward
def _pool_windows(a0):
    """NHWC [B,48,48,C] -> (max [B,C,24,24], first maximal slot, last maximal slot, tied) over the 3x3 / stride-2 / pad-1 windows, slot = dy*3+dx"""
    p = F.pad(nchw(a0), (1, 1, 1, 1), value=float('-inf'))
    win = p.unfold(2, 3, 2).unfold(3, 3, 2).reshape(a0.shape[0], a0.shape[3], 24, 24, 9)
    mx = win.max(-1).values
    eq = win == mx.unsqueeze(-1)
    slots = torch.arange(9).view(1, 1, 1, 1, 9)
    first = torch.where(eq, slots, torch.full_like(slots, 9)).min(-1).values
    last = torch.where(eq, slots, torch.full_like(slots, -1)).max(-1).values
    return mx, first, last, eq.sum(-1) > 1


def _stem_coeff(S):
    """scale | shift of the stem's BatchNorm as stem_pool_fwd_kernel forms them: stored in the train modes, from the running statistics
    (bn_coeff: fp64, rounded once) in eval mode, where nothing stores them"""
    if S.mode != 'eval':
        return S.t['stem.bn'][0], S.t['stem.bn'][1]
    sc, sh = _eval_coeff64(S.sd0, 'resnet18.bn1')
    return sc.float(), sh.float()


def _check_stem_forward(S, log):
    t, sd = S.t, S.sd0
    B = S.B
    y0 = t['stem.y0']
    assert y0.dtype == torch.float32 and tuple(y0.shape) == (B, 48, 48, 64)
    y0ref = F.conv2d(nchw(t['x'].double()), sd['resnet18.conv1.weight'].double(), stride=2, padding=3)
    _close(log, 'stem.y0 (7x7 / stride 2)', nchw(y0), y0ref, 1e-5, 'conv direct')
    if S.mode != 'eval':
        _check_bn_train(log, S, 'stem.bn', t['stem.bn'], y0, 'resnet18.bn1')
    sc, sh = _stem_coeff(S)
    a0 = torch.relu(_fma32(y0, sc, sh))
    mx, first, last, tied = _pool_windows(a0)
    _ulp(log, 'stem.pool', nchw(t['stem.pool']), mx.double())
    slot = nchw(t['stem.idx']).long()
    frac_tied = float(tied.double().mean())
    wrong_unique, wrong_tied = int(((slot != first) & ~tied).sum()), int(((slot != first) & tied).sum())
    log.note('pool tied windows', frac_tied, '%-26s %.1f %% of the windows tied; idx != first maximal slot in %d unique / %d tied windows' % ('stem.idx', 100 * frac_tied, wrong_unique, wrong_tied))
    assert frac_tied >= 0.01, 'the tie rule of the max-pool is not exercised: %.3g of the windows tied' % frac_tied
    assert wrong_unique == 0, 'stem.idx is not the maximal slot of %d windows' % wrong_unique
    assert wrong_tied == 0, 'stem.idx is not the FIRST tied slot in %d windows' % wrong_tied


def _block_iter():
    for li in range(1, 5):
        for bi in range(2):
            yield li, bi, 'layer%d.%d' % (li, bi), 'resnet18.layer%d.%d.' % (li, bi), (li > 1 and bi == 0)


def _check_blocks_forward(S, log):
    t, sd, B, mode = S.t, S.sd0, S.B, S.mode
    cur = t['stem.pool']
    for li, bi, b, key, ds in _block_iter():
        p = PLANES[li]
        cin = cur.shape[-1]
        f1, f2 = _fwd_form(cin, p, 3, B, mode), _fwd_form(p, p, 3, B, mode)
        xin = nchw(cur.double())
        c1 = F.conv2d(xin, sd[key + 'conv1.weight'].double(), padding=1)
        if mode == 'eval':
            # conv -> folded BatchNorm (running statistics) -> [+ identity] -> ReLU in the convolution's epilogue
            bn1, bn2 = t[b + '.bn1'], t[b + '.bn2']
            _check_bn_eval(log, S, b + '.bn1', bn1, key + 'bn1')
            _check_bn_eval(log, S, b + '.bn2', bn2, key + 'bn2')
            v = lambda c, aux: c * aux[0].double().view(1, -1, 1, 1) + aux[1].double().view(1, -1, 1, 1)
            a1 = t[b + '.a1']
            _close(log, b + '.a1 (%s)' % f1, nchw(a1), torch.relu(v(c1, bn1)), FWD_BAR[f1], 'conv ' + f1)
            if ds:
                bnd, yd = t[b + '.bnd'], t[b + '.yd']
                _check_bn_eval(log, S, b + '.bnd', bnd, key + 'downsample.1')
                _close(log, b + '.yd (1x1)', nchw(yd), v(F.conv2d(xin, sd[key + 'downsample.0.weight'].double()), bnd), 1e-5, 'conv direct')
                identity = nchw(yd.double())
            else:
                identity = xin
            c2 = F.conv2d(nchw(a1.double()), sd[key + 'conv2.weight'].double(), padding=1)
            _close(log, b + '.out (%s)' % f2, nchw(t[b + '.out']), torch.relu(v(c2, bn2) + identity), FWD_BAR[f2], 'conv ' + f2)
            cur = t[b + '.out']
            continue
        y1, y2, bn1, bn2 = t[b + '.y1'], t[b + '.y2'], t[b + '.bn1'], t[b + '.bn2']
        _close(log, b + '.y1 (%s)' % f1, nchw(y1), c1, FWD_BAR[f1], 'conv ' + f1)
        _check_bn_train(log, S, b + '.bn1', bn1, y1, key + 'bn1')
        # the activation between the two convolutions is never stored (fuse_bn1_apply): rebuilt from the stored coefficients as conv2 does
        act1 = torch.relu(_fma32(y1, bn1[0], bn1[1]))
        _close(log, b + '.y2 (%s)' % f2, nchw(y2), F.conv2d(nchw(act1.double()), sd[key + 'conv2.weight'].double(), padding=1), FWD_BAR[f2], 'conv ' + f2)
        _check_bn_train(log, S, b + '.bn2', bn2, y2, key + 'bn2')
        if ds:
            yd, bnd = t[b + '.yd'], t[b + '.bnd']
            _close(log, b + '.yd (1x1)', nchw(yd), F.conv2d(xin, sd[key + 'downsample.0.weight'].double()), 1e-5, 'conv direct')
            _check_bn_train(log, S, b + '.bnd', bnd, yd, key + 'downsample.1')
            identity = _fma32(yd, bnd[0], bnd[1])
        else:
            identity = cur
        _ulp(log, b + '.out', t[b + '.out'], torch.relu(_fma32(y2, bn2[0], bn2[1]).double() + identity.double()))
        cur = t[b + '.out']


def _check_head_forward(S, log):
    t, sd, B, mode = S.t, S.sd0, S.B, S.mode
    out7 = nchw(t['layer4.1.out'].double())
    c1 = F.conv2d(out7, sd['conv1.weight'].double(), sd['conv1.bias'].double())
    bcast = lambda v: v.double().view(1, -1, 1, 1)
    if mode == 'eval':
        bn1, bn2 = t['head.bn1'], t['head.bn2']
        _check_bn_eval(log, S, 'head.bn1', bn1, 'bn1')
        _check_bn_eval(log, S, 'head.bn2', bn2, 'bn2')
        a1 = t['head.a1']
        _close(log, 'head.a1 (1x1 + folded bn1)', nchw(a1), torch.relu(c1 * bcast(bn1[0]) + bcast(bn1[1])), 1e-5, 'conv direct')
        z2 = t['head.z2']
        c2 = F.conv2d(nchw(a1.double()), sd['conv2.weight'].double(), sd['conv2.bias'].double())
        _close(log, 'head.z2 (1x1 + folded bn2)', nchw(z2), c2 * bcast(bn2[0]) + bcast(bn2[1]), 1e-5, 'conv direct')
        # head_up_relu_conv3_kernel: bilinear x2 -> ReLU -> conv3 in one pass, nothing stored in between
        a2 = torch.relu(_up2x_emul(z2, fused=False).float())
    else:
        y1 = t['head.y1']
        _close(log, 'head.y1 (1x1)', nchw(y1), c1, 1e-5, 'conv direct')
        _check_bn_train(log, S, 'head.bn1', t['head.bn1'], y1, 'bn1')
        act1 = torch.relu(_fma32(y1, t['head.bn1'][0], t['head.bn1'][1]))
        z2 = t['head.z2']
        _close(log, 'head.z2 (1x1 + bias)', nchw(z2), F.conv2d(nchw(act1.double()), sd['conv2.weight'].double(), sd['conv2.bias'].double()), 1e-5, 'conv direct')
        y2 = t['head.y2']
        assert tuple(y2.shape) == (B, 48, 48, 32)
        _ulp(log, 'head.y2 (bilinear x2)', y2, _up2x_emul(z2, fused=False), 'bilinear')
        _check_bn_train(log, S, 'head.bn2', t['head.bn2'], y2, 'bn2')
        a2ref = torch.relu(y2.double() * t['head.bn2'][0].double() + t['head.bn2'][1].double())
        if mode == 'train':
            a2 = t['head.a2']
            _ulp(log, 'head.a2', a2, a2ref)
        else:
            a2 = a2ref.float()                                       # (the no-grad forward never stores it)
    z3 = t['head.z3'].reshape(B, COUT, 48, 48)                       # (stored channel-major, like the Q-map it becomes)
    _close(log, 'head.z3 (conv3, no bias)', z3, F.conv2d(nchw(a2.double()), sd['conv3.weight'].double()), 1e-5, 'conv direct')
    # head_upsample_q_kernel forms l1 = scale*o - i0 once per output row and four times per thread along x: the compiler contracts some of
    # them with real = scale*o into one fma (one rounding) and leaves the others as written (two), column by column as its scheduling falls
    # out -- the two weights differ by up to an ulp of `real` (2e-6), 5 x this check's resolution.  Either is lerp2x; an element must be the
    # emulation under one of the two forms per axis (a wrong tap or weight is 1e3 ulp away from all four: stage C)
    cands = [nchw(_up2x_emul(nhwc(z3), fx, fy)).float().double() + bcast(sd['conv3.bias']) for fx in (True, False) for fy in (True, False)]
    _ulp(log, 'Q (bilinear x2 + bias)', t['q'], _nearest_candidate(t['q'], cands), 'bilinear')


def _assert_forward_launches(S):
    B, mode, ran = S.B, S.mode, S.ran_fwd
    print('\n  B = %d %s forward launch log: %s' % (B, mode, _fmt(ran)))
    form = lambda cin, cout, k: _fwd_form(cin, cout, k, B, mode)
    assert ran.get('winograd_f4', 0) == _count(form, 'f4') and ran.get('winograd_f2', 0) == _count(form, 'f2'), (ran, _count(form, 'f4'), _count(form, 'f2'))
    assert ran.get('stem_conv_f32', 0) == 1, ran
    if B == 5:
        assert ran.get('winograd_f4', 0) == 0 and ran.get('winograd_f2', 0) == 11, ran
    else:
        assert ran.get('winograd_f4', 0) > 0 and ran.get('conv_img_f32', 0) > 0, ran
        if mode == 'train':
            assert ran.get('winograd_f2', 0) > 0, ran
    if S.plan_options['gemm_split'] == 1:
        assert ran.get('gemm_split3_batched', 0) > 0 and ran.get('gemm_f32_batched', 0) == 0, ran


def _check_forward(S, tag):
    log = _Log(tag)
    try:
        with _Threads():
            _check_stem_forward(S, log)
            _check_blocks_forward(S, log)
            _check_head_forward(S, log)
    finally:
        log.dump()


_FWD_CASES = [(m, B) for m in ('train', 'nograd', 'eval') for B in (5, 8)] + [('train', 32), ('nograd', 32)]


@pytest.mark.parametrize('mode,B', _FWD_CASES, ids=['%s_b%d' % c for c in _FWD_CASES])
def test_fp32_forward_teacher_forced(simq_mod, request, mode, B):
    """Stage A: every tensor a forward of the fp32 plan stores, in the three modes of simq_forward, against fp64 on the stored tensors it was
    made from (bars: the header).  MODE_EVAL runs on a plan with fuse_bn1_apply = 0 -- the folded eval path does not read the option, it
    only lets the accessor return a1, which eval-mode forwards do store -- and its Q-map must equal the default plan's bit for bit."""
    if mode == 'eval':
        S = _run(simq_mod, B, 'eval', {'fuse_bn1_apply': 0})
        assert S.plan_options['fuse_bn1_apply'] == 0
        D = _run(simq_mod, B, 'eval', None, q_only=True)
        assert D.plan_options['fuse_bn1_apply'] == 1
        assert torch.equal(S.t['q'], D.t['q']), 'the eval-mode Q-map depends on fuse_bn1_apply'
        assert D.ran_fwd == S.ran_fwd, (D.ran_fwd, S.ran_fwd)
    elif (mode, B) == ('train', 8):
        S = request.getfixturevalue('walk_b8')
    else:
        S = _run(simq_mod, B, mode, None)
    _assert_forward_launches(S)
    _check_forward(S, 'fp32 forward, %s, B = %d' % (mode, B))


# ---------------------------------------------------------------------------------------------------------------- stage B: backward
def _sum_multiple(red, dz64, xhat64):
    """the stored [sum dz | sum dz*xhat] against the fp64 sums of the same fp32 terms, per channel, in units of 2^-24 sum|term|"""
    C = dz64.shape[-1]
    t0, t1 = dz64.reshape(-1, C), (dz64 * xhat64).reshape(-1, C)
    m0 = ((red[0] - t0.sum(0)).abs() / (U24 * t0.abs().sum(0)).clamp_min(1e-300)).max()
    m1 = ((red[1] - t1.sum(0)).abs() / (U24 * t1.abs().sum(0)).clamp_min(1e-300)).max()
    return max(float(m0), float(m1))


def _check_bn_backward(S, log, name, red, dz64, y, aux, gamma, gkey, bkey, dy_traced):
    """sums, d gamma / d beta, and the BatchNorm input gradient gamma * invstd * (dz - sum dz / M - xhat * sum(dz*xhat) / M) with the STORED sums"""
    xhat = (y.double() - aux[2].double()) * aux[3].double()
    m = _sum_multiple(red, dz64, xhat)
    log.note('bn sums (x 2^-24 sum|term|)', m, '%-26s sums: %.2f x 2^-24 sum|term| (bound %d)' % (name, m, _N_FP32_TERMS))
    assert m <= _N_FP32_TERMS, (name, m)
    _close(log, name + ' d beta', S.grads[bkey], red[0].float().double(), 1e-6, 'bn dparam')
    _close(log, name + ' d gamma', S.grads[gkey], red[1].float().double(), 1e-6, 'bn dparam')
    S.checked.update((gkey, bkey))
    M = float(dz64.numel() // dz64.shape[-1])
    _close(log, name + ' input gradient', dy_traced, gamma.double() * aux[3].double() * (dz64 - red[0] / M - xhat * red[1] / M), BN_BWD_BAR, 'bn input gradient')
    return xhat


def _wgrad(S, log, key, x, dy, form, stride=1, pad=1):
    want = torch.nn.grad.conv2d_weight(nchw(x.double()), tuple(S.sd0[key].shape), nchw(dy.double()), stride=stride, padding=pad)
    _close(log, key + ' (%s)' % form, S.grads[key], want, WGRAD_BAR[form], 'wgrad ' + form)
    S.checked.add(key)


def _check_head_backward(S, log):
    t, sd, B = S.t, S.sd0, S.B
    dq = t['dq'].double()
    a2 = t['head.a2']
    w3 = sd['conv3.weight'].double().reshape(COUT, 32)
    # conv3 at 96x96 on the bilinear x2 of the stored a2 (upsample2x_fwd_kernel), then the bilinear transpose (upsample2x_bwd_kernel)
    W = _lerp_matrix(48, False)
    up = torch.einsum('qj,bojc->boqc', W, torch.einsum('oi,bijc->bojc', W, a2.double()))
    _close(log, 'conv3.weight', S.grads['conv3.weight'].reshape(COUT, 32), torch.einsum('bkyx,byxc->kc', dq, up), 1e-5, 'head conv3 gradients')
    _close(log, 'conv3.bias', S.grads['conv3.bias'], dq.sum(dim=(0, 2, 3)), 1e-5, 'head conv3 gradients')
    S.checked.update(('conv3.weight', 'conv3.bias'))
    da2 = t['tr.head.da2']
    _close(log, 'head.da2', da2, _up2x_transpose64(torch.einsum('bkyx,kc->byxc', dq, w3), True), 5e-6, 'bilinear transpose')
    y2, bn2 = t['head.y2'], t['head.bn2']
    dz = da2.double() * (a2 > 0).double()
    dy2 = t['tr.head.dy2']
    _check_bn_backward(S, log, 'head.bn2', t['head.red2'], dz, y2, bn2, sd['bn2.weight'], 'bn2.weight', 'bn2.bias', dy2)
    dz2 = t['tr.head.dz2']
    _close(log, 'head.dz2', dz2, _up2x_transpose64(dy2, True), 5e-6, 'bilinear transpose')
    # (the biases in front of a BatchNorm have a gradient that is zero in exact arithmetic: measured against the magnitudes that were added)
    _close(log, 'conv2.bias', S.grads['conv2.bias'], dz2.double().sum(dim=(0, 1, 2)), 1e-5, 'bias column sums', scale=float(dz2.double().abs().sum(dim=(0, 1, 2)).max()))
    y1, bn1 = t['head.y1'], t['head.bn1']
    pre1 = _fma32(y1, bn1[0], bn1[1])
    act1 = torch.relu(pre1)
    _close(log, 'conv2.weight', S.grads['conv2.weight'].reshape(32, 128), dz2.double().reshape(-1, 32).t() @ act1.double().reshape(-1, 128), 1e-5, 'wgrad direct')
    da1 = t['tr.head.da1']
    _close(log, 'head.da1', da1.reshape(-1, 128), dz2.double().reshape(-1, 32) @ sd['conv2.weight'].double().reshape(32, 128), 1e-5, 'dgrad direct')
    dy1 = t['tr.head.dy1']
    _check_bn_backward(S, log, 'head.bn1', t['head.red1'], da1.double() * (pre1 > 0).double(), y1, bn1, sd['bn1.weight'], 'bn1.weight', 'bn1.bias', dy1)
    _close(log, 'conv1.bias', S.grads['conv1.bias'], dy1.double().sum(dim=(0, 1, 2)), 1e-5, 'bias column sums', scale=float(dy1.double().abs().sum(dim=(0, 1, 2)).max()))
    out7 = t['layer4.1.out']
    _close(log, 'conv1.weight', S.grads['conv1.weight'].reshape(128, 512), dy1.double().reshape(-1, 128).t() @ out7.double().reshape(-1, 512), 1e-5, 'wgrad direct')
    S.checked.update(('conv2.bias', 'conv2.weight', 'conv1.bias', 'conv1.weight'))
    _close(log, 'layer4.1.g_out', t['tr.layer4.1.g_out'].reshape(-1, 512), dy1.double().reshape(-1, 128) @ sd['conv1.weight'].double().reshape(128, 512), 1e-5, 'dgrad direct')


def _check_blocks_backward(S, log):
    t, sd, B = S.t, S.sd0, S.B
    prev_g_in = None
    for li, bi, b, key, ds in reversed(list(_block_iter())):
        p = PLANES[li]
        xin = t['layer%d.%d.out' % ((li, 0) if bi == 1 else (li - 1, 1))] if (li, bi) != (1, 0) else t['stem.pool']
        cin = xin.shape[-1]
        y1, y2, out, bn1, bn2 = t[b + '.y1'], t[b + '.y2'], t[b + '.out'], t[b + '.bn1'], t[b + '.bn2']
        tr = lambda w: t['tr.' + b + '.' + w]
        g_out = tr('g_out')
        if prev_g_in is not None:
            assert torch.equal(g_out, prev_g_in), b + ': the gradient the block receives is not the one the block above produced'
        # out = relu(bn2(y2) + identity): dz = g_out * [out > 0] feeds bn2, the downsample BatchNorm or the identity shortcut
        dz64 = g_out.double() * (out > 0).double()
        dy2 = tr('dy2')
        _check_bn_backward(S, log, b + '.bn2', t[b + '.red2'], dz64, y2, bn2, sd[key + 'bn2.weight'], key + 'bn2.weight', key + 'bn2.bias', dy2)
        if ds:
            dyd = tr('dyd')
            _check_bn_backward(S, log, b + '.bnd', t[b + '.redd'], dz64, t[b + '.yd'], t[b + '.bnd'], sd[key + 'downsample.1.weight'],
                               key + 'downsample.1.weight', key + 'downsample.1.bias', dyd)
        else:
            assert torch.equal(tr('dz'), dz64.float()), b + '.dz: the masked gradient of the identity shortcut is not exact'
        # a1 = relu(bn1(y1)) was never stored: conv2's weight gradient and bn1's mask rebuild it from y1 with the forward's own scale / shift
        pre1 = _fma32(y1, bn1[0], bn1[1])
        _wgrad(S, log, key + 'conv2.weight', torch.relu(pre1), dy2, _wgrad_form(p, p, 3, B))
        da1 = tr('da1')
        f = _dgrad_form(p, p, 3, B)
        _close(log, b + '.da1 (%s)' % f, nchw(da1), F.conv_transpose2d(nchw(dy2.double()), sd[key + 'conv2.weight'].double(), padding=1), FWD_BAR[f], 'dgrad ' + f)
        dy1 = tr('dy1')
        _check_bn_backward(S, log, b + '.bn1', t[b + '.red1'], da1.double() * (pre1 > 0).double(), y1, bn1, sd[key + 'bn1.weight'], key + 'bn1.weight', key + 'bn1.bias', dy1)
        _wgrad(S, log, key + 'conv1.weight', xin, dy1, _wgrad_form(cin, p, 3, B))
        gin = F.conv_transpose2d(nchw(dy1.double()), sd[key + 'conv1.weight'].double(), padding=1)
        if ds:
            _wgrad(S, log, key + 'downsample.0.weight', xin, dyd, 'direct', pad=0)
            g_ds = tr('g_ds')
            _close(log, b + '.g_ds (1x1)', nchw(g_ds), F.conv_transpose2d(nchw(dyd.double()), sd[key + 'downsample.0.weight'].double()), 1e-5, 'dgrad direct')
            gin = gin + nchw(g_ds.double())
        else:
            gin = gin + nchw(tr('dz').double())
        prev_g_in = tr('g_in')
        f = _dgrad_form(cin, p, 3, B)
        _close(log, b + '.g_in (%s + addend)' % f, nchw(prev_g_in), gin, FWD_BAR[f], 'dgrad ' + f)


def _pool_backward_emul(g, pooled, idx):
    """stem_pool_bwd_kernel's gather in its own fp32 order: a pixel of the 48x48 map adds, window row 2 / 1 before row 0 and column 2 / 1
    before column 0, the gradient of every window whose first maximal slot it is and whose pooled value is positive (the ReLU)"""
    B, _, _, C = g.shape
    acc = torch.zeros(B, 48, 48, C, dtype=torch.float32)
    live = pooled > 0
    zero = torch.zeros((), dtype=torch.float32)
    rows = {0: (slice(1, 46, 2), slice(1, 24)), 1: (slice(0, 47, 2), slice(0, 24)), 2: (slice(1, 48, 2), slice(0, 24))}     # 2*p - 1 + d
    for dy in (1, 2, 0):
        for dx in (1, 2, 0):
            c = torch.where((idx == dy * 3 + dx) & live, g, zero)
            (ty, sy), (tx, sx) = rows[dy], rows[dx]
            acc[:, ty, tx] = acc[:, ty, tx] + c[:, sy, sx]
    return acc


def _check_stem_backward(S, log):
    t, sd, B = S.t, S.sd0, S.B
    dz = t['tr.stem.dz']
    _ulp(log, 'stem.dz (max-pool + ReLU)', dz, _pool_backward_emul(t['tr.layer1.0.g_in'], t['stem.pool'], t['stem.idx']).double())
    dy0 = t['tr.stem.dy0']
    _check_bn_backward(S, log, 'stem.bn', t['stem.red'], dz.double(), t['stem.y0'], t['stem.bn'], sd['resnet18.bn1.weight'], 'resnet18.bn1.weight', 'resnet18.bn1.bias', dy0)
    _wgrad(S, log, 'resnet18.conv1.weight', t['x'], dy0, 'direct', stride=2, pad=3)


def _assert_backward_launches(S):
    B = S.B
    ran = dict(S.ran_bwd)
    print('\n  B = %d backward launch log: %s' % (B, _fmt(ran)))
    dg = lambda cin, cout, k: _dgrad_form(cin, cout, k, B)
    wg = lambda cin, cout, k: _wgrad_form(cin, cout, k, B)
    n4, n2 = _count(dg, 'f4'), _count(dg, 'f2')                       # (every block convolution has a data gradient, layer1.0.conv1's feeds the stem)
    assert ran.get('winograd_f4', 0) == n4 and ran.get('winograd_f2', 0) == n2, (ran, n4, n2)
    assert ran.get('winograd_f4_wgrad', 0) == _count(wg, 'f4') and ran.get('winograd_f2_wgrad', 0) == _count(wg, 'f2'), (ran, _count(wg, 'f4'), _count(wg, 'f2'))
    both = {k: S.ran_fwd.get(k, 0) + ran.get(k, 0) for k in set(S.ran_fwd) | set(ran)}
    if B == 5:
        assert both.get('winograd_f4', 0) == 0 and both.get('winograd_f2_wgrad', 0) > 0 and both.get('winograd_f4_wgrad', 0) == 0, both
    else:
        missing = [f for f in ('winograd_f4', 'winograd_f2', 'winograd_f4_wgrad', 'conv_img_f32', 'stem_conv_f32') if both.get(f, 0) == 0]
        assert not missing, 'B = %d did not select %s (ran: %s)' % (B, missing, both)
    assert both.get('gemm_split3_batched', 0) > 0 and both.get('gemm_f32_batched', 0) == 0, both


def _check_backward(S, tag):
    log = _Log(tag)
    S.checked = set()
    try:
        with _Threads():
            _check_head_backward(S, log)
            _check_blocks_backward(S, log)
            _check_stem_backward(S, log)
    finally:
        log.dump()
    assert S.checked == set(S.param_names), 'gradients left unchecked: %s' % sorted(set(S.param_names) ^ S.checked)


_BWD_CASES = [('default', 5), ('default', 8), ('deterministic', 5), ('deterministic', 8), ('deterministic', 32)]


@pytest.mark.parametrize('plan,B', _BWD_CASES, ids=['%s_b%d' % c for c in _BWD_CASES])
def test_fp32_backward_teacher_forced(simq_mod, request, plan, B):
    """Stage B: one grad-mode forward + simq_backward_traced with the dense upstream gradient: every traced gradient tensor, every BatchNorm
    sum and EVERY parameter gradient (the checked keys must be the full set of net._param_names) against fp64 on the stored operands.
    Deterministic plans (what the headline B = 32 runs) must also repeat the gradient bit for bit on a second traced backward."""
    if (plan, B) == ('default', 8):
        S = request.getfixturevalue('walk_b8')
    else:
        S = _run(simq_mod, B, 'train', {'deterministic': 1} if plan == 'deterministic' else None, backward=True)
    assert S.plan_options['deterministic'] == (1 if plan == 'deterministic' else 0)
    assert S.plan_options['fuse_bn1_apply'] == 1 and S.plan_options['fuse_bn_backward_sums'] == 1
    _assert_backward_launches(S)
    _check_backward(S, 'fp32 backward, %s plan, B = %d' % (plan, B))
    if plan == 'deterministic':
        assert S.repeat_equal, 'deterministic plan: a second traced backward gave another gradient'


# ---------------------------------------------------------------------------------------------------------------- stage C: the bars bite
def test_fp32_bars_bite_on_mutated_references(walk_b8):
    """Stage C: no kernel is touched -- the REFERENCE recomputation of B = 8's walk is corrupted the way a wiring bug would corrupt the plan,
    and each comparison must then miss its bar by at least 10 x (factor = mutated figure / bar; the unmutated figures are stage A's / B's):
      mask taken from the activation of the wrong block (layer2.1's bn1 sums with layer2.0's mask)      bn sums bound n 2^-24 sum|term|
      identity taken from y1 instead of the block input (layer1.1.out)                                 _ulp_close32: 4e-7 of the value
      sum dz computed without the ReLU mask (layer3.1's bn2 sums)                                      bn sums bound
      bilinear with align_corners=False (head.y2)                                                      _ulp_close32
      max-pool keeping the LAST tied slot (stem.idx)                                                   bar: NO window may differ; the mutant
                                                                                                       must differ in >= 10 windows
      one-pixel shift of one layer's input (layer3.1.y1)                                               convolution bar 1e-5
    Measured factors (B = 8): wrong mask 1.3e4, identity from y1 1.8e9, unmasked sum 5.3e3, align_corners=False 3.6e8, last tied slot
    10 400 windows (1.0e3 x 10), shifted input 1.1e5 -- none below 10: no bar of this file is too loose for the fault it is there for."""
    S = walk_b8
    t, sd = S.t, S.sd0
    factors = {}
    with _Threads():
        # 1. wrong mask source
        b, o = 'layer2.1', 'layer2.0'
        mask = _fma32(t[o + '.y1'], t[o + '.bn1'][0], t[o + '.bn1'][1]) > 0
        bn1, y1 = t[b + '.bn1'], t[b + '.y1']
        xhat = (y1.double() - bn1[2].double()) * bn1[3].double()
        factors['mask of the wrong block'] = _sum_multiple(t[b + '.red1'], t['tr.' + b + '.da1'].double() * mask.double(), xhat) / _N_FP32_TERMS
        # 2. identity from y1
        b = 'layer1.1'
        bn2 = t[b + '.bn2']
        _, worst = _ulp_worst(t[b + '.out'], torch.relu(_fma32(t[b + '.y2'], bn2[0], bn2[1]).double() + t[b + '.y1'].double()))
        factors['identity from y1'] = worst / 4e-7
        # 3. unmasked sum
        b = 'layer3.1'
        bn2, y2 = t[b + '.bn2'], t[b + '.y2']
        xhat = (y2.double() - bn2[2].double()) * bn2[3].double()
        factors['sum dz without the mask'] = _sum_multiple(t[b + '.red2'], t['tr.' + b + '.g_out'].double(), xhat) / _N_FP32_TERMS
        # 4. the other bilinear
        ref = nhwc(F.interpolate(nchw(t['head.z2'].double()), scale_factor=2, mode='bilinear', align_corners=False))
        _, worst = _ulp_worst(t['head.y2'], ref)
        factors['align_corners=False'] = worst / 4e-7
        # 5. last tied slot
        a0 = torch.relu(_fma32(t['stem.y0'], t['stem.bn'][0], t['stem.bn'][1]))
        _, first, last, tied = _pool_windows(a0)
        slot = nchw(t['stem.idx']).long()
        assert int((slot != first).sum()) == 0
        factors['last tied slot (windows that differ / 10)'] = int((slot != last).sum()) / 10.0
        # 6. shifted input
        b, key = 'layer3.1', 'resnet18.layer3.1.'
        xin = torch.roll(t['layer3.0.out'], 1, dims=2)
        y1ref = F.conv2d(nchw(xin.double()), sd[key + 'conv1.weight'].double(), padding=1)
        factors['one-pixel shift of the input'] = relmax(nchw(t[b + '.y1']), y1ref) / FWD_BAR[_fwd_form(256, 256, 3, 8, 'train')]
    print('\nstage C, B = 8: factor by which each mutated reference misses its bar: %s' % ', '.join('%s %.3g' % kv for kv in factors.items()))
    weak = {k: v for k, v in factors.items() if v < 10}
    assert not weak, 'bars too loose to see these mutations: %s' % weak
