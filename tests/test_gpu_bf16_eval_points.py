"""GPU: the OTHER two forwards of a bf16 TD step, teacher-forced kernel by kernel -- the target net's eval forward (MODE_EVAL: what
DQNPolicy.step / step_many act with, train.py:122) and the policy's no-grad train-mode forward over the next states (train.py:120).
tests/test_gpu_bf16_points.py walks the grad-mode forward and the backward; the eval forward of a default bf16 plan runs code no train-mode
forward runs (csrc/forward.hip, `folded16`): conv_bn_folded_planes -- scale / shift, a bf16 residual, ReLU and ONE rounding to a bf16 plane in
the convolution epilogue (both implementations of csrc/igemm_epilogue.h, every bf16 forward family) --, the downsample branch as a
post-BatchNorm plane in the idle `yd` buffer, block 1's identity from the pooled PLANE, bn_eval_coeff, stem_pool_fwd on running statistics,
the head's conv2 with BatchNorm 2 folded at 24x24, head_up_relu_conv3.  None of that can be reached at operator level
(simq_conv2d_fwd_bf16 takes a bias and statistics only), and the network-level bars that saw it (TD targets 3e-2, Q 5e-2) cannot see a
residual from the wrong plane or a second rounding.  Here every tensor that forward stores is recomputed in fp64 from the STORED tensors
it was made from (tests/bf16_eval_points_ref.py, exercised on the CPU by tests/test_bf16_eval_points_cpu.py), so every comparison has the
bar of one kernel -- the bars the train-mode walks already use for the same kernels, none fitted here:
  BatchNorm coefficients   layer*.bn1|bn2|bnd, head.bn1|bn2 rows scale | shift against fp64 from the running statistics: 1e-6; the running
                           statistics bit-identical before and after
  stem.y0                  == bf16(fp64 conv7x7(bf16(x), bf16(w))): _check_conv (< 1 % one-ulp flips, worst < 2^-7 of the value)
  stem.pool / .plane / idx maxpool(relu(fma(y0, sc, sh))) BIT for bit, its rounding, the first maximal slot (>= 1 % of the windows tied)
  every folded convolution layer*.a1, layer*.yd (no ReLU), layer*.out (identity = the stored yd plane | the previous out plane | stem.pool.plane),
                           head.a1.plane (with conv1's bias): the stored plane == bf16([relu](conv64(stored input plane, bf16(w)) [+ bias]) *
                           stored scale + stored shift [+ stored identity plane]) under _check_conv
  head.z2 (fp32)           (conv1x1(a1 plane, bf16(w2)) + b2) * scale2 + shift2: 2e-5 of the range
  head.z3, Q               conv3(relu(bilinear x2 of the stored z2)): 1e-5; bilinear x2 of the stored z3 + bias: 1e-6
  inputs                   every post-ReLU reference plane holds >= 5 % zeros and >= 5 % positives
B = 6 / 29 (ragged) run the register-staged and 288-row tiles; only B = 128, the bench's batch, selects the image-tile, LDS-resident and
large 1x1 families (asserted through the launch log; the plain bn_apply, upsample2x_fwd and the head's kernels are no families of that log,
so their absence from it proves nothing: the log is printed, and bn_apply16 must not be in it).
Section 2: the two unfolded eval forms the library ships (fold_eval_bn_bf16 = 0; keep_fp32_activations = 1) at B = 6 -- the train-mode block
walk with coefficients from the running statistics.  Section 3: the no-grad train-mode forward at B = 6 / 29 -- the train-mode walks with
MODE_TRAIN_NOGRAD and workspace slot 'tmp'.  Section 4: the bars bite -- the REFERENCE of B = 6's eval walk corrupted six ways, each
comparison must then miss its bar by >= 10 x.

MEASURED (MI355X, one run of this file together with tests/test_gpu_bf16_points.py; every test prints its own figures):
  eval walk, B = 6 / 29 / 128   coefficients 5.7e-8; convolutions worst 0.014 / 0.012 / 0.012 % one-ulp flips, 0.0039 of the value (2^-8: half
                                a bf16 ulp, the rounding itself); stem.pool, its plane and idx exact, 25.6 / 25.6 / 25.4 % of the windows tied;
                                head.z2 1.9e-7 / 1.9e-7 / 2.0e-7, head.z3 2.1e-7 / 2.1e-7 / 2.5e-7, Q 5.3e-7 / 5.4e-7 / 5.5e-7; reference planes
                                25 % zeros (pooled map) .. 58 %
  launch log, B = 128           igemm_bf16_img_whole x 8, igemm_bf16_img_half x 4, igemm_bf16_c64 x 4, igemm_bf16_pp x 2, igemm_bf16_dma x 2,
                                igemm_bf16_reg x 1, stem_conv_bf16 x 1 -- the families of the train-mode forward at that batch, less bn_apply16 x 15
  unfolded forms, B = 6         pre-BatchNorm convolutions worst 0.025 % flips, a1 / out 0 elements off the emulation; bn_apply16 x 15 (no_fold);
                                Q-map against the folded plan's, rel-L2: 6.2e-3 (no_fold), 6.2e-3 (fp32_act)
  no-grad walk, B = 6 / 29      convolutions worst 0.023 % flips, elementwise 0 elements off; Q against the bilinear map of the stored z3
                                2.2e-8 / 4.0e-8 with lerp2x's fp32 weights, 1.55e-6 / 1.02e-6 with fp64 weights
  mutants, B = 6 (factor by which the comparisons a fault reaches miss their bar, smallest .. largest)
                                a 12.3 (layer1.1.a1) .. 30.1 (layer2.0.yd), b 16.8, c 1.2e4 .. 1.7e4, d 1.2e3 .. 5.0e3, e 128 (a stored zero
                                against a positive reference: worst = 1, the cap of that figure), f 7.7e3 -- none below 10
  wall time                     this file 28 s: eval b6 / b29 / b128 1.0 / 3.2 / 15.7 s, unfolded forms 0.6 s each, no-grad b6 / b29 0.8 / 3.4 s,
                                mutants 0.5 s.  The train-mode walks in the same run: blocks b6 / b29 / b128 0.5 / 2.1 / 13.7 s, stem + head
                                b6 / b128 0.2 / 1.2 s (backward b128 30.8 s) -- the eval walk at B = 128, which covers stem, blocks and head,
                                costs 1.05 x its two train-mode siblings together (15.0 s), 0.3 s of it on the GPU side.
"""
import time

import pytest
import torch

import bf16_eval_points_ref as R
from oracle import fcn as ofcn
from oracle import learner as olearner
from simq import synth
from test_gpu_bf16_points import _FWD_FAMILIES_B128, _check_conv, rl2, walk_blocks_forward, walk_stem_and_head_forward
from test_gpu_fp32_points import _Threads, _fmt, _nearest_candidate, _up2x_emul, nchw, nhwc

pytestmark = pytest.mark.gpu

CIN, COUT = 5, 2


@pytest.fixture(scope='module')
def simq_mod():
    import simq
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return simq


class _Snap:
    pass


def _run_eval(simq_mod, B):
    """ONE eval forward of the default bf16 plan (seeds 77 / 78, as the train-mode block walk) with every stored tensor copied to the host"""
    from simq import _lib
    S = _Snap()
    S.B = B
    net = simq_mod.FCN(CIN, COUT, precision='bf16')
    o = net.plan.options
    assert o['fold_eval_bn_bf16'] == 1 and o['keep_fp32_activations'] == 0 and o['stem_bf16'] == 1, o
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(CIN, COUT, 77)))
    net.eval()
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, CIN, 78)]).permute(0, 2, 3, 1).contiguous().cuda()
    strip = lambda sd: {k[len('module.'):]: v.detach().cpu().clone() for k, v in sd.items()}
    S.sd = strip(net.state_dict())
    net._ensure_weights()
    _lib.lib.call('simq_launch_counts_reset')
    q = net._forward_raw(x, _lib.MODE_EVAL)
    torch.cuda.synchronize()
    S.ran = _lib.launch_counts()
    stored = lambda name: net.stored_tensor(name, B, 'tmp').cpu()
    t = S.t = {'x': x.cpu(), 'q': q.cpu(), 'stem.pool': net.saved_activation('stem.pool', B, 'tmp').cpu()}
    planes = ['stem.y0', 'stem.pool.plane', 'head.a1.plane']
    for b, _, ds in R.blocks():
        planes += [b + '.a1', b + '.out'] + ([b + '.yd'] if ds else [])
    for name in planes + ['stem.idx', 'head.z2'] + [n for n, _ in R.bn_layers()]:
        t[name] = stored(name)
    assert all(t[name].dtype == torch.bfloat16 for name in planes) and t['head.z2'].dtype == torch.float32
    t['head.z3'] = stored('head.z3').reshape(B, COUT, 48, 48)          # (stored channel-major, like the Q-map it becomes)
    sd1 = strip(net.state_dict())
    moved = [k for k in S.sd if 'running_' in k and not torch.equal(S.sd[k], sd1[k])]
    assert not moved, 'an eval forward moved the running statistics: %s' % moved
    return S


@pytest.fixture(scope='module')
def walk_b6(simq_mod):
    """the default plan's eval forward at B = 6, shared by section 1 (b6), section 2 (the Q-map the unfolded forms are printed against) and
    section 4"""
    return _run_eval(simq_mod, 6)


def _assert_eval_launches(S):
    B, ran = S.B, S.ran
    print('\n  B = %d eval forward launch log: %s' % (B, _fmt(ran)))
    assert ran.get('stem_conv_bf16', 0) == 1, ran
    for f in ('bn_apply16', 'bn_apply', 'upsample2x_fwd'):
        assert ran.get(f, 0) == 0, (f, ran)
    if B == 128:
        missing = [f for f in _FWD_FAMILIES_B128 if f != 'bn_apply16' and ran.get(f, 0) == 0]
        assert not missing, 'B = 128 eval forward did not select %s (ran: %s)' % (missing, ran)
        assert ran.get('igemm_bf16_pp', 0) + ran.get('igemm_bf16_dma', 0) > 0          # the 1x1 downsample / head convolutions: large LDS-DMA tiles


@pytest.mark.parametrize('B', [6, 29, 128], ids=['b6', 'b29', 'b128'])
def test_bf16_eval_forward_teacher_forced(simq_mod, request, B):
    """Section 1: every tensor ONE eval forward of the default bf16 plan stores, against fp64 on the stored tensors it was made from (bars:
    the header).  B = 128 must have run the image-tile, c64 and large 1x1 families -- with the folded epilogue, there is no other in this mode."""
    t0 = time.perf_counter()
    S = request.getfixturevalue('walk_b6') if B == 6 else _run_eval(simq_mod, B)
    t1 = time.perf_counter()
    _assert_eval_launches(S)
    log = []
    try:
        with _Threads():
            for c in R.eval_walk(S.t, S.sd):
                R.assert_check(c, log, _check_conv)
    finally:
        print('\n'.join(log))
        print('  B = %d: forward + copies %.1f s, fp64 walk %.1f s' % (B, t1 - t0, time.perf_counter() - t1))


_UNFOLDED = {'no_fold': {'fold_eval_bn_bf16': 0}, 'fp32_act': {'keep_fp32_activations': 1}}


@pytest.mark.parametrize('form', sorted(_UNFOLDED))
def test_bf16_unfolded_eval_forms_teacher_forced(simq_mod, walk_b6, form):
    """Section 2: the eval forward of a plan with the fold switched off (fold_eval_bn_bf16 = 0, or keep_fp32_activations = 1 through
    planes_only()) is the train-mode sequence with coefficients from the running statistics: pre-BatchNorm y1 / y2 / yd under _check_conv,
    a1 / out == the fma / add / max emulation (bit-exact but for < 1e-4 half-way cases; the fp32 copies where the plan keeps them), the running
    statistics untouched.  Launch log: bn_apply16 took the 8 a1 and 7 of the 8 out launches of the planes-only form (layer1.0.out adds the
    fp32 pooled map: bn_apply_kernel, which like every launch of the fp32-copies form is no family of the log -- there bn_apply16 must be
    absent).  Printed, not asserted: rel-L2 of each form's Q-map against the default plan's -- bf16 re-rounding noise (an eval Q is 2.9e-3
    from the model, header of test_gpu_bf16_points.py)."""
    q, ran = walk_blocks_forward(simq_mod, 6, 'eval', _UNFOLDED[form])
    assert ran.get('stem_conv_bf16', 0) == 1, ran
    assert ran.get('bn_apply16', 0) == (15 if form == 'no_fold' else 0), ran
    print('  %s: Q-map vs the default (folded) plan, rel-L2 %.3g' % (form, rl2(q, walk_b6.t['q'])))


@pytest.mark.parametrize('B', [6, 29], ids=['b6', 'b29'])
def test_bf16_nograd_forward_teacher_forced(simq_mod, B):
    """Section 3: the policy's no-grad train-mode forward (MODE_TRAIN_NOGRAD, workspace slot 'tmp') under the train-mode walks' bars: the
    blocks (seeds 77 / 78), the stem and the head (91 / 92) -- where head.a2 must be refused for that slot and the Q-map is what conv3 and
    the bilinear map make of the stored y2 / bn2: z3 at 1e-5, Q at the train-mode walk's own 2e-6 against the fp64 bilinear map of the stored
    z3 -- and at 1e-6 against the bilinear map with the weights the operation forms in fp32 (head.hip lerp2x, as torch's float32 kernel:
    scale * o in fp32 carries an ulp of a coordinate up to 47, 3.8e-6, times the step between two neighbours of z3; the references of
    tests/test_gpu_fp32_points.py for the same kernel, which forms l1 with one rounding or two, column by column).  Against exact fp64
    weights this Q-map is 1.55e-6 (B = 6) / 1.02e-6 (B = 29) off -- the same number the train-mode walk passes under 2e-6, both forwards being the same arithmetic --:
    1e-6 there is below what fp32 coordinates give, on this seed; the eval walk's Q (seeds 77 / 78) is 5.3e-7 .. 5.5e-7 and keeps 1e-6."""
    walk_blocks_forward(simq_mod, B, 'nograd')
    q, z3, b3 = walk_stem_and_head_forward(simq_mod, B, 'nograd')
    with _Threads():
        cands = [nchw(_up2x_emul(nhwc(z3), fx, fy)).float().double() + b3.double().view(1, -1, 1, 1) for fx in (True, False) for fy in (True, False)]
        e_k, e_64 = R.rel_error(q, _nearest_candidate(q, cands)), R.rel_error(q, R.head_q(z3, b3))
    print('  B = %d no-grad Q-map vs the bilinear x2 of the stored z3 + bias: %.2e with lerp2x\'s fp32 weights (bar 1e-6), %.2e with fp64 weights' % (B, e_k, e_64))
    assert e_k < 1e-6, (e_k, e_64)


def test_bf16_eval_bars_bite_on_mutated_references(walk_b6):
    """Section 4: no kernel is touched -- the REFERENCE of B = 6's eval walk is corrupted the way a wiring bug would corrupt the forward
    (tests/bf16_eval_points_ref.py: a two roundings, b layer1.0's identity from the fp32 pooled map, c ReLU on the downsample branch, d bn1's
    coefficients for `out`, e identity added after the ReLU, f the head's ReLU before the bilinear map), and EVERY comparison the fault reaches
    must then miss its bar by at least 10 x (factor = figure / bar; conv: max(flips / 1 %, worst / 2^-7)).  The factors are printed."""
    S = walk_b6
    weak = {}
    with _Threads():
        for m in R.MUTANTS:
            targets = R.mutant_targets(m)
            factors = {c.name: R.miss_factor(c) for c in R.eval_walk(S.t, S.sd, mutant=m, only=set(targets))}
            assert set(factors) == set(targets)
            lo, hi = min(factors, key=factors.get), max(factors, key=factors.get)
            print('\n  mutant %s: %d comparisons miss their bar by %.3g (%s) .. %.3g (%s)' % (m, len(factors), factors[lo], lo, factors[hi], hi))
            if factors[lo] < 10:
                weak[m] = {k: v for k, v in factors.items() if v < 10}
    assert not weak, 'bars too loose to see these mutations: %s' % weak
