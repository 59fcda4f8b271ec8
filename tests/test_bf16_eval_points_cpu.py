"""CPU: the reference arithmetic of the bf16 plan's eval walk (tests/bf16_eval_points_ref.py) before any GPU time is spent on it.
  1. fed the model's own planes (oracle/bf16_points.py fcn_forward(training=False), its optional taps) the helper reproduces the model plane
     for plane and its Q-map to 1e-12: the teacher-forced formulas ARE the model of DESIGN.md 3, one convolution at a time;
  2. a stand-in "kernel" -- torch float32 convolutions of the same bf16 operands with the float32 epilogue, i.e. what a correct HIP kernel
     computes up to its accumulation order -- passes every bar of the GPU walk (tests/test_gpu_bf16_eval_points.py, section 1): the reference
     stays inside the caps on its own, and the input conditions (>= 5 % zeros and >= 5 % positives in every post-ReLU plane, >= 1 % tied
     max-pool windows) hold for the seeds the GPU walk uses;
  3. the stand-in with each of the six wiring faults of the helper's header (mutants a-f) built into it fails the comparison of the tensor
     the fault produces, by the printed factor.
B = 2.  Measured here: the stand-in's worst convolution 0.014 % flips (layer4.0.out), 0.0039 of the value (2^-8: half a bf16 ulp, the rounding
itself), head.z2 2.4e-7, head.z3 4.0e-7, Q 5.6e-7 (torch's float32 bilinear map; bar 1e-6); zeros 25 % (pooled map), 31-57 % (the planes);
25 % of the max-pool windows tied; mutants: see test_mutated_standin_fails."""
import pytest
import torch

import bf16_eval_points_ref as R
from oracle import bf16_points as bp
from oracle import cases
from oracle import fcn as ofcn
from oracle import learner as olearner
from simq import synth
from test_gpu_bf16_points import _check_conv

CIN, COUT, B = 5, 2, 2
nchw, nhwc, rnd16 = R.nchw, R.nhwc, R.rnd16


@pytest.fixture(scope='module')
def net():
    sd = {k[len('module.'):]: v for k, v in ofcn.state_from_numpy(synth.make_state_dict(CIN, COUT, 77)).items()}
    x = torch.cat([olearner.apply_transform(s) for s in synth.make_states(B, CIN, 78)]).permute(0, 2, 3, 1).contiguous()
    return sd, x


def standin_forward(sd, x, mutant=None):
    """the eval forward as a correct kernel computes it, in float32 torch: every stored tensor by its workspace name"""
    f32 = torch.float32
    rc = mutant == 'a'
    plane = lambda v: nhwc(rnd16(v)).contiguous()
    t = {'x': x}
    for name, bnkey in R.bn_layers():
        t[name] = torch.stack(R.eval_coeff64(sd, bnkey)).float()
    t['stem.y0'] = plane(R.stem_conv(x, sd['resnet18.conv1.weight'], f32))
    sc, sh = R.eval_coeff64(sd, 'resnet18.bn1')
    mx, first, _ = R.stem_pool(t['stem.y0'], sc.float(), sh.float())
    t['stem.pool'], t['stem.idx'] = nhwc(mx).contiguous(), nhwc(first).to(torch.uint8).contiguous()
    cur = t['stem.pool.plane'] = rnd16(t['stem.pool'])
    for b, key, ds in R.blocks():
        bn1, bn2 = t[b + '.bn1'], t[b + '.bn2']
        t[b + '.a1'] = plane(R.folded(cur, sd[key + 'conv1.weight'], None, bn1[0], bn1[1], dtype=f32, round_conv=rc))
        identity = t['stem.pool'] if (mutant == 'b' and b == 'layer1.0') else cur
        if ds:
            bnd = t[b + '.bnd']
            identity = t[b + '.yd'] = plane(R.folded(cur, sd[key + 'downsample.0.weight'], None, bnd[0], bnd[1], relu=(mutant == 'c'), dtype=f32, round_conv=rc))
        co = bn1 if mutant == 'd' else bn2
        cur = t[b + '.out'] = plane(R.folded(t[b + '.a1'], sd[key + 'conv2.weight'], None, co[0], co[1], identity=identity, dtype=f32,
                                             round_conv=rc, add_after_relu=(mutant == 'e')))
    hb1, hb2 = t['head.bn1'], t['head.bn2']
    t['head.a1.plane'] = plane(R.folded(cur, sd['conv1.weight'], sd['conv1.bias'], hb1[0], hb1[1], dtype=f32, round_conv=rc))
    t['head.z2'] = nhwc(R.head_z2(t['head.a1.plane'], sd['conv2.weight'], sd['conv2.bias'], hb2[0], hb2[1], f32)).contiguous()
    t['head.z3'] = R.head_z3(t['head.z2'], sd['conv3.weight'], f32, relu_first=(mutant == 'f'))
    t['q'] = R.head_q(t['head.z3'], sd['conv3.bias'], f32)
    return t


def test_helper_reproduces_the_model_plane_for_plane(net):
    """1: the model's eval forward, tapped; every tap must be the helper's reference of it, computed from the taps in front of it."""
    sd, x = net
    state = cases.oracle_state(CIN, COUT, 77, torch.float64)
    taps = {}
    q = bp.fcn_forward(state, nchw(x).double(), False, taps=taps)
    assert torch.equal(q, bp.fcn_forward(state, nchw(x).double(), False)), 'the taps changed the model'
    t = {'x': x, 'stem.y0': nhwc(taps['stem.conv']), 'stem.pool': nhwc(taps['stem.pool']), 'stem.idx': torch.zeros(B, 24, 24, 64),
         'stem.pool.plane': rnd16(nhwc(taps['stem.pool'])).double()}
    for name, bnkey in R.bn_layers():
        t[name] = torch.stack(R.eval_coeff64(sd, bnkey))
    for b, _, ds in R.blocks():
        t[b + '.a1'], t[b + '.out'] = nhwc(taps[b + '.a1']), nhwc(taps[b])
        if ds:
            t[b + '.yd'] = nhwc(taps[b + '.yd'])
    t['head.a1.plane'], t['head.z2'] = nhwc(taps['head.a1']), nhwc(taps['head.z2'])
    t['head.z3'] = R.head_z3(t['head.z2'], sd['conv3.weight'])         # (the model runs conv3 behind the second bilinear map: no tap, they commute)
    t['q'] = q
    seen = set()
    for c in R.eval_walk(t, sd):
        if c.kind == 'conv':                                           # the model's plane == the rounding of the helper's reference
            e = float((c.got.double() - rnd16(c.ref).double()).abs().max())
            assert e <= 1e-12 * float(c.ref.abs().max()), (c.name, e)
        elif c.kind == 'rel':
            assert R.rel_error(c.got, c.ref) <= 1e-12, c.name
        elif c.name == 'stem.pool':                                    # (the helper forms the pooled map as the kernel does, fp32 fma; the model in fp64)
            assert R.rel_error(c.got, c.ref) < 4e-7, c.name
        seen.add(c.name)
    want = {'stem.y0', 'head.a1.plane', 'head.z2', 'head.z3', 'q'} | {b + w for b, _, ds in R.blocks() for w in ('.a1', '.out') + (('.yd',) if ds else ())}
    assert want <= seen, want - seen


@pytest.fixture(scope='module')
def standin(net):
    sd, x = net
    return standin_forward(sd, x)


def test_standin_kernel_passes_every_bar(net, standin):
    """2: float32 convolutions of the same operands stay inside every bar of the GPU walk, and the inputs exercise ReLU and max-pool ties."""
    sd, _ = net
    log = []
    try:
        for c in R.eval_walk(standin, sd):
            R.assert_check(c, log, _check_conv)
    finally:
        print('\n' + '\n'.join(log))


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_mutated_standin_fails(net, standin, mutant):
    """3: each wiring fault built into the stand-in fails the comparison of the tensor it produces -- a fault that sits in ONE kernel shows in
    one tensor only, so EVERY target tensor of the mutant must miss its bar by at least 10 x (factor = figure / bar).  Measured (B = 2, smallest
    .. largest factor over the mutant's target tensors): a 12 .. 30 (the downsample branches, which have no zeros, 27-30), b 18, c 128,
    d 1.4e3 .. 6.5e3, e 4.0e3 .. 1.1e4, f 6.5e3."""
    sd, x = net
    targets = R.mutant_targets(mutant)
    t = standin_forward(sd, x, mutant)
    clean = {c.name: R.miss_factor(c) for c in R.eval_walk(standin, sd, only=set(targets))}
    factors = {c.name: R.miss_factor(c) for c in R.eval_walk(t, sd, only=set(targets))}
    assert set(factors) == set(targets)
    print('\nmutant %s: the stand-in misses its bar by %s' % (mutant, ', '.join('%s %.3g' % (k, factors[k]) for k in targets)))
    assert max(clean.values()) < 1, clean
    assert min(factors.values()) >= 10, 'mutant %s is all but invisible: %s' % (mutant, factors)
