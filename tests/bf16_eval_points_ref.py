"""Reference arithmetic of the bf16 plan's EVAL forward (csrc/forward.hip, `folded16` branch), tensor by tensor: what every tensor that
forward stores must be, given the STORED tensors it was made from.  Pure torch on the host -- tests/test_gpu_bf16_eval_points.py feeds it
the workspace of a HIP forward, tests/test_bf16_eval_points_cpu.py the planes of the model (oracle/bf16_points.py) and of a float32
stand-in, so the formulas the GPU test relies on are exercised without a GPU.

The eval forward (reference: networks.py:16-26, resnet.py:31-47,93-104 with BatchNorm in eval mode), in the order the plan runs it:
  stem.y0            bf16( conv7x7 / stride 2 ( bf16(x), bf16(w) ) )
  stem.pool          maxpool3x3 / stride 2 ( relu( fma(y0, scale, shift) ) ) in fp32, scale / shift from the running statistics (fp64,
                     rounded once); stem.pool.plane its rounding, stem.idx the first maximal window slot
  layer<l>.<b>.a1    bf16( relu( conv3x3(input plane, bf16(w1)) * scale1 + shift1 ) )
  layer<l>.<b>.yd    bf16(       conv1x1(input plane, bf16(wd)) * scaled + shiftd )                     (no ReLU; downsample blocks)
  layer<l>.<b>.out   bf16( relu( conv3x3(a1 plane, bf16(w2)) * scale2 + shift2 + identity plane ) )     identity = yd | the input plane
  head.a1.plane      bf16( relu( (conv1x1(layer4.1.out, bf16(w1)) + b1) * scale1 + shift1 ) )
  head.z2            fp32: (conv1x1(a1 plane, bf16(w2)) + b2) * scale2 + shift2 at 24x24 (the affine map commutes with the bilinear map)
  head.z3            fp32: conv3( relu( bilinear x2 (z2) ) ) at 48x48, no bias
  Q                  bilinear x2 (z3) + b3
Every convolution is computed here in `dtype` (float64: the reference; float32: the stand-in "kernel" of the CPU test) on operands that are
bf16 values, ONE rounding per stored plane.

MUTANTS (the ways a wiring bug would corrupt that forward; `mutant=` of folded-form functions below, used to show that the bars bite):
  'a'  the pre-affine convolution rounded to bf16 first (two roundings)
  'b'  layer1.0's identity taken from the fp32 pooled map instead of its plane
  'c'  ReLU applied to the downsample branch
  'd'  bn1's coefficients used for `out`
  'e'  the identity added after the ReLU
  'f'  the head's ReLU applied before the bilinear map
"""
import collections

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
BF16 = torch.bfloat16
MUTANTS = ('a', 'b', 'c', 'd', 'e', 'f')

nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)
rnd16 = lambda t: t.to(BF16)


def blocks():
    """(block name, state-dict prefix, has a downsample branch) in forward order"""
    for li in range(1, 5):
        for bi in range(2):
            yield 'layer%d.%d' % (li, bi), 'resnet18.layer%d.%d.' % (li, bi), (li > 1 and bi == 0)


def bn_layers():
    """(stored name of the coefficients, state-dict prefix of the BatchNorm) of every layer bn_eval_coeff serves"""
    for b, key, ds in blocks():
        yield b + '.bn1', key + 'bn1'
        yield b + '.bn2', key + 'bn2'
        if ds:
            yield b + '.bnd', key + 'downsample.1'
    yield 'head.bn1', 'bn1'
    yield 'head.bn2', 'bn2'


def eval_coeff64(sd, bnkey):
    """scale | shift of an eval-mode BatchNorm from its running statistics, fp64"""
    invstd = 1.0 / torch.sqrt(sd[bnkey + '.running_var'].double() + BN_EPS)
    sc = sd[bnkey + '.weight'].double() * invstd
    return sc, sd[bnkey + '.bias'].double() - sd[bnkey + '.running_mean'].double() * sc


def fma32(y, sc, sh):
    """fp32 fma(y, sc[c], sh[c]) through fp64 (exact product and sum, one rounding)"""
    return (y.double() * sc.double() + sh.double()).float()


def pool_windows(a0):
    """NHWC [B,48,48,C] -> (max [B,C,24,24], first maximal slot, tied) over the 3x3 / stride-2 / pad-1 windows, slot = dy*3+dx"""
    p = F.pad(nchw(a0), (1, 1, 1, 1), value=float('-inf'))
    win = p.unfold(2, 3, 2).unfold(3, 3, 2).reshape(a0.shape[0], a0.shape[3], 24, 24, 9)
    mx = win.max(-1).values
    eq = win == mx.unsqueeze(-1)
    slots = torch.arange(9).view(1, 1, 1, 1, 9)
    first = torch.where(eq, slots, torch.full_like(slots, 9)).min(-1).values
    return mx, first, eq.sum(-1) > 1


def up2(t):
    return F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=True)


def _c(v, dtype):
    return v.to(dtype).view(1, -1, 1, 1)


def stem_conv(x, w, dtype=torch.float64):
    """NCHW, in front of the rounding: conv7x7 / stride 2 of bf16(x) [B,96,96,Cin] with bf16(w)"""
    return F.conv2d(nchw(rnd16(x).to(dtype)), rnd16(w).to(dtype), stride=2, padding=3)


def stem_pool(y0, sc, sh):
    """stem_pool_fwd on the stored bf16 y0 [B,48,48,64] with fp32 coefficients: (pooled fp32 NCHW, first maximal slot, tied)"""
    return pool_windows(torch.relu(fma32(y0.float(), sc, sh)))


def folded(xplane, w, bias, scale, shift, identity=None, relu=True, dtype=torch.float64, round_conv=False, add_after_relu=False):
    """NCHW value in front of the ONE rounding of a folded convolution:  [relu]( (conv(plane, bf16(w)) [+ bias]) * scale + shift [+ identity] ).
    xplane / identity: NHWC tensors holding bf16 values (identity may be fp32: mutant 'b').  round_conv: mutant 'a'; add_after_relu: 'e'."""
    y = F.conv2d(nchw(xplane.to(dtype)), rnd16(w).to(dtype), None if bias is None else bias.to(dtype), padding=w.shape[-1] // 2)
    if round_conv:
        y = rnd16(y).to(dtype)
    y = y * _c(scale, dtype) + _c(shift, dtype)
    if identity is not None and not add_after_relu:
        y = y + nchw(identity.to(dtype))
    if relu:
        y = torch.relu(y)
    if identity is not None and add_after_relu:
        y = y + nchw(identity.to(dtype))
    return y


def head_z2(a1plane, w2, b2, scale, shift, dtype=torch.float64):
    """NCHW [B,32,24,24]: conv2 + bias with BatchNorm 2's affine map folded, on the stored a1 plane"""
    y = F.conv2d(nchw(a1plane.to(dtype)), rnd16(w2).to(dtype), b2.to(dtype))
    return y * _c(scale, dtype) + _c(shift, dtype)


def head_z3(z2, w3, dtype=torch.float64, relu_first=False):
    """[B,Cout,48,48]: conv3 (no bias) of relu(bilinear x2 of the stored z2 [B,24,24,32]).  relu_first: mutant 'f'"""
    z = nchw(z2.to(dtype))
    a2 = up2(torch.relu(z)) if relu_first else torch.relu(up2(z))
    return F.conv2d(a2, w3.to(dtype))


def head_q(z3, b3, dtype=torch.float64):
    """[B,Cout,96,96]: bilinear x2 of the stored z3 [B,Cout,48,48] + bias"""
    return up2(z3.to(dtype)) + _c(b3, dtype)


# a comparison the walk asks for.  kind: 'coeff' (got [2,C] fp32 | ref [2,C] fp64, 1e-6), 'conv' (got bf16 NCHW | ref fp64 in front of the
# rounding: the bf16 walks' _check_conv bar), 'exact' (torch.equal), 'idx' (got slot | ref (first maximal slot, tied)), 'rel' (max-abs error
# over max-abs value < bar).  relu: ref is a post-ReLU tensor (the zero / positive fractions are asserted on it)
Check = collections.namedtuple('Check', 'name kind got ref bar relu')


def conv_figures(got16, ref64):
    """the two figures the bf16 walks' _check_conv asserts: fraction of stored elements != bf16(ref), worst error of the value"""
    frac = float((got16 != rnd16(ref64)).double().mean())
    worst = float(((got16.double() - ref64).abs() / ref64.abs().clamp_min(1e-2 * float(ref64.abs().max()))).max())
    return frac, worst


def conv_factor(got16, ref64):
    """by how much a comparison misses the _check_conv bar (< 1 % flips, worst < 2^-7 of the value): > 1 fails"""
    frac, worst = conv_figures(got16, ref64)
    return max(frac / 1e-2, worst / 2 ** -7)


def rel_error(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def assert_check(c, log, check_conv):
    """one comparison of the eval walk under its bar (check_conv: the bf16 walks' _check_conv); post-ReLU references must exercise the ReLU"""
    if c.kind == 'coeff':
        e = max(rel_error(c.got[0], c.ref[0]), rel_error(c.got[1], c.ref[1]))
        log.append('  %-22s scale / shift vs fp64 from the running statistics %.1e' % (c.name, e))
        assert e < c.bar, (c.name, e)
    elif c.kind == 'conv':
        check_conv(c.name, c.got, c.ref, log)
    elif c.kind == 'exact':
        assert torch.equal(c.got, c.ref), c.name + ' is not its bit-exact emulation'
    elif c.kind == 'idx':
        first, tied = c.ref
        frac = float(tied.double().mean())
        wrong = int((c.got != first).sum())
        log.append('  %-22s %.1f %% of the windows tied; idx != first maximal slot in %d windows' % (c.name, 100 * frac, wrong))
        assert frac >= 0.01, 'the tie rule of the max-pool is not exercised: %.3g of the windows tied' % frac
        assert wrong == 0, c.name
    else:
        e = rel_error(c.got, c.ref)
        log.append('  %-22s %.2e of the range (bar %.0e)' % (c.name, e, c.bar))
        assert e < c.bar, (c.name, e)
    if c.relu:
        plane = c.ref if c.kind == 'exact' else rnd16(c.ref)
        zeros, pos = float((plane == 0).double().mean()), float((plane > 0).double().mean())
        log.append('  %-22s reference plane: %.0f %% zeros, %.0f %% positive' % (c.name, 100 * zeros, 100 * pos))
        assert zeros >= 0.05 and pos >= 0.05, (c.name, zeros, pos)


def eval_walk(t, sd, mutant=None, only=None):
    """Every comparison of the eval walk, one at a time (a generator: the fp64 references of a large batch are not held together).  t: stored tensors by their workspace names, as stored (NHWC; 'x' the fp32 input, 'stem.pool' the
    fp32 pooled map, 'head.z3' [B,Cout,48,48], 'q' the returned Q-map); sd: the state dict without the 'module.' prefix.  The reference of
    a tensor is computed from the STORED tensors it was made from.  mutant: corrupt the reference (see the header); only: names to compute."""
    assert mutant is None or mutant in MUTANTS
    want = lambda name: only is None or name in only
    rc = mutant == 'a'
    for name, bnkey in bn_layers():
        if want(name):
            yield Check(name, 'coeff', t[name][:2], torch.stack(eval_coeff64(sd, bnkey)), 1e-6, False)
    if want('stem.y0'):
        yield Check('stem.y0', 'conv', nchw(t['stem.y0']), stem_conv(t['x'], sd['resnet18.conv1.weight']), None, False)
    if want('stem.pool') or want('stem.idx'):
        sc, sh = eval_coeff64(sd, 'resnet18.bn1')
        mx, first, tied = stem_pool(t['stem.y0'], sc.float(), sh.float())
        yield Check('stem.pool', 'exact', nchw(t['stem.pool']), mx, None, True)
        yield Check('stem.idx', 'idx', nchw(t['stem.idx']).long(), (first, tied), None, False)
    if want('stem.pool.plane'):
        yield Check('stem.pool.plane', 'exact', t['stem.pool.plane'], rnd16(t['stem.pool']), None, False)
    cur = t['stem.pool.plane']
    for b, key, ds in blocks():
        bn1, bn2 = t[b + '.bn1'], t[b + '.bn2']
        if want(b + '.a1'):
            yield Check(b + '.a1', 'conv', nchw(t[b + '.a1']), folded(cur, sd[key + 'conv1.weight'], None, bn1[0], bn1[1], round_conv=rc), None, True)
        identity = t['stem.pool'] if (mutant == 'b' and b == 'layer1.0') else cur
        if ds:
            bnd = t[b + '.bnd']
            if want(b + '.yd'):
                yield Check(b + '.yd', 'conv', nchw(t[b + '.yd']),
                                 folded(cur, sd[key + 'downsample.0.weight'], None, bnd[0], bnd[1], relu=(mutant == 'c'), round_conv=rc), None, False)
            identity = t[b + '.yd']
        if want(b + '.out'):
            co = bn1 if mutant == 'd' else bn2
            yield Check(b + '.out', 'conv', nchw(t[b + '.out']),
                             folded(t[b + '.a1'], sd[key + 'conv2.weight'], None, co[0], co[1], identity=identity, round_conv=rc,
                                    add_after_relu=(mutant == 'e')), None, True)
        cur = t[b + '.out']
    hb1, hb2 = t['head.bn1'], t['head.bn2']
    if want('head.a1.plane'):
        yield Check('head.a1.plane', 'conv', nchw(t['head.a1.plane']),
                         folded(cur, sd['conv1.weight'], sd['conv1.bias'], hb1[0], hb1[1], round_conv=rc), None, True)
    if want('head.z2'):
        yield Check('head.z2', 'rel', nchw(t['head.z2']), head_z2(t['head.a1.plane'], sd['conv2.weight'], sd['conv2.bias'], hb2[0], hb2[1]), 2e-5, False)
    if want('head.z3'):
        yield Check('head.z3', 'rel', t['head.z3'], head_z3(t['head.z2'], sd['conv3.weight'], relu_first=(mutant == 'f')), 1e-5, False)
    if want('q'):
        yield Check('q', 'rel', t['q'], head_q(t['head.z3'], sd['conv3.bias']), 1e-6, False)


# the tensors whose comparison each mutant must break
def mutant_targets(mutant):
    if mutant == 'a':
        names = []
        for b, _, ds in blocks():
            names += [b + '.a1', b + '.out'] + ([b + '.yd'] if ds else [])
        return names + ['head.a1.plane']
    if mutant == 'b':
        return ['layer1.0.out']
    if mutant == 'c':
        return [b + '.yd' for b, _, ds in blocks() if ds]
    if mutant in ('d', 'e'):
        return [b + '.out' for b, _, _ in blocks()]
    return ['head.z3']


def miss_factor(c):
    """by how much a 'conv' / 'rel' comparison misses its bar"""
    return conv_factor(c.got, c.ref) if c.kind == 'conv' else rel_error(c.got, c.ref) / c.bar
