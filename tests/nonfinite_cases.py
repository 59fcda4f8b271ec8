"""Shared pieces of tests/test_nonfinite_reference_cpu.py and tests/test_gpu_nonfinite.py: where a non-finite value is
injected, and the plain torch references whose non-finite sets the kernels are held to.  No GPU, no libsimq."""
import numpy as np
import torch
import torch.nn.functional as F

NAN, PINF, NINF = float('nan'), float('inf'), float('-inf')
VALUES = {'nan': NAN, 'pinf': PINF, 'ninf': NINF}


def sites(H, W=None):
    """The two pixels a value is injected at: one interior (its 3x3 window lies inside the map), one in a corner (the window crosses the
    zero padding on two sides, so a halo / padding select is on the path)."""
    W = H if W is None else W
    return {'interior': (H // 2 + 1, W // 2 - 2), 'border': (0, W - 1)}


# the first convolution (7x7, stride 2, pad 3, 96 -> 48): an odd interior pixel is read by 4 x 4 outputs, the corner (0, 95) by 2 x 2
STEM_SITES = {'interior': (41, 53), 'border': (0, 95)}


def nonfinite(t):
    return ~torch.isfinite(t)


def conv_ref(x_nhwc, w_ohwi, bias=None, stride=1, pad=1):
    """fp64 F.conv2d on NHWC / OHWI operands, NHWC result"""
    return F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w_ohwi.double().permute(0, 3, 1, 2), None if bias is None else bias.double(),
                    stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def wgrad_ref(a_nhwc, dy_nhwc, k, pad):
    """fp64 weight gradient dW = dY^T * a, OHWI"""
    cout, cin = dy_nhwc.shape[3], a_nhwc.shape[3]
    return torch.nn.grad.conv2d_weight(a_nhwc.double().permute(0, 3, 1, 2), (cout, cin, k, k), dy_nhwc.double().permute(0, 3, 1, 2),
                                       padding=pad).permute(0, 2, 3, 1).contiguous()


def tile_closure(mask_nhwc, t):
    """Every t x t output tile that `mask` touches, as a mask: what a Winograd form may add to the reference's non-finite set (its output
    transform mixes the whole tile)."""
    B, H, W, C = mask_nhwc.shape
    m = mask_nhwc.reshape(B, H // t, t, W // t, t, C).any(dim=4, keepdim=True).any(dim=2, keepdim=True)
    return m.expand(B, H // t, t, W // t, t, C).reshape(B, H, W, C)


def tap_closure(mask_ohwi):
    """Every (cout, cin) filter that `mask` touches, all taps: what the transform-domain weight gradient may add (G^T dU G mixes the 16 / 36
    transform elements of a filter into each of its nine taps)."""
    return mask_ohwi.any(dim=2, keepdim=True).any(dim=1, keepdim=True).expand_as(mask_ohwi)


def check_against_reference(out, ref, bar, allow=None, what=''):
    """DESIGN.md 22, rules 1 and 2.  out: the kernel's result, ref: the fp64 reference.  Rule 1: a NaN of the reference is a NaN, a
    non-finite value of the reference is not finite.  Rule 2: nothing else is non-finite -- but for `allow` (a mask: the tile closure
    of the Winograd forms) -- and where both are finite the kernel meets `bar` (max |error| over max |reference|, finite elements)."""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    rn, rnf, on, onf = torch.isnan(ref), nonfinite(ref), torch.isnan(out), nonfinite(out)
    assert bool(rnf.any()) and not bool(rnf.all()), '%s: vacuous case, the reference has %d of %d non-finite' % (what, int(rnf.sum()), rnf.numel())
    assert bool(on[rn].all()), '%s: %d of the reference\'s %d NaNs were swallowed' % (what, int((~on[rn]).sum()), int(rn.sum()))
    assert bool(onf[rnf].all()), '%s: %d of the reference\'s %d non-finite values came out finite' % (what, int((~onf[rnf]).sum()), int(rnf.sum()))
    extra = onf & ~rnf
    if allow is not None:
        extra = extra & ~allow
    assert not bool(extra.any()), '%s: %d non-finite outputs outside the reference\'s set' % (what, int(extra.sum()))
    both = ~onf & ~rnf
    err = float((out - ref)[both].abs().max() / ref[both].abs().max().clamp_min(1e-30))
    print('%s: %d non-finite (reference %d), finite elements %.3g of the range' % (what, int(onf.sum()), int(rnf.sum()), err))
    assert err < bar, (what, err, bar)
    return err


def network_state(cin, batch, seed, sample=1, pixel=(40, 57), channel=2, value=NAN):
    """`batch` synthetic HWC states with `value` in one pixel of one channel of one sample"""
    from simq import synth
    x = np.array(synth.make_states(batch, cin, seed), dtype=np.float32, copy=True)
    x[sample, pixel[0], pixel[1], channel] = value
    return x
