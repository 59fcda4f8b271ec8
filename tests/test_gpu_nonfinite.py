"""GPU: NaN and Inf through the learner kernels, against PyTorch on the CPU evaluated live.

Rule 1, no swallowing: where the reference is NaN the kernel is NaN, where it is not finite the kernel is not finite.  Rule 2, containment:
nothing else is non-finite (the Winograd forms may add the output tiles the reference's set touches), and what both give as finite meets the
bar the kernel has in tests/test_gpu_ops.py / test_gpu_bnfuse.py.  Rule 3: simq_q_argmax is tensor.max(1).  A value is injected at one
interior element and at one on the border (so that a halo / padding select is crossed), NaN, +Inf and -Inf one at a time; shapes are the
smallest at which the kernel family is still selected.  Every reference's non-finite set is asserted to be neither empty nor everything
(nonfinite_cases.check_against_reference; the counts themselves: tests/test_nonfinite_reference_cpu.py)."""
import random
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nonfinite_cases as nc
from nonfinite_cases import NAN, PINF, NINF, VALUES, check_against_reference, nonfinite
from oracle import cases
from oracle import fcn as ofcn
from oracle import learner as olearner
from simq import synth

pytestmark = pytest.mark.gpu

SITES = ['interior', 'border']


@pytest.fixture(scope='module')
def L():
    from simq import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib


@pytest.fixture(scope='module')
def simq_mod():
    import simq
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return simq


def same_sets(got, ref, what=''):
    """elementwise kernels: the NaN set and the +Inf / -Inf sets are the reference's"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    for name, f in (('NaN', torch.isnan), ('+Inf', torch.isposinf), ('-Inf', torch.isneginf)):
        assert torch.equal(f(got), f(ref)), '%s: %s set differs: %d vs the reference\'s %d' % (what, name, int(f(got).sum()), int(f(ref).sum()))


def bits_equal_outside(got, clean, mask):
    """bit-equal to the clean run of the same call outside `mask`"""
    a, b = got.detach().cpu(), clean.detach().cpu()
    keep = ~mask.cpu()
    return torch.equal(a[keep].view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b[keep].view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def close_where_finite(got, ref, tol, what=''):
    """same NaN / Inf sets, finite elements within tol of the largest finite reference value"""
    same_sets(got, ref, what)
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    fin = torch.isfinite(ref)
    if bool(fin.any()):
        err = float((got - ref)[fin].abs().max() / ref[fin].abs().max().clamp_min(1e-30))
        assert err < tol, (what, err)


# ---- simq_bn_relu_apply / simq_bn_relu_backward ---------------------------------------------------------------------------------------

ROWS, C = 2 * 24 * 24, 64
ELEMS = {'interior': (ROWS // 2 + 7, 21), 'border': (ROWS - 1, C - 1)}        # (the last element of the tensor: the end of the last block's trip)


def _bn_operands(storage, residual, seed):
    g = torch.Generator().manual_seed(seed)
    acc = torch.randn(ROWS, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    stats = torch.cat([acc.double().sum(0), (acc.double() ** 2).sum(0)])
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.4 * torch.randn(C, generator=g)
    res = torch.randn(ROWS, C, generator=g) if residual else None
    dt = torch.bfloat16 if storage else torch.float32
    return acc.to(dt), stats, gamma, beta, None if res is None else res.to(dt)


def _bn_apply(L, y, stats, gamma, beta, res, storage):
    out = torch.zeros(ROWS, C, dtype=y.dtype, device='cuda')
    saved, running = torch.zeros(4 * C, device='cuda'), torch.cat([torch.full((C,), 0.25), torch.full((C,), 1.5)]).cuda()
    keep = [y.cuda(), stats.cuda(), gamma.cuda(), beta.cuda(), None if res is None else res.cuda()]
    L.lib.call('simq_bn_relu_apply', L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(keep[3]), L.ptr(keep[4]), 1, L.ptr(out), ROWS, C, storage,
               L.ptr(saved), L.ptr(running), L.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu(), saved.cpu(), running.cpu()


# (storage, residual, where, site, value): a y element and a residual element at both sites with NaN, +Inf and -Inf; one NaN statistic
APPLY = [(st, res, where, site, value) for st in (0, 1) for res in (False, True) for where in (('y', 'res') if res else ('y',))
         for site in SITES for value in VALUES] + [(st, res, 'stats', site, 'nan') for st in (0, 1) for res in (False, True) for site in SITES]


@pytest.mark.parametrize('storage,residual,where,site,value', APPLY,
                         ids=['%s_%s_%s_%s_%s' % (('fp32', 'bf16')[a[0]], ('plain', 'res')[a[1]], a[2], a[3], a[4]) for a in APPLY])
def test_bn_relu_apply(L, storage, residual, where, site, value):
    """relu(fma(y, scale, shift) [+ res]): bn_apply_kernel / bn_apply16_kernel.  Reference: the same expression in torch, with the scale / shift
    the clean call saved.  A NaN statistic (the sum of one channel) makes that channel's scale and shift NaN, hence the whole channel.  The
    elements the injection cannot reach are bit-equal to the clean run of the same call."""
    y, stats, gamma, beta, res = _bn_operands(storage, residual, 40 + storage)
    clean, saved, _ = _bn_apply(L, y, stats, gamma, beta, res, storage)
    r, c = ELEMS[site]
    y2, stats2, res2 = y.clone(), stats.clone(), None if res is None else res.clone()
    sc, sh = saved[:C].clone(), saved[C:2 * C].clone()
    assert float(sc[c]) > 0                                   # (gamma > 0: an Inf of y keeps its sign)
    reach = torch.zeros(ROWS, C, dtype=torch.bool)
    if where == 'y':
        y2[r, c] = VALUES[value]
        reach[r, c] = True
    elif where == 'res':
        res2[r, c] = VALUES[value]
        reach[r, c] = True
    else:
        stats2[c] = NAN
        sc[c] = sh[c] = NAN
        reach[:, c] = True
    got, saved2, running2 = _bn_apply(L, y2, stats2, gamma, beta, res2, storage)
    ref = torch.addcmul(sh, y2.float(), sc)
    if res2 is not None:
        ref = ref + res2.float()
    ref = torch.relu(ref)
    bad = nonfinite(ref)
    if value == 'ninf':
        assert not bool(bad.any()) and float(got[r, c]) == 0.0          # relu(-Inf) is 0: nothing non-finite may appear
    else:
        assert torch.equal(bad, reach)
    same_sets(got, ref, 'bn_relu_apply %s %s' % (where, value))
    assert bits_equal_outside(got, clean, reach)
    if where == 'stats':
        assert bool(torch.isnan(saved2.view(4, C)[:, c]).all()) and bool(torch.isnan(running2.view(2, C)[:, c]).all())
        keep = torch.ones(C, dtype=torch.bool); keep[c] = False
        assert torch.equal(saved2.view(4, C)[:, keep], saved.view(4, C)[:, keep])
    else:
        assert torch.equal(saved2, saved)


BACKWARD = [(st, mk, site, 'g') for st in (0, 1) for mk in (0, 1, 2) for site in SITES] + [(st, 1, site, 'mask') for st in (0, 1) for site in SITES]


@pytest.mark.parametrize('storage,mask_kind,site,where', BACKWARD,
                         ids=['%s_%s_%s_%s' % (('fp32', 'bf16')[a[0]], ('nomask', 'mask_tensor', 'mask_from_preact')[a[1]], a[2], a[3]) for a in BACKWARD])
def test_bn_relu_backward(L, storage, mask_kind, site, where):
    """dz = g * (a > 0), dy = gamma * invstd * (dz - sum/rows - xhat * sum/rows) with the sums given.  A NaN of g reaches dz and dy at its own
    element where the mask is set and nowhere else; a NaN in the mask ACTIVATION selects nothing ((NaN > 0) is false, as in the reference's
    ReLU backward): that case must stay finite and equal -- it guards against a fix that makes every comparison NaN-aware."""
    y, stats, gamma, beta, _ = _bn_operands(storage, False, 60 + storage + mask_kind)
    dt = y.dtype
    act, saved, _ = _bn_apply(L, y, stats, gamma, beta, None, storage)
    g = torch.randn(ROWS, C, generator=torch.Generator().manual_seed(5)).to(dt)
    r, c = ELEMS[site]
    pre = torch.addcmul(saved[C:2 * C], y.float(), saved[:C])
    if mask_kind:                                             # an element the mask keeps, next to the site
        while not (act[r, c].float() > 0 and pre[r, c] > 0):
            r -= 1
    red = torch.cat([g.double().sum(0), (g.double() * 0.1).sum(0)])          # (any finite pair of sums: they are operands here)

    def run(gv, av):
        dy, dzo = torch.zeros(ROWS, C, dtype=dt, device='cuda'), torch.zeros(ROWS, C, dtype=dt, device='cuda')
        dgam, dbet = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
        keep = [gv.cuda(), av.cuda(), y.cuda(), saved.cuda(), gamma.cuda(), red.cuda()]
        L.lib.call('simq_bn_relu_backward', L.ptr(keep[0]), L.ptr(keep[1]) if mask_kind == 1 else None, mask_kind, L.ptr(keep[2]), L.ptr(keep[3]),
                   L.ptr(keep[4]), L.ptr(keep[5]), L.ptr(dy), L.ptr(dzo), L.ptr(dgam), L.ptr(dbet), ROWS, C, storage, L.stream_ptr())
        torch.cuda.synchronize()
        return dy.cpu(), dzo.cpu()

    dy0, dz0 = run(g, act)
    assert bool(torch.isfinite(dy0.float()).all())
    g2, act2 = g.clone(), act.clone()
    if where == 'g':
        g2[r, c] = NAN
    else:
        act2[r, c] = NAN
    dy1, dz1 = run(g2, act2)
    mask = torch.ones(ROWS, C, dtype=torch.bool) if mask_kind == 0 else (act2.float() > 0) if mask_kind == 1 else (pre > 0)
    dz_ref = torch.where(mask, g2.float(), torch.zeros(()))
    want = torch.isnan(dz_ref)
    assert int(want.sum()) == (1 if where == 'g' else 0)
    assert torch.equal(torch.isnan(dz1.float()), want) and torch.equal(torch.isnan(dy1.float()), want)
    assert bool(torch.isfinite(dy1.float())[~want].all())
    changed = want.clone()
    if where == 'mask':
        changed[r, c] = True                                 # the one element whose mask bit the NaN clears
        assert float(dz1[r, c]) == 0.0
    assert bits_equal_outside(dy1, dy0, changed) and bits_equal_outside(dz1, dz0, changed)


# ---- convolutions with the BatchNorm + ReLU on load ------------------------------------------------------------------------------------

def _bnrelu_operands(B, H, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, H, H, Cin, generator=g)
    y[:, 0, :, :] *= 6.0; y[:, -1, :, :] *= 6.0; y[:, :, 0, :] *= 6.0; y[:, :, -1, :] *= 6.0
    sc, sh = 0.5 + torch.rand(Cin, generator=g), 0.3 + 0.5 * torch.randn(Cin, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) / (Cin * 9) ** 0.5
    dy = torch.randn(B, H, H, Cout, generator=g)
    return y, sc, sh, w, dy


def _poison_bnrelu(y, sc, sh, where, site):
    y, sc = y.clone(), sc.clone()
    if where == 'y_pre':
        py, px = nc.sites(y.shape[1])[site]
        y[1, py, px, 5] = NAN
    else:
        sc[5] = NAN
    a = torch.relu(torch.addcmul(sh.double(), y.double(), sc.double()))      # F.relu keeps the NaN
    return y, sc, a


# form 0: image tile (64 -> 64) / implicit GEMM; 1: F(2x2,3x3); 2: F(4x4,3x3); the split-bf16 GEMMs where test_gpu_bnfuse.py runs them
FWD_BN = [(C_, form, gs) for C_ in (64, 128) for form in (0, 1, 2) for gs in ((0, 1) if form else (0,))]


@pytest.mark.parametrize('where,site', [('y_pre', 'interior'), ('y_pre', 'border'), ('in_scale', 'interior')], ids=['y_interior', 'y_border', 'scale'])
@pytest.mark.parametrize('C_,form,gemm_split', FWD_BN, ids=['c%d_form%d%s' % (c, f, '_split3' if s else '') for c, f, s in FWD_BN])
def test_conv_fwd_bnrelu_in(L, C_, form, gemm_split, where, site):
    B, H = 2, 24
    y, sc, sh, w, _ = _bnrelu_operands(B, H, C_, C_, 700 + C_ + form)
    y2, sc2, a = _poison_bnrelu(y, sc, sh, where, site)
    ref = nc.conv_ref(a, w)
    planes = {0: 0, 1: 16, 2: 36}[form]
    scratch = torch.empty(max(1, planes * C_ * C_ + 16 * B * (H // 2) ** 2 * 2 * C_), device='cuda') if form else None
    out = torch.zeros(B, H, H, C_, device='cuda')
    keep = [y2.cuda(), sc2.cuda(), sh.cuda(), w.cuda()]
    L.lib.call('simq_conv2d_fwd_bnrelu_in', L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(keep[3]), None, L.ptr(out), B, H, H, C_, C_, 3, 3, 1, 1,
               form, L.ptr(scratch), L.stream_ptr(), opts=L.launch_opts(gemm_split=gemm_split))
    torch.cuda.synchronize()
    what = 'conv(relu(bn(y))) %d form %d split %d %s %s' % (C_, form, gemm_split, where, site)
    if where == 'in_scale':                # a whole input channel is NaN: so is every output, in the reference and here
        assert bool(torch.isnan(ref).all()) and bool(torch.isnan(out).all()), what
        return
    check_against_reference(out, ref, 2e-5 if form == 2 else 1e-5, nc.tile_closure(nonfinite(ref), 2 * form) if form else None, what)


WG_BN = [(64, 0, 0), (128, 0, 0), (128, 1, 0), (128, 1, 1)]


@pytest.mark.parametrize('where,site', [('y_pre', 'interior'), ('y_pre', 'border'), ('in_scale', 'interior')], ids=['y_interior', 'y_border', 'scale'])
@pytest.mark.parametrize('C_,form,gemm_split', WG_BN, ids=['c%d_form%d%s' % (c, f, '_split3' if s else '') for c, f, s in WG_BN])
def test_conv_wgrad_bnrelu_in(L, C_, form, gemm_split, where, site):
    """dW = dY^T * relu(bn(y)): a poisoned activation element of channel ci reaches the taps of dW[:, :, :, ci] whose window holds it (all nine
    from the interior, four from the corner), a poisoned scale all of dW[:, :, :, ci].  The transform-domain form (1) may fill the filters it
    touches: G^T dU G mixes a filter's transform elements into each of its taps."""
    B, H = 2, 24
    y, sc, sh, _, dy = _bnrelu_operands(B, H, C_, C_, 900 + C_ + form)
    y2, sc2, a = _poison_bnrelu(y, sc, sh, where, site)
    ref = nc.wgrad_ref(a, dy, 3, 1)
    scratch = torch.empty(36 * C_ * C_ + 16 * B * (H // 2) ** 2 * 2 * C_, device='cuda') if form else None
    dw = torch.zeros(C_, 3, 3, C_, device='cuda')
    keep = [y2.cuda(), sc2.cuda(), sh.cuda(), dy.cuda()]
    L.lib.call('simq_conv2d_wgrad_bnrelu_in', L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(keep[3]), L.ptr(dw), B, H, H, C_, C_, 3, 3, 1, 1, form,
               L.ptr(scratch), L.stream_ptr(), opts=L.launch_opts(gemm_split=gemm_split))
    torch.cuda.synchronize()
    bad = torch.isnan(ref)
    assert int(bad.sum()) == C_ * {'interior': 9, 'border': 4}[site] and bool(bad[..., 5].any()) and int(bad.sum()) == int(bad[..., 5].sum())
    # (B = 2: 72 F(4x4,3x3) tiles are no multiple of 16, so form 1 runs F(2x2,3x3) -- the 1e-5 bar of test_gpu_bnfuse.py)
    check_against_reference(dw, ref, 1e-5, nc.tap_closure(bad) if form else None, 'wgrad over relu(bn(y)) %d form %d split %d %s %s' % (C_, form, gemm_split, where, site))


# ---- simq_wino4f_output ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', [0, 1], ids=['one_pixel_kernel', 'two_phase_kernel'])
def test_wino4f_output_with_relu(L, form):
    """One NaN transform-domain product m[1][2] of one channel (C = 64, one tile: the smallest geometry of test_gpu_wino4f_output.py).  A^T m A
    gives every pixel of the 4x4 tile a non-zero multiple of it (rows 1 .. 4 of A have no zero), so the whole tile of that channel is NaN
    behind scale / shift / residual / ReLU, and every other channel is bit-equal to the clean run."""
    Cc, B, H, ch = 64, 1, 4, 37
    gen = torch.Generator(device='cuda').manual_seed(11)
    mt = torch.randn(36, 1, Cc, generator=gen, device='cuda')
    t = {k: torch.randn(Cc, generator=gen, device='cuda') for k in ('bias', 'scale', 'shift')}
    t['addend'] = torch.randn(B, H, H, Cc, generator=gen, device='cuda')
    clean = L.wino4f_output(mt, torch.zeros(B, H, H, Cc, device='cuda'), form=form, relu=True, **t).clone()
    assert bool(torch.isfinite(clean).all()) and bool((clean == 0).any())          # the ReLU clips somewhere
    mt2 = mt.clone()
    mt2[1 * 6 + 2, 0, ch] = NAN
    got = L.wino4f_output(mt2, torch.zeros(B, H, H, Cc, device='cuda'), form=form, relu=True, **t)
    torch.cuda.synchronize()
    want = torch.zeros(B, H, H, Cc, dtype=torch.bool)
    want[..., ch] = True
    assert torch.equal(torch.isnan(got).cpu(), want), 'NaN at %d of the tile\'s 16 pixels' % int(torch.isnan(got).sum())
    assert bits_equal_outside(got, clean, want)


# ---- the plain convolution entries ------------------------------------------------------------------------------------------------------

def _conv_case(B, H, Cin, Cout, k, seed, relu_input=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, H, Cin, generator=g)
    if relu_input:
        x = torch.relu(x)
    w = torch.randn(Cout, k, k, Cin, generator=g) / (Cin * k * k) ** 0.5
    return x, w


def _poison_conv(x, w, what, site, stem=False):
    x, w = x.clone(), w.clone()
    if what == 'w_nan':
        w[3, w.shape[1] // 2, 0, 1] = NAN
    else:
        py, px = (nc.STEM_SITES if stem else nc.sites(x.shape[1]))[site]
        x[1, py, px, 1] = VALUES[what[2:]]
    return x, w


WHATS = [('x_nan', 'interior'), ('x_nan', 'border'), ('x_pinf', 'interior'), ('x_pinf', 'border'), ('w_nan', 'interior')]
WHAT_IDS = ['x_nan_interior', 'x_nan_border', 'x_pinf_interior', 'x_pinf_border', 'w_nan']


@pytest.mark.parametrize('what,site', WHATS, ids=WHAT_IDS)
@pytest.mark.parametrize('tile', [(0, 0), (32, 32)], ids=['image_tile', 'implicit_gemm'])
def test_conv2d_fwd(L, tile, what, site):
    B, H, Cin, Cout = 2, 24, 64, 64
    x, w = _conv_case(B, H, Cin, Cout, 3, 1234)
    x2, w2 = _poison_conv(x, w, what, site)
    y = torch.zeros(B, H, H, Cout, device='cuda')
    keep = [x2.cuda(), w2.cuda()]
    L.lib.call('simq_conv2d_fwd', L.ptr(keep[0]), L.ptr(keep[1]), None, L.ptr(y), B, H, H, Cin, Cout, 3, 3, 1, 1, None, L.stream_ptr(), opts=L.launch_opts(tile=tile))
    torch.cuda.synchronize()
    check_against_reference(y, nc.conv_ref(x2, w2), 1e-4, None, 'conv2d_fwd %s %s %s' % (tile, what, site))


@pytest.mark.parametrize('what,site', WHATS, ids=WHAT_IDS)
@pytest.mark.parametrize('nplanes,bar', [(2, 5e-5), (1, 2e-5)], ids=['split_bf16x3', 'bf16'])
def test_conv2d_fwd_bf16(L, nplanes, bar, what, site):
    """split-bf16: fp32-class against fp64 (5e-5); plain bf16: 2e-5 against fp64 on the bf16-ROUNDED operands -- the bars of
    test_conv_bf16_matrix_core_paths.  Rounding to bf16 keeps NaN and Inf, so the reference's non-finite set is the same on either operand."""
    B, H, Cin, Cout = 3, 24, 64, 64
    x, w = _conv_case(B, H, Cin, Cout, 3, 99)
    x2, w2 = _poison_conv(x, w, what, site)
    y = torch.zeros(B, H, H, Cout, device='cuda')
    scratch = torch.empty(2 * (x.numel() + w.numel()) + 64, dtype=torch.int16, device='cuda')
    keep = [x2.cuda(), w2.cuda()]
    L.lib.call('simq_conv2d_fwd_bf16', L.ptr(keep[0]), L.ptr(keep[1]), None, L.ptr(y), B, H, H, Cin, Cout, 3, 3, 1, 1, nplanes, L.ptr(scratch), None, L.stream_ptr())
    torch.cuda.synchronize()
    ref = nc.conv_ref(x2, w2) if nplanes == 2 else nc.conv_ref(x2.bfloat16(), w2.bfloat16())
    check_against_reference(y, ref, bar, None, 'conv2d_fwd_bf16 planes %d %s %s' % (nplanes, what, site))


WINO = [(False, 2, 8, 64, 64, 0), (False, 2, 24, 128, 128, 1), (True, 2, 24, 128, 128, 0), (True, 2, 24, 128, 128, 1)]


@pytest.mark.parametrize('what,site', WHATS, ids=WHAT_IDS)
@pytest.mark.parametrize('f4,B,H,Cin,Cout,gemm_split', WINO, ids=['f2_narrow', 'f2_l2_split3', 'f4_l2', 'f4_l2_split3'])
def test_conv2d_fwd_winograd(L, f4, B, H, Cin, Cout, gemm_split, what, site):
    """Both Winograd forms, fp32-MFMA and split-bf16 GEMMs ('narrow': the smallest case of test_conv_winograd_forward_matches_direct, which the
    split form does not take).  Tile allowance of rule 2: 2x2 / 4x4 output tiles.  A NaN weight: the whole output channel, as in the reference."""
    x, w = _conv_case(B, H, Cin, Cout, 3, 17 + Cin + (1 if f4 else 0), relu_input=f4)
    x2, w2 = _poison_conv(x, w, what, site)
    nb, T = (36, B * (H // 4) ** 2) if f4 else (16, B * (H // 2) ** 2)
    scratch = torch.empty(nb * Cout * Cin + nb * T * (Cin + Cout) + 64, device='cuda')
    y = torch.zeros(B, H, H, Cout, device='cuda')
    keep = [x2.cuda(), w2.cuda()]
    L.lib.call('simq_conv2d_fwd_winograd4' if f4 else 'simq_conv2d_fwd_winograd', L.ptr(keep[0]), L.ptr(keep[1]), None, L.ptr(y), B, H, H, Cin, Cout, None,
               L.ptr(scratch), L.stream_ptr(), opts=L.launch_opts(gemm_split=gemm_split))
    torch.cuda.synchronize()
    ref = nc.conv_ref(x2, w2)
    check_against_reference(y, ref, 2e-5 if f4 else 1e-5, nc.tile_closure(nonfinite(ref), 4 if f4 else 2), 'winograd f4=%s split %d %s %s' % (f4, gemm_split, what, site))


@pytest.mark.parametrize('what,site', WHATS, ids=WHAT_IDS)
@pytest.mark.parametrize('bf16', [False, True], ids=['stem_f32', 'stem_bf16'])
def test_conv2d_fwd_stem(L, bf16, what, site):
    """7x7 / stride 2 / pad 3, Cin = 5: one pixel reaches 4 x 4 (corner: 2 x 2) outputs x 64 channels.  Bars of the two stem tests of
    test_gpu_ops.py: fp32 1e-5 of the range against fp64; bf16 2^-8 against fp64 on the bf16-rounded operands."""
    B, Cc = 2, 5
    g = torch.Generator().manual_seed(43)
    x = torch.randn(B, 96, 96, Cc, generator=g)
    x[:, 0, :, :] += 3.0; x[:, -1, :, :] -= 3.0; x[:, :, 0, :] += 5.0; x[:, :, -1, :] -= 5.0
    w = torch.randn(64, 7, 7, Cc, generator=g) * (2.0 / (49 * Cc)) ** 0.5
    x2, w2 = _poison_conv(x, w, what, site, stem=True)
    keep = [x2.cuda(), w2.cuda()]
    if bf16:
        y = torch.zeros(B, 48, 48, 64, dtype=torch.bfloat16, device='cuda')
        scratch = torch.empty(58368, dtype=torch.uint8, device='cuda')
        L.lib.call('simq_conv2d_fwd_stem_bf16', L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(y), B, 96, 96, Cc, None, L.ptr(scratch), L.stream_ptr())
        ref, bar = nc.conv_ref(x2.bfloat16(), w2.bfloat16(), stride=2, pad=3), 2.0 ** -8
    else:
        y = torch.zeros(B, 48, 48, 64, device='cuda')
        L.lib.call('simq_conv2d_fwd_stem_f32', L.ptr(keep[0]), L.ptr(keep[1]), L.ptr(y), B, 96, 96, Cc, None, L.stream_ptr())
        ref, bar = nc.conv_ref(x2, w2, stride=2, pad=3), 1e-5
    torch.cuda.synchronize()
    check_against_reference(y.float(), ref, bar, None, 'stem bf16=%s %s %s' % (bf16, what, site))


# ---- learner kernels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [2 * 96 * 96, 1000], ids=['n18432', 'n1000'])
def test_q_argmax_and_gather_are_tensor_max(L, n):
    """Rule 3: a NaN is the maximum, the first NaN's index is returned, the maximum is NaN.  n = 1000 is no multiple of the 1024-thread block
    (24 threads hold nothing); 'late' puts the NaN past a thread's first trip where the row allows it (index >= 1024), behind a larger finite value."""
    g = torch.Generator().manual_seed(n)
    q = torch.randn(8, n, generator=g)
    late = 1500 if n > 1500 else n - 2
    q[0, 17] = q[0, n - 100] = NAN
    q[1] = NAN
    q[2] = NINF
    q[3, n - 1] = NAN
    q[4, 3] = 50.0; q[4, late] = NAN
    q[5] = -1.0; q[5, 0] = -0.0; q[5, 1] = 0.0
    q[6] = 0.0; q[6, 0] = -0.0
    q[7, 5] = PINF; q[7, 9] = NAN
    ref_max, ref_idx = q.max(1)
    assert ref_idx.tolist() == [17, 0, 0, n - 1, late, 0, 0, 9] and torch.isnan(ref_max).tolist() == [True, True, False, True, True, False, False, True]
    qd = q.cuda()
    idx, mx, out = torch.full((8,), -7, dtype=torch.int64, device='cuda'), torch.zeros(8, device='cuda'), torch.zeros(8, device='cuda')
    L.lib.call('simq_q_argmax', L.ptr(qd), 8, n, L.ptr(idx), L.ptr(mx), L.stream_ptr())
    L.lib.call('simq_q_gather', L.ptr(qd), 8, n, L.ptr(idx), L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == ref_idx.tolist()
    for v in (mx.cpu(), out.cpu()):
        assert torch.equal(torch.isnan(v), torch.isnan(ref_max))
        keep = ~torch.isnan(ref_max)
        assert torch.equal(v[keep].view(torch.int32), ref_max[keep].view(torch.int32))          # bit for bit: -Inf, and the -0.0 at index 0


def _td_case(with_nonfinite):
    B, n, gamma = 9, 2 * 96 * 96, 0.85
    below, above = float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2)))
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, n, generator=g)
    a = torch.randint(0, n, (B,), generator=g)
    # q_sa = 0, next value 0, reward -d: the difference q_sa - (r + gamma * 0) is d exactly
    d = [1.0, -1.0, 0.0, below, above, 0.3, -2.5, 0.75, 1.5]
    q[torch.arange(B), a] = 0.0
    r = -torch.tensor(d)
    nsv = torch.zeros(B)
    if with_nonfinite:
        r[5] = NAN                     # a NaN reward
        q[6, a[6]] = NAN               # a NaN Q at the action
        r[7] = NINF                    # y = -Inf: the difference is +Inf
    q[8, a[8]] = 0.25; nsv[8] = 0.4    # one ordinary row
    return B, n, gamma, q, a, r, nsv


@pytest.mark.parametrize('with_nonfinite', [True, False], ids=['nan_inf_rows', 'knee_rows_only'])
def test_td_huber_at_the_knee_and_with_nonfinite_differences(L, with_nonfinite):
    """Differences of exactly +-1, 0, the two neighbours of 1, NaN (from the reward, and from Q at the action) and +Inf against smooth_l1_loss and
    its autograd: same NaN / Inf positions in q_sa, y, td, the two sums and dq, the rest to the 1e-6 of test_td_huber_and_scatter.  The second
    case has the same rows without the three non-finite ones, so that the Huber SUM at the knee is compared as a number too."""
    B, n, gamma, q, a, r, nsv = _td_case(with_nonfinite)
    qt = q.clone().requires_grad_(True)
    q_sa = qt.gather(1, a.unsqueeze(1)).squeeze(1)
    y = r + gamma * nsv
    loss = F.smooth_l1_loss(q_sa, y)
    loss.backward()
    outs = [torch.zeros(B, device='cuda') for _ in range(3)]
    out4, dq = torch.zeros(4, device='cuda'), torch.empty(B, n, device='cuda')
    keep = [q.cuda(), a.cuda(), r.cuda(), nsv.cuda()]
    L.lib.call('simq_td_huber', L.ptr(keep[0]), B, n, L.ptr(keep[1]), L.ptr(keep[2]), L.ptr(keep[3]), gamma, 1.0 / B,
               L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(out4), L.ptr(dq), L.stream_ptr())
    torch.cuda.synchronize()
    td_ref = (q_sa - y).abs().detach()
    assert torch.isnan(td_ref).tolist() == [False] * 5 + [with_nonfinite, with_nonfinite, False, False] and (float(td_ref[7]) == PINF) == with_nonfinite
    close_where_finite(outs[0], q_sa.detach(), 1e-6, 'q_sa')
    close_where_finite(outs[1], y, 1e-6, 'y')
    close_where_finite(outs[2], td_ref, 1e-6, 'td')
    close_where_finite(out4[0:1] / B, loss.detach().reshape(1), 1e-6, 'loss')
    close_where_finite(out4[1:2] / B, td_ref.mean().reshape(1), 1e-6, 'td sum')
    assert bool(torch.isnan(loss)) == with_nonfinite
    close_where_finite(dq, qt.grad, 1e-6, 'dq')
    rows = dq.cpu()[torch.arange(B), a]
    assert torch.isnan(rows).tolist() == [False] * 5 + [with_nonfinite, with_nonfinite, False, False]
    assert int((dq != 0).sum()) <= B


@pytest.mark.parametrize('kind', ['nan', 'inf', 'zero'])
def test_clip_sgd_with_nonfinite_and_zero_gradients(L, kind):
    """clip_grad_norm_ + optim.SGD (momentum 0.9, weight decay 1e-4), count = 1003 (a tail of three behind the float4 body): a clean first step,
    then a step whose gradient holds one NaN / one Inf / only zeros.  NaN: the norm, every gradient, parameter and momentum element are NaN.
    Inf: the norm is Inf, the coefficient 0 -- the finite gradients become 0, the Inf one NaN.  Zeros: nothing is scaled."""
    count, max_norm = 1003, 100.0
    g = torch.Generator().manual_seed(count)
    p = torch.randn(count, generator=g)
    grads = [torch.randn(count, generator=g) * 0.05, torch.randn(count, generator=g) * 0.05]
    if kind == 'zero':
        grads[1] = torch.zeros(count)
    else:
        grads[1][1001] = NAN if kind == 'nan' else PINF          # (in the scalar tail)
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([pt], lr=0.01, momentum=0.9, weight_decay=1e-4)
    pd, md = p.cuda(), torch.zeros(count, device='cuda')
    scratch, tn = torch.zeros(4, dtype=torch.float64, device='cuda'), torch.zeros(1, device='cuda')
    for step, grad in enumerate(grads):
        pt.grad = grad.clone()
        tn_ref = torch.nn.utils.clip_grad_norm_([pt], max_norm)
        g_ref = pt.grad.clone()
        opt.step()
        gd = grad.cuda()
        scratch.zero_()
        L.lib.call('simq_clip_sgd_step', L.ptr(pd), L.ptr(gd), L.ptr(md), count, max_norm, 0.01, 0.9, 1e-4, 1 if step == 0 else 0, L.ptr(scratch), L.ptr(tn),
                   L.stream_ptr())
        torch.cuda.synchronize()
        close_where_finite(tn, tn_ref.reshape(1), 1e-6, 'total_norm step %d' % step)
        close_where_finite(gd, g_ref, 1e-6, 'gradient step %d' % step)
        close_where_finite(pd, pt.detach(), 1e-6, 'parameters step %d' % step)
        close_where_finite(md, opt.state[pt]['momentum_buffer'], 1e-5, 'momentum step %d' % step)
    if kind == 'nan':
        assert bool(torch.isnan(tn).all()) and bool(torch.isnan(gd).all()) and bool(torch.isnan(pd).all()) and bool(torch.isnan(md).all())
    elif kind == 'inf':
        assert float(tn) == PINF and int(torch.isnan(gd).sum()) == 1 and bool((gd[:1001] == 0).all()) and int(torch.isnan(pd).sum()) == 1
    else:
        assert float(tn) == 0.0 and bool((gd == 0).all()) and bool(torch.isfinite(pd).all())


# ---- network level ----------------------------------------------------------------------------------------------------------------------

CIN, COUT, NB = 5, 2, 2
PRECISIONS = ['fp32', 'bf16']
Q_BAR = {'fp32': 1e-4, 'bf16': 3e-2}        # fp32: the Q-map bar of test_gpu_fcn.py; bf16: the bf16-class bar of a forward against fp64 (test_gpu_ops.py)
BN_BAR = {'fp32': 1e-4, 'bf16': 5e-3}       # running statistics: test_gpu_fcn.py / test_gpu_bf16_points.py


def _net(simq_mod, seed, training, precision):
    net = simq_mod.FCN(CIN, COUT, precision=precision)
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(CIN, COUT, seed)))
    net.train(training)
    return net


@pytest.fixture(scope='module')
def oracle_runs():
    """The fp64 oracle on the poisoned pair of states, once for every test of this section: eval-mode Q-map, train-mode Q-map and buffers."""
    x = nc.network_state(CIN, NB, 22)
    x_nchw = torch.cat([olearner.apply_transform(s) for s in x]).double()
    with torch.no_grad():
        q_eval = ofcn.fcn_forward(cases.oracle_state(CIN, COUT, 12, torch.float64), x_nchw, False)
        st = cases.oracle_state(CIN, COUT, 12, torch.float64)
        q_train = ofcn.fcn_forward(st, x_nchw, True)
    return dict(x=x, q_eval=q_eval, q_train=q_train, bn=cases.bn_buffer_vector(st))


@pytest.mark.parametrize('precision', PRECISIONS)
def test_train_mode_forward_on_a_poisoned_state(simq_mod, oracle_runs, precision):
    """One NaN pixel in sample 1: the batch statistics of the first BatchNorm are NaN, so both Q-maps are NaN throughout and every running
    statistic the oracle leaves NaN is NaN (the parent returned a finite, state-blind Q-map and NaN buffers behind it)."""
    o = oracle_runs
    assert bool(torch.isnan(o['q_train']).all())
    net = _net(simq_mod, 12, True, precision)
    with torch.no_grad():
        q = net.forward_nhwc(torch.from_numpy(o['x']).cuda())
    assert bool(torch.isnan(q).all()), '%d of %d Q values are not NaN' % (int((~torch.isnan(q)).sum()), q.numel())
    sd = net.state_dict()
    got = np.concatenate([sd[k].cpu().double().numpy().ravel() for k in sd if k.endswith('running_mean') or k.endswith('running_var')])
    bad = np.isnan(o['bn'])
    assert bad.any() and np.isnan(got[bad]).all(), '%d of the oracle\'s %d NaN running statistics are finite' % (int((~np.isnan(got[bad])).sum()), int(bad.sum()))
    if (~bad).any():
        assert np.isfinite(got[~bad]).all()
        assert float(np.abs(got[~bad] - o['bn'][~bad]).max() / np.abs(o['bn'][~bad]).max()) < BN_BAR[precision]


@pytest.mark.parametrize('precision', PRECISIONS)
def test_eval_mode_forward_on_a_poisoned_state(simq_mod, oracle_runs, precision):
    o = oracle_runs
    bad = torch.isnan(o['q_eval'])
    assert bool(bad[1].any()) and not bool(bad[0].any())
    net = _net(simq_mod, 12, False, precision)
    clean = np.array(o['x'], copy=True)
    clean[1] = synth.make_states(NB, CIN, 22)[1]
    with torch.no_grad():
        q = net.forward_nhwc(torch.from_numpy(o['x']).cuda()).cpu()
        q_clean = net.forward_nhwc(torch.from_numpy(clean).cuda()).cpu()
    assert bool(torch.isfinite(q_clean).all())
    assert torch.equal(q[0].view(torch.int32), q_clean[0].view(torch.int32)), 'sample 0 changed with sample 1\'s NaN'
    assert bool(torch.isnan(q[1])[bad[1]].all()), '%d of the oracle\'s %d NaNs of sample 1 are finite' % (int((~torch.isnan(q[1])[bad[1]]).sum()), int(bad[1].sum()))
    both = torch.isfinite(q[1]) & ~bad[1]
    if bool(both.any()):
        assert float((q[1].double() - o['q_eval'][1])[both].abs().max() / o['q_eval'][1][both].abs().max()) < Q_BAR[precision]
    assert float((q[0].double() - o['q_eval'][0]).abs().max() / o['q_eval'][0].abs().max()) < Q_BAR[precision]


def _fused_step(simq_mod, precision, poison):
    B = 2
    cfg, batch = cases.make_cfg(B), cases.make_batch(CIN, COUT, B, 43)
    if poison == 'state':
        s = [np.array(v, dtype=np.float32, copy=True) for v in batch.state]
        s[1][40, 57, 2] = NAN
        batch = batch._replace(state=tuple(s))
    else:
        batch = batch._replace(reward=(batch.reward[0], NAN))
    policy, target = _net(simq_mod, 33, True, precision), _net(simq_mod, 1033, False, precision)
    opt = torch.optim.SGD(policy.parameters(), lr=cases.LR, momentum=cases.MOMENTUM, weight_decay=cases.WEIGHT_DECAY)
    info = simq_mod.train(cfg, policy, target, opt, batch, olearner.apply_transform, cases.GAMMA)
    torch.cuda.synchronize()
    return info, policy


@pytest.mark.parametrize('poison', ['state', 'reward'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_fused_step_on_a_poisoned_transition(simq_mod, precision, poison):
    """simq.train on two transitions, a NaN in one state / a NaN reward on clean states: the reported loss, TD error and gradient norm are NaN and
    no parameter or momentum element survives, as clip_grad_norm_ + SGD leave them (the parent reported NaN and applied a finite step)."""
    info, policy = _fused_step(simq_mod, precision, poison)
    tn = float(policy._simq_opt_state.total_norm.item())
    assert np.isnan(info['loss']) and np.isnan(info['td_error']) and np.isnan(tn), (info, tn)
    for name, flat in (('parameter', policy.flat_params), ('momentum', policy._simq_opt_state.momentum)):
        for (pname, _, _), v in zip(policy._param_names, policy.reference_views(flat)):
            assert bool(torch.isnan(v).all()), '%s %s: %d of %d elements are not NaN' % (name, pname, int((~torch.isnan(v)).sum()), v.numel())


def test_onehot_head_backward_with_a_nan_td_error(simq_mod):
    """The one-hot head backward against the dense backward of the dQ map simq_td_huber writes (test_onehot_backward_equals_dense_backward), one
    transition's reward NaN: the same NaN set in the gradient of the last convolution (dw3 / db3: the output channel of that transition)."""
    from simq._lib import MODE_TRAIN, lib, ptr, stream_ptr
    cin, cout, B = 4, 2, 6
    net = simq_mod.FCN(cin, cout)
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, 77)))
    net.train(True)
    x = torch.from_numpy(synth.make_states(B, cin, 5)).cuda()
    q = net._forward_raw(x, MODE_TRAIN)
    n = cout * 96 * 96
    pix = [0, 95, 96 * 95, 96 * 96 - 1, 96 * 40 + 17, 96 * 3 + 94]
    action = torch.tensor([(i % cout) * 9216 + pix[i] for i in range(B)], dtype=torch.int64, device='cuda')
    reward = torch.linspace(-1.5, 2.0, B, device='cuda')
    reward[4] = NAN                                            # transition 4 acts on output channel 0
    nsv = torch.linspace(-0.5, 0.5, B, device='cuda')
    outs = [torch.empty(B, device='cuda') for _ in range(3)]
    out4, dq = torch.empty(4, device='cuda'), torch.empty_like(q)
    lib.call('simq_td_huber', ptr(q), B, n, ptr(action), ptr(reward), ptr(nsv), 0.75, 1.0 / B, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(out4), ptr(dq),
             stream_ptr(torch.device('cuda')))
    assert int(torch.isnan(dq).sum()) == 1
    views = lambda flat: {name: v.clone() for (name, _, _), v in zip(net._param_names, net.reference_views(flat))}
    g_dense = views(net._backward_raw(dq, B))
    g_onehot = views(net._backward_onehot(action, outs[0], outs[1], 1.0 / B, B))
    torch.cuda.synchronize()
    tail = [k for k in g_dense if k.endswith('conv3.weight') or k.endswith('conv3.bias')]
    assert len(tail) == 2
    for k in tail:
        bad = torch.isnan(g_dense[k])
        assert bool(bad[0].all()) and not bool(bad[1].any()), k          # channel 0 is NaN, channel 1 is not
        assert torch.equal(torch.isnan(g_onehot[k]), bad), k
        assert float((g_onehot[k] - g_dense[k])[~bad].abs().max() / g_dense[k][~bad].abs().max()) < 1e-4


def test_policy_step_on_a_poisoned_state(simq_mod):
    """DQNPolicy.step on one NaN state: the greedy action is what output.view(1, -1).max(1)[1] gives on the Q-map read back from the device."""
    cfg = types.SimpleNamespace(robot_config=[{'lifting_robot': 1}], num_input_channels=CIN, final_exploration=0.01, checkpoint_path=None)
    pol = simq_mod.DQNPolicy(cfg, train=False, random_seed=5)
    pol.policy_nets[0].load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(CIN, pol.policy_nets[0].num_output_channels, 51)))
    random.seed(5)
    s = nc.network_state(CIN, 1, 61, sample=0)[0]
    a, info = pol.step([[s]], exploration_eps=0.0, debug=True)
    out = torch.as_tensor(np.asarray(info['output'][0][0])).float()
    assert bool(torch.isnan(out).any())
    assert a[0][0] == int(out.reshape(1, -1).max(1)[1])
