"""CPU: what PyTorch does with NaN and Inf in the operations of the learner -- the reference DESIGN.md 22 pins the HIP kernels to, asserted
here so that a torch upgrade that changes it is seen first -- and the reference-side counts tests/test_gpu_nonfinite.py relies on not to
be vacuous (how many outputs one poisoned input reaches)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import nonfinite_cases as nc
from oracle import cases
from oracle import fcn as ofcn
from oracle import learner as olearner

NAN, INF = float('nan'), float('inf')


def test_relu_keeps_nan_and_orders_the_infinities():
    r = F.relu(torch.tensor([NAN, -INF, INF, -0.0, -1.0, 2.0]))
    assert math.isnan(float(r[0])) and r[1:].tolist() == [0.0, INF, 0.0, 0.0, 2.0]
    # (the SIGN of relu(-0.0) is not taken from torch, whose CPU kernel hands -0.0 on: the kernels give +0.0, as they always did -- rule 4)


def test_max_pool_propagates_a_nan_of_the_window():
    x = torch.arange(36.0).reshape(1, 1, 6, 6)
    x[0, 0, 2, 3] = NAN
    p = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    want = torch.zeros(3, 3, dtype=torch.bool)
    want[1, 1] = want[1, 2] = True                          # the two windows (rows 1..3, columns 1..3 / 3..5) that hold the pixel
    assert torch.equal(torch.isnan(p[0, 0]), want)


def test_max_over_a_row_takes_the_first_nan():
    v, i = torch.tensor([[1.0, NAN, 3.0, NAN]]).max(1)
    assert math.isnan(float(v)) and int(i) == 1
    v, i = torch.full((1, 4), -INF).max(1)
    assert float(v) == -INF and int(i) == 0
    v, i = torch.tensor([[-0.0, 0.0, 0.0, 0.0]]).max(1)
    assert int(i) == 0


def test_smooth_l1_gradient_of_a_nan_and_at_the_knee():
    below, above = np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))
    assert below == np.float32(0.99999994) and above == np.float32(1.0000001) and below < 1 < above
    d = torch.tensor([1.0, -1.0, 0.0, float(below), float(above), NAN, INF], requires_grad=True)
    loss = F.smooth_l1_loss(d, torch.zeros(7), reduction='none')
    loss.sum().backward()
    g = d.grad
    # (to 1e-6: just below the knee the gradient is the difference itself, 0.99999994 -- pinned exactly in the next test)
    assert torch.allclose(g[:5], torch.tensor([1.0, -1.0, 0.0, 1.0, 1.0]), rtol=0, atol=1e-6) and g[:3].tolist() == [1.0, -1.0, 0.0] and float(g[4]) == 1.0
    assert math.isnan(float(g[5])) and float(g[6]) == 1.0
    assert torch.allclose(loss[:5], torch.tensor([0.5, 0.5, 0.0, 0.5, 0.5]), rtol=0, atol=1e-6) and loss[:3].tolist() == [0.5, 0.5, 0.0]
    assert math.isnan(float(loss[5])) and float(loss[6]) == INF


def test_smooth_l1_gradient_just_below_the_knee_is_the_difference_itself():
    below = float(np.nextafter(np.float32(1), np.float32(0)))
    d = torch.tensor([below], requires_grad=True)
    F.smooth_l1_loss(d, torch.zeros(1), reduction='sum').backward()
    assert float(d.grad[0]) == below                         # the quadratic branch: the gradient is d, 0.99999994 -- "1" to seven digits


def _clip(grads, max_norm=100.0):
    ps = [torch.zeros_like(g).requires_grad_(True) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return float(tn), [p.grad for p in ps]


def test_clip_grad_norm_with_nan_inf_and_zero_gradients():
    tn, g = _clip([torch.tensor([1.0, NAN, -2.0]), torch.tensor([3.0])])
    assert math.isnan(tn) and all(bool(torch.isnan(t).all()) for t in g)
    tn, g = _clip([torch.tensor([1.0, INF, -2.0]), torch.tensor([3.0])])
    assert tn == INF and torch.isnan(g[0]).tolist() == [False, True, False] and g[0][0] == 0 and g[0][2] == 0 and g[1][0] == 0
    tn, g = _clip([torch.zeros(3), torch.zeros(1)])
    assert tn == 0.0 and all(bool((t == 0).all()) for t in g)


def test_train_mode_batchnorm_with_one_nan():
    bn = torch.nn.BatchNorm2d(3).train()
    x = torch.randn(2, 3, 4, 4, generator=torch.Generator().manual_seed(1))
    x[1, 1, 2, 2] = NAN
    y = bn(x)
    assert torch.isnan(y).reshape(2, 3, -1).all(2).all(0).tolist() == [False, True, False]
    assert torch.isnan(y).reshape(2, 3, -1).any(2).any(0).tolist() == [False, True, False]
    assert torch.isnan(bn.running_mean).tolist() == [False, True, False] and torch.isnan(bn.running_var).tolist() == [False, True, False]


def test_one_poisoned_pixel_reaches_the_window_and_one_poisoned_weight_its_channel():
    """The counts of tests/test_gpu_nonfinite.py: 3x3 / pad 1 at 24x24, one pixel of one channel -> 9 * Cout outputs (4 * Cout from the corner);
    one weight -> every pixel of its output channel (the fp64 convolution multiplies the zero padding too)."""
    B, H, Cin, Cout = 2, 24, 16, 8
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(B, H, H, Cin, generator=g), torch.randn(Cout, 3, 3, Cin, generator=g)
    for site, n in (('interior', 9), ('border', 4)):
        for v in (NAN, INF):
            xi = x.clone()
            py, px = nc.sites(H)[site]
            xi[1, py, px, 5] = v
            bad = nc.nonfinite(nc.conv_ref(xi, w))
            assert int(bad.sum()) == n * Cout and not bool(bad[0].any())
            assert int(nc.tile_closure(bad, 2).sum()) >= n * Cout
    wi = w.clone()
    wi[3, 1, 2, 7] = NAN
    bad = torch.isnan(nc.conv_ref(x, wi))
    assert int(bad.sum()) == B * H * H and bool(bad[..., 3].all())


def test_one_poisoned_pixel_of_the_first_convolution():
    """7x7 / stride 2 / pad 3 at 96x96: an odd interior pixel is read by 4 x 4 outputs, the corner (0, 95) by 2 x 2."""
    g = torch.Generator().manual_seed(4)
    x, w = torch.randn(2, 96, 96, 5, generator=g), torch.randn(64, 7, 7, 5, generator=g)
    for site, n in (('interior', 16), ('border', 4)):
        xi = x.clone()
        py, px = nc.STEM_SITES[site]
        xi[1, py, px, 2] = NAN
        bad = torch.isnan(nc.conv_ref(xi, w, stride=2, pad=3))
        assert int(bad.sum()) == n * 64 and not bool(bad[0].any())


def test_the_oracle_network_on_one_poisoned_state():
    """oracle/fcn.py in fp64 on two states, one pixel of sample 1 poisoned.  Eval mode: sample 0 is clean, sample 1 is not.  Train mode: both
    Q-maps are NaN throughout (the batch statistics mix the samples) and so is every running statistic of the first BatchNorm."""
    cin, cout, B = 5, 2, 2
    x = torch.cat([olearner.apply_transform(s) for s in nc.network_state(cin, B, 22)]).double()
    with torch.no_grad():
        q = ofcn.fcn_forward(cases.oracle_state(cin, cout, 12, torch.float64), x, False)
    bad = torch.isnan(q)
    assert not bool(bad[0].any()) and bool(bad[1].any()) and bool(torch.isfinite(q[0]).all())
    st = cases.oracle_state(cin, cout, 12, torch.float64)
    with torch.no_grad():
        q = ofcn.fcn_forward(st, x, True)
    assert bool(torch.isnan(q).all())
    buf = cases.bn_buffer_vector(st)
    assert np.isnan(buf[:128]).all() and np.isnan(buf).any()
