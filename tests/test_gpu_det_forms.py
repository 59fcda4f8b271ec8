"""GPU: the fixed-order sums of deterministic plans (simq_plan_options.deterministic = 1) after they left the step's critical path.

The slab sum (simq_wgrad_slab_sum) loads its splits in batches and the one-hot head backward runs one block per transition with a
one-block fold behind it; neither may change an operand, an operation or the order of a sum.  So everything here is an EQUALITY: against
a float32 fold on the CPU, against a step recorded from the build in front of the change, against the default plan where every sum has
two terms, and between two runs whose gradient buffer started as zeros and as NaNs.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import det_step_case as case                                         # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    from simq import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib


# ---- the slab sum on its own ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,splits', [(1, 1), (4099, 2), (12544, 33), (36864, 84), (147456, 96)])
@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'plus_one_float'])
def test_slab_sum_is_the_float32_fold_in_split_order(L, n, splits, offset):
    """d_dw[e] = ((slab[0][e] + slab[1][e]) + slab[2][e]) + ... in float32, element by element equal to the same fold on the CPU.
    Magnitudes are spread over 2^-20 ... 2^20 (no denormals: a difference of two such floats is 0 or at least 2^-44), so a sum taken in
    another order, in pairs or in a wider type differs in most elements.  Sizes: one element; a ragged n with two splits; the first
    convolution's 64 x 49 x 4 with a split count one past a batch of loads; the smallest and the largest slab a headline step sums
    (36 864 x 84, 147 456 x 96).  Once from 256-byte aligned pointers, once with both moved by one float."""
    g = torch.Generator().manual_seed(1000 * splits + n % 997)
    mag = torch.exp2(40.0 * torch.rand(splits, n, generator=g) - 20.0)
    slab = mag * (1.0 + torch.rand(splits, n, generator=g)) * (torch.randint(0, 2, (splits, n), generator=g).float() * 2 - 1)
    assert float(slab.abs().min()) >= 2.0 ** -21
    want = slab[0].clone()
    for s in range(1, splits):
        want = want + slab[s]
    dslab = torch.empty(splits * n + 1, device='cuda')[offset:offset + splits * n]
    dslab.copy_(slab.reshape(-1))
    ddw = torch.full((n + 1,), float('nan'), device='cuda')[offset:offset + n]
    assert dslab.data_ptr() % 256 == 4 * offset and ddw.data_ptr() % 256 == 4 * offset
    L.lib.call('simq_wgrad_slab_sum', L.ptr(dslab), L.ptr(ddw), n, splits, L.stream_ptr())
    got = ddw.cpu()
    assert torch.equal(got, want), '%d of %d elements differ from the float32 fold' % (int((got != want).sum()), n)


# ---- the step the build in front of the change computed ------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def parent_step(golden_dir):
    return np.load(os.path.join(golden_dir, 'det_step_parent.npz'))


@pytest.mark.parametrize('cin,cout,batch', case.SHAPES, ids=[case.key(*s) for s in case.SHAPES])
def test_deterministic_step_equals_the_recorded_parent_step(parent_step, cin, cout, batch):
    """tests/golden/det_step_parent.npz (tools/gen_det_step_golden.py) holds one deterministic fp32 TD step per shape as commit edad565
    ("Batched GPU shortest-path distance queries for the partial rewards") computed it on an MI355X, built by hipcc of ROCm 7.2.0 with
    --offload-arch=gfx950 -O3 -munsafe-fp-atomics: the one-hot head backward there was one block walking the transitions, the slab sum one
    load per add.  Loss, TD error, the last layer's gradients, 4096 seeded gradient elements and the SHA-256 of the whole gradient buffer
    and of the updated parameters must be EQUAL: the change moved when the terms are loaded, not what is added to what."""
    got = case.run(cin, cout, batch)
    for k, v in got.items():
        want = parent_step['%s.%s' % (case.key(cin, cout, batch), k)]
        if k in ('dw3', 'db3', 'picked'):
            print('\n%s %s: %d of %d elements differ' % (case.key(cin, cout, batch), k, int((v != want).sum()), v.size))
        assert np.array_equal(v, want), '%s of %s differs from the recorded parent step' % (k, case.key(cin, cout, batch))


# ---- the head's fold against the default plan where the order cannot matter ----------------------------------------------------------

def _net(cin, cout, options, seed=3):
    import simq
    from oracle import fcn as ofcn
    from simq import synth
    net = simq.FCN(cin, cout, precision='fp32', options=options)
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, seed)))
    net.train()
    return net


def _states(batch, cin, seed=5):
    from simq import synth
    return torch.from_numpy(synth.make_states(batch, cin, seed)).cuda()


def _head_grads(net, x, action, delta):
    """dw3, db3 of a one-hot backward with TD targets q_sa + delta, and q_sa."""
    from simq import _lib
    B = x.shape[0]
    q = net._forward_raw(x, _lib.MODE_TRAIN)
    q_sa = q.reshape(B, -1).gather(1, action.view(-1, 1)).reshape(-1).contiguous()
    g = net._backward_onehot(action, q_sa, (q_sa + delta).contiguous(), 1.0 / B, B)
    torch.cuda.synchronize()
    w0, w1 = case.tensor_range(net.plan, 'conv3.weight')
    b0, b1 = case.tensor_range(net.plan, 'conv3.bias')
    return g[w0:w1].clone(), g[b0:b1].clone(), q_sa


@pytest.mark.parametrize('batch', [4, 1])
def test_head_fold_equals_the_atomic_form_when_every_sum_has_two_terms(batch):
    """B = 4 with two transitions per output channel (B = 1: one): every fp32 sum of dw3 / db3 is 0 + a + b, which no order of the
    default plan's atomics can round differently, so the deterministic plan's per-transition stores + fold must give the very bits of
    the default plan's one-block-per-transition atomics.  Pixels include both corners of the 96x96 map (clamped bilinear taps)."""
    cin, cout = 4, 2
    pix = [0, 95 * 96 + 95, 37 * 96 + 5, 64 * 96 + 91][:batch]
    action = torch.tensor([(b % cout) * 9216 + p for b, p in enumerate(pix)], dtype=torch.int64, device='cuda')
    x = _states(batch, cin)
    out = {}
    for det in (1, 0):
        net = _net(cin, cout, {'deterministic': det})
        out[det] = _head_grads(net, x, action, torch.tensor([0.3, -0.6, 2.0, -0.05][:batch], device='cuda'))    # (one clamped Huber derivative)
        assert net.plan.options['deterministic'] == det
    assert torch.equal(out[1][2], out[0][2]), 'the forwards differ: the comparison below would mean nothing'
    assert float(out[0][0].abs().max()) > 0 and float(out[0][1].abs().max()) > 0
    assert torch.equal(out[1][0], out[0][0]), 'dw3: deterministic fold vs atomics'
    assert torch.equal(out[1][1], out[0][1]), 'db3: deterministic fold vs atomics'


# ---- no gradient element depends on what the buffer held before the backward pass ------------------------------------------------------

def _backward_forms(options):
    from simq import _lib
    cin, cout, B = 4, 2, 5
    x = _states(B, cin, seed=9)
    net = _net(cin, cout, options)
    gen = torch.Generator().manual_seed(17)
    action = torch.randint(0, cout * 9216, (B,), generator=gen).cuda()
    dq = (torch.randn(B, cout, 96, 96, generator=gen) / (B * 9216)).cuda()
    res = {}
    for form in ('onehot', 'dense', 'phases'):
        for fill in (0, 0x7fc00000):
            q = net._forward_raw(x, _lib.MODE_TRAIN)
            q_sa = q.reshape(B, -1).gather(1, action.view(-1, 1)).reshape(-1).contiguous()
            target = (q_sa - 0.5).contiguous()
            net.flat_grads.view(torch.int32).fill_(fill)
            if form == 'onehot':
                net._backward_onehot(action, q_sa, target, 1.0 / B, B)
            elif form == 'dense':
                net._backward_raw(dq, B)
            else:
                net._backward_onehot(action, q_sa, target, 1.0 / B, B, phase=1)
                net._backward_onehot(action, q_sa, target, 1.0 / B, B, phase=2)
            torch.cuda.synchronize()
            res[form, fill] = net.flat_grads.clone()
    return res


def test_no_gradient_element_is_left_from_before_the_backward_pass():
    """A deterministic fp32 plan, B = 5: the gradient buffer is pre-filled with zeros and then with quiet NaNs (0x7fc00000) in front of
    the one-hot backward, the dense backward, and phase 1 followed by phase 2.  Whatever the pass zeroes, overwrites or adds into, no
    element may keep or absorb what was there: no NaN, and both pre-fills give the same bits (entries no kernel writes, the
    resnet18.fc.* slots, read zero).  A default plan, whose atomics need the whole buffer zeroed, passes the same pre-fills NaN-free and
    agrees with itself to the summation-order round-off tests/test_gpu_bnfuse.py allows between two orders (1e-5 relative L2)."""
    res = _backward_forms({'deterministic': 1})
    for form in ('onehot', 'dense', 'phases'):
        z, n = res[form, 0], res[form, 0x7fc00000]
        assert not torch.isnan(n).any() and not torch.isnan(z).any(), form
        assert float(z.abs().max()) > 0
        assert torch.equal(z.view(torch.int32), n.view(torch.int32)), '%s: %d elements depend on the pre-fill' % (form, int((z != n).sum()))
    dflt = _backward_forms({})
    for form in ('onehot', 'dense', 'phases'):
        z, n = dflt[form, 0].double(), dflt[form, 0x7fc00000].double()
        assert not torch.isnan(n).any(), form
        assert float((z - n).norm() / z.norm()) < 1e-5, form
