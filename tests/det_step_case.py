"""One deterministic fp32 TD step from seeded weights and a seeded batch, reduced to what tests/golden/det_step_parent.npz pins
(tools/gen_det_step_golden.py writes it, tests/test_gpu_det_forms.py compares): the reported loss and TD error, the last layer's
gradients in full, 4096 seeded elements of the gradient buffer, SHA-256 of the gradient buffer and of the updated parameters."""
import hashlib

import numpy as np
import torch

SHAPES = [(4, 2, 5), (4, 2, 32), (5, 1, 6)]          # (num_input_channels, num_output_channels, transitions)
WEIGHT_SEED, BATCH_SEED, PICK_SEED, PICKS = 3, 7, 11, 4096


def key(cin, cout, batch):
    return 'c%do%d_b%d' % (cin, cout, batch)


def tensor_range(plan, name):
    for n, off, shape, _ in plan.tensors:
        if n == name or n.endswith('.' + name):
            return off, off + int(np.prod(shape))
    raise KeyError(name)


def run(cin, cout, batch, options=None):
    """{name: numpy array} of one step on the current GPU; options: simq_plan_options on top of deterministic = 1."""
    import simq
    import simq.learner as sl
    from oracle import cases, fcn as ofcn
    from simq import synth
    opts = dict({'deterministic': 1}, **(options or {}))
    policy = simq.FCN(cin, cout, precision='fp32', options=opts)
    target = simq.FCN(cin, cout, precision='fp32', options=opts)
    policy.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, WEIGHT_SEED)))
    target.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(cin, cout, WEIGHT_SEED + 1)))
    policy.train(); target.eval()
    b = cases.make_batch(cin, cout, batch, BATCH_SEED)
    info = sl.train_step(policy, target, b, cases.GAMMA, batch, cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY, cases.CLIP, use_double_dqn=True)
    torch.cuda.synchronize()
    assert policy.plan.options['deterministic'] == 1
    g = policy.flat_grads.detach().cpu().numpy()
    w = policy.flat_params.detach().cpu().numpy()
    w0, w1 = tensor_range(policy.plan, 'conv3.weight')                      # the last layer (networks.py:14)
    b0, b1 = tensor_range(policy.plan, 'conv3.bias')
    assert w1 - w0 == cout * 32 and b1 - b0 == cout
    pick = np.random.RandomState(PICK_SEED).randint(0, g.size, PICKS)
    return {'loss': np.float64(info['loss']), 'td_error': np.float64(info['td_error']), 'dw3': g[w0:w1].copy(), 'db3': g[b0:b1].copy(),
            'picked': g[pick].copy(), 'grad_sha256': np.frombuffer(hashlib.sha256(g.tobytes()).digest(), np.uint8).copy(),
            'param_sha256': np.frombuffer(hashlib.sha256(w.tobytes()).digest(), np.uint8).copy()}
