"""GPU: simq_state_output_visualizations / simq.state_output_visualizations against the reference's own images
(tests/golden/visualization.npz) and the numpy oracle (tests/visualization_oracle.py), bit for bit (compared as uint32 bit patterns)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import visualization_oracle as oracle

pytestmark = pytest.mark.gpu

SENTINEL = 123.0
FAMILY = b'state_output_visualization'


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return oracle.load_fixture(os.path.join(golden_dir, 'visualization.npz'))


@pytest.fixture(scope='module')
def grid(fixture):
    """Random (state, output) pairs for C in {1, 2, 3, 5} x n in {1, 2, 3, 4} with the oracle's images at alpha 0.5 and 0.3, computed once."""
    jet = fixture[0]
    rng = np.random.RandomState(31)
    cases = []
    for C in (1, 2, 3, 5):
        for n in (1, 2, 3, 4):
            state = rng.uniform(-0.25, 1.25, (96, 96, C)).astype(np.float32)
            output = (rng.randn(n, 96, 96) * 10.0 ** rng.randint(-2, 3) + rng.uniform(-3, 3)).astype(np.float32)
            cases.append({'C': C, 'n': n, 'state': state, 'output': output,
                          0.5: oracle.state_output_visualization(state, output, jet, 0.5),
                          0.3: oracle.state_output_visualization(state, output, jet, 0.3)})
    return cases


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_image_equal(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), '%s: %d of %d floats differ, first at %s' % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist())


def test_every_fixture_through_the_python_interface(simq_mod, fixture):
    jet, cases, _ = fixture
    for c in cases:
        got = simq_mod.state_output_visualizations([c['state']], [c['output']], jet=jet, alpha=c['alpha'])
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1,) + c['want'].shape
        assert_image_equal(got[0], c['want'], c['name'])
    half = [c for c in cases if c['alpha'] == 0.5]                                     # ... and all of one alpha in one mixed launch
    got = simq_mod.state_output_visualizations([c['state'] for c in half], [c['output'] for c in half], jet=jet)
    assert isinstance(got, list) and len(got) == len(half)
    for g, c in zip(got, half):
        assert_image_equal(g, c['want'], 'mixed ' + c['name'])


def test_constant_output_is_jet_zero_and_scaling_is_global(simq_mod, fixture):
    jet, cases, _ = fixture
    by_name = {c['name']: c for c in cases}
    c = by_name['constant']                        # max == min: every output pixel is JET[0] blended over the overhead channel
    got = simq_mod.state_output_visualizations([c['state']], [c['output']], jet=jet)[0].cpu().numpy()
    blend = np.float32(0.5) * c['state'][:, :, :1] + np.float32(0.5) * jet[0][None, None, :]
    for q in range(2):
        assert_image_equal(got[:, 97 + 97 * q:97 + 97 * q + 96], blend, 'constant panel %d' % q)
    assert not got[:, 96].any() and not got[:, 193].any() and got.shape[1] == 290
    d = by_name['dominant_channel']                # one channel 1000 times the others: one minimum and one maximum for all three
    got = simq_mod.state_output_visualizations([d['state']], [d['output']], jet=jet)[0]
    assert_image_equal(got, d['want'], 'dominant channel')
    per_channel = np.concatenate([oracle.state_output_visualization(d['state'], d['output'][q:q + 1], jet)[:, 97:] for q in range(3)], axis=1)
    assert (bits(per_channel) != bits(np.delete(d['want'][:, 97:], [96, 193], axis=1))).mean() > 0.2


def test_grid_of_channel_counts_through_python_and_the_c_abi(simq_mod, fixture, grid):
    from simq import _lib
    from simq.visualization import VisualizationProblem
    jet = fixture[0]
    got = simq_mod.state_output_visualizations([c['state'] for c in grid], [c['output'] for c in grid], jet=jet)
    for g, c in zip(got, grid):
        assert tuple(g.shape) == (96, oracle.image_width(c['n']), 3)
        assert_image_equal(g, c[0.5], 'C = %d, n = %d' % (c['C'], c['n']))
    # the same 16 problems through the raw C-ABI, images packed back to front with a gap between them
    states = [torch.from_numpy(c['state']).cuda() for c in grid]
    outputs = [torch.from_numpy(c['output']).cuda() for c in grid]
    d_jet = torch.from_numpy(jet).cuda()
    sizes = [c[0.5].size for c in grid]
    offsets, at = [], 0
    for s in reversed(sizes):
        offsets.insert(0, at)
        at += s + 5
    out = torch.full((at,), SENTINEL, device='cuda')
    probs = (VisualizationProblem * len(grid))(*[VisualizationProblem(s.data_ptr(), o.data_ptr(), off, c['n'], c['C'])
                                                  for s, o, off, c in zip(states, outputs, offsets, grid)])
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device='cuda')
    _lib.lib.c.simq_launch_counts_reset()
    _lib.lib.call('simq_state_output_visualizations', probs, len(grid), _lib.ptr(d_probs), _lib.ptr(d_jet), 0.5, 0, _lib.ptr(out),
                  ctypes.c_int64(out.numel()), _lib.stream_ptr())
    assert _lib.lib.c.simq_launch_count(FAMILY) == 1 and _lib.launch_counts() == {FAMILY.decode(): 1}
    host = out.cpu().numpy()
    for off, size, c in zip(offsets, sizes, grid):
        assert_image_equal(host[off:off + size].reshape(c[0.5].shape), c[0.5], 'C-ABI C = %d, n = %d' % (c['C'], c['n']))
        assert (host[off + size:off + size + 5] == SENTINEL).all()


def test_uniform_batches_return_one_tensor_and_p_equals_one(simq_mod, fixture, grid):
    jet = fixture[0]
    for n in (1, 4):
        sel = [c for c in grid if c['n'] == n and c['C'] == 3] * 2
        states = torch.from_numpy(np.stack([c['state'] for c in sel])).cuda()
        outputs = torch.from_numpy(np.stack([c['output'] for c in sel])).cuda()
        got = simq_mod.state_output_visualizations(states, outputs, jet=jet)
        assert isinstance(got, torch.Tensor) and tuple(got.shape) == (2, 96, oracle.image_width(n), 3)
        for p in range(2):
            assert_image_equal(got[p], sel[p][0.5], 'batch n = %d row %d' % (n, p))
    one = grid[6]
    got = simq_mod.state_output_visualizations(one['state'][None], one['output'][None], jet=jet)
    assert tuple(got.shape) == (1,) + one[0.5].shape
    assert_image_equal(got[0], one[0.5], 'P = 1')


def test_mixed_launch_of_forty_problems(simq_mod, fixture, grid):
    """40 problems in one launch, every (C, n) of the grid in a shuffled order and alpha = 0.3, states and outputs already on the device,
    into a caller's buffer."""
    jet = fixture[0]
    order = [grid[(7 * k) % 16] for k in range(40)]
    states = [torch.from_numpy(c['state']).cuda() for c in order]
    outputs = [torch.from_numpy(c['output']).cuda() for c in order]
    total = sum(c[0.3].size for c in order)
    buf = torch.full((total + 7,), SENTINEL, device='cuda')
    got = simq_mod.state_output_visualizations(states, outputs, jet=torch.from_numpy(jet).cuda(), alpha=0.3, out=buf)
    assert len(got) == 40 and got[0].data_ptr() == buf.data_ptr()
    for k, (g, c) in enumerate(zip(got, order)):
        assert_image_equal(g, c[0.3], 'problem %d (C = %d, n = %d)' % (k, c['C'], c['n']))
    assert bool((buf[total:] == SENTINEL).all())


def test_chw_is_the_transpose(simq_mod, fixture, grid):
    jet = fixture[0]
    sel = [grid[1], grid[11], grid[12], grid[6]]
    for alpha in (0.5, 0.3):
        got = simq_mod.state_output_visualizations([c['state'] for c in sel], [c['output'] for c in sel], jet=jet, alpha=alpha, chw=True)
        for g, c in zip(got, sel):
            assert tuple(g.shape) == (3, 96, oracle.image_width(c['n']))
            assert_image_equal(g, c[alpha].transpose(2, 0, 1), 'chw C = %d, n = %d, alpha = %s' % (c['C'], c['n'], alpha))
    both = [c for c in grid if c['n'] == 2 and c['C'] in (2, 3)]
    got = simq_mod.state_output_visualizations(np.stack([c['state'][:, :, :2] for c in both]), np.stack([c['output'] for c in both]), jet=jet,
                                               chw=True)
    assert tuple(got.shape) == (2, 3, 96, 290)
    assert_image_equal(got[0], both[0][0.5].transpose(2, 0, 1), 'chw batch')


def test_near_ties_pin_half_even_rounding_and_the_true_division(simq_mod, fixture):
    jet, cases, _ = fixture
    case = {c['name']: c for c in cases}['near_tie']
    near, even, odd = oracle.near_tie_count(case['output'])
    print('near ties %d, exact on even k %d, exact on odd k %d' % (near, even, odd))
    assert near >= 100 and even >= 10 and odd >= 10
    for alpha in (0.5, 0.3):
        want = case['want'] if alpha == 0.5 else oracle.state_output_visualization(case['state'], case['output'], jet, alpha)
        got = simq_mod.state_output_visualizations([case['state']], [case['output']], jet=jet, alpha=alpha)
        assert_image_equal(got[0], want, 'near ties, alpha = %s' % alpha)


def test_alpha_point_three_catches_a_fused_blend(simq_mod, fixture, grid):
    """At alpha = 0.5 both products of the blend are exact, so a fused multiply-add gives the same bits; at 0.3 it does not: the oracle's
    image differs from the fused evaluation at many pixels, and the kernel equals the oracle."""
    jet = fixture[0]
    c = grid[9]
    state, output = c['state'], c['output']
    levels = oracle.to_uint8_image(oracle.scale_min_max(output))
    a = np.float64(np.float32(1 - 0.3)) * state[:, :, :1].astype(np.float64)
    fused = (np.float64(np.float32(0.3)) * jet[levels[0]].astype(np.float64) + a.astype(np.float32).astype(np.float64)).astype(np.float32)
    assert (bits(fused) != bits(c[0.3][:, 97:193])).sum() >= 100
    got = simq_mod.state_output_visualizations([state], [output], jet=jet, alpha=0.3)
    assert_image_equal(got[0], c[0.3], 'alpha = 0.3')
    case = {x['name']: x for x in fixture[1]}['alpha_0.3']
    got = simq_mod.state_output_visualizations([case['state']], [case['output']], jet=jet, alpha=0.3)
    assert_image_equal(got[0], case['want'], 'the reference at alpha = 0.3')


def test_ring_states_and_network_outputs_where_they_lie(simq_mod, fixture):
    """States read in place from DeviceReplayBuffer.states, Q-maps from the network: infer_argmax_batch(need_q=True) returns them on the
    host (its contract), forward_nhwc leaves them in HBM; neither path copies a state to the host, and both give the oracle's image."""
    from simq import synth
    from oracle import fcn as ofcn
    jet = fixture[0]
    rng = np.random.RandomState(8)
    ring = simq_mod.DeviceReplayBuffer(8, 4)
    host_states = rng.uniform(0, 1, (5, 96, 96, 4)).astype(np.float32)
    ring.push_many(host_states, [0] * 5, [0.0] * 5, host_states, [False] * 5)
    torch.cuda.synchronize()
    net = simq_mod.FCN(4, 2)
    net.load_state_dict(ofcn.state_from_numpy(synth.make_state_dict(4, 2, 2)))
    net.eval()
    sel = (1, 3, 4)
    _, qmaps = net.infer_argmax_batch([ring.states[k:k + 1] for k in sel], need_q=True)
    q_dev = net.forward_nhwc(ring.states[1:5])
    assert q_dev.is_cuda and tuple(q_dev.shape) == (4, 2, 96, 96)
    got = simq_mod.state_output_visualizations([ring.states[k] for k in sel], qmaps, jet=jet)
    in_place = simq_mod.state_output_visualizations([ring.states[k] for k in sel], [q_dev[k - 1] for k in sel], jet=jet, chw=True)
    assert tuple(got.shape) == (3, 96, 290, 3) and tuple(in_place.shape) == (3, 3, 96, 290)
    q_host = q_dev.cpu().numpy()                   # (the batch of 4 may round its sums in another order than the batch of 3: its own oracle)
    assert np.isfinite(q_host).all() and np.ptp(q_host) > 0
    for p, k in enumerate(sel):
        assert_image_equal(got[p], oracle.state_output_visualization(host_states[k], qmaps[p], jet), 'ring state %d, host Q-map' % k)
        assert_image_equal(in_place[p], oracle.state_output_visualization(host_states[k], q_host[k - 1], jet).transpose(2, 0, 1),
                           'ring state %d, device Q-map' % k)
    # the intention image of train.py:300-303: the state's last channel over a prediction
    pred = rng.uniform(0, 1, (96, 96)).astype(np.float32)
    stacked = torch.stack((ring.states[3][:, :, -1], torch.from_numpy(pred).cuda()))
    got = simq_mod.state_output_visualizations([ring.states[3]], [stacked], jet=jet)
    assert_image_equal(got[0], oracle.state_output_visualization(host_states[3], np.stack((host_states[3][:, :, -1], pred)), jet), 'intention')
    assert_image_equal(ring.states[:5], host_states, 'the ring is untouched')


def test_drop_ins_and_the_default_table(simq_mod, fixture):
    from simq import _lib
    jet, cases, _ = fixture
    c = {x['name']: x for x in cases}['c3_n3']
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        with pytest.raises(_lib.SimqError, match='matplotlib'):
            simq_mod.state_output_visualization(c['state'], c['output'])
        return
    got = simq_mod.state_output_visualization(c['state'], c['output'])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert_image_equal(got, c['want'], 'drop-in')
    for x in cases[:5]:
        panel = simq_mod.state_visualization(x['state'])
        assert isinstance(panel, np.ndarray) and panel.shape == (96, 96, 3)
        assert_image_equal(panel, oracle.state_visualization(x['state']), 'state panel ' + x['name'])
        assert_image_equal(panel, x['want'][:, :96], 'state panel of the reference ' + x['name'])


def test_refusals_launch_nothing_and_leave_a_message(simq_mod, fixture, grid):
    from simq import _lib
    from simq.visualization import VisualizationProblem
    jet = torch.from_numpy(fixture[0]).cuda()
    c = grid[5]                                    # C = 2, n = 2
    state, output = torch.from_numpy(c['state']).cuda(), torch.from_numpy(c['output']).cuda()
    size = c[0.5].size
    out = torch.full((size + 4,), SENTINEL, device='cuda')
    d_probs = torch.empty(64, dtype=torch.uint8, device='cuda')

    def refused(match, problem=None, out_ptr=None, out_floats=None, jet_ptr=None):
        p = problem or VisualizationProblem(state.data_ptr(), output.data_ptr(), 0, 2, 2)
        _lib.lib.c.simq_launch_counts_reset()
        rc = _lib.lib.c.simq_state_output_visualizations(ctypes.byref(p), 1, _lib.ptr(d_probs), jet_ptr or _lib.ptr(jet), 0.5, 0,
                                                         out_ptr or _lib.ptr(out), size if out_floats is None else out_floats, _lib.stream_ptr())
        assert rc == -1 and match in _lib.last_error(), (match, rc, _lib.last_error())
        torch.cuda.synchronize()
        assert _lib.lib.c.simq_launch_count(FAMILY) == 0 and bool((out == SENTINEL).all())

    refused('n = 0', VisualizationProblem(state.data_ptr(), output.data_ptr(), 0, 0, 2))
    refused('n = 5', VisualizationProblem(state.data_ptr(), output.data_ptr(), 0, 5, 2))
    refused('outside', out_floats=size - 1)                                                        # a short out
    refused('aligned', VisualizationProblem(state.data_ptr() + 2, output.data_ptr(), 0, 2, 2))     # a misaligned pointer
    refused('aligned', out_ptr=ctypes.c_void_p(out.data_ptr() + 1))
    # out over an input: the output, the state, the table
    both = torch.full((size + 2 * 9216,), SENTINEL, device='cuda')
    for what, p, o in (('output', VisualizationProblem(state.data_ptr(), both[size - 1:].data_ptr(), 0, 2, 2), both),
                       ('state', VisualizationProblem(both[100:].data_ptr(), output.data_ptr(), 0, 2, 2), both)):
        _lib.lib.c.simq_launch_counts_reset()
        rc = _lib.lib.c.simq_state_output_visualizations(ctypes.byref(p), 1, _lib.ptr(d_probs), _lib.ptr(jet), 0.5, 0, _lib.ptr(o), size,
                                                         _lib.stream_ptr())
        assert rc == -1 and 'overlaps' in _lib.last_error(), (what, _lib.last_error())
        torch.cuda.synchronize()
        assert _lib.lib.c.simq_launch_count(FAMILY) == 0 and bool((both == SENTINEL).all())
    refused('d_jet', jet_ptr=ctypes.c_void_p(out.data_ptr() + 64))
    # through Python: the message arrives as a SimqError; shapes the library never sees are ValueErrors
    _lib.lib.c.simq_launch_counts_reset()
    with pytest.raises(_lib.SimqError, match='overlaps'):
        simq_mod.state_output_visualizations([both[:9216 * 2].view(96, 96, 2)], [output], jet=jet, out=both)
    with pytest.raises(ValueError, match='1 <= n <= 4'):
        simq_mod.state_output_visualizations([state], [torch.zeros(5, 96, 96, device='cuda')], jet=jet)
    with pytest.raises(ValueError, match='1 <= n <= 4'):
        simq_mod.state_output_visualizations([state], [torch.zeros(0, 96, 96, device='cuda')], jet=jet)
    with pytest.raises(ValueError, match='contiguous'):
        simq_mod.state_output_visualizations([torch.zeros(96, 96, 4, device='cuda')[:, :, :2]], [output], jet=jet)
    with pytest.raises(ValueError, match='at least'):
        simq_mod.state_output_visualizations([state], [output], jet=jet, out=out[:size - 1])
    torch.cuda.synchronize()
    assert _lib.lib.c.simq_launch_count(FAMILY) == 0
    # the library still works afterwards
    got = simq_mod.state_output_visualizations([state], [output], jet=jet, out=out)
    assert_image_equal(got[0], c[0.5], 'after the refusals')
    assert _lib.lib.c.simq_launch_count(FAMILY) == 1 and bool((out[size:] == SENTINEL).all())
