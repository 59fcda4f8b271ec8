"""Write tests/golden/visualization.npz: Q-map visualisations computed by the reference's own utils.py.

    python tools/gen_visualization_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and matplotlib (for its JET table).  utils.py is imported as it is, with empty stand-in modules for what it
imports but the visualisation code never touches (munch, prompt_toolkit, skimage, envs, policies); nothing of it is copied or kept.  The
expected images come from utils.get_state_output_visualization; the one case with alpha = 0.3, which that function cannot be asked
for, chains the reference's own get_state_visualization / get_overhead_image / scale_min_max / to_uint8_image /
get_output_visualization(alpha=0.3) in its order.  Every image is asserted equal, bit for bit, to tests/visualization_oracle.py before
anything is written.  The file holds arrays only: the reference's JET table, the (state, output, image) triples and the numpy version
that computed them (the bits hold for numpy >= 2, where a python float combined with a float32 array stays float32).
"""
import argparse
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import visualization_oracle as oracle                               # noqa: E402


def import_reference(ref):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def absent(*args, **kwargs):
        raise NotImplementedError('not part of the visualisation path')

    stub('munch', Munch=object)
    stub('prompt_toolkit')
    stub('prompt_toolkit.shortcuts', radiolist_dialog=absent)
    stub('skimage')
    stub('skimage.draw', circle_perimeter=absent)
    stub('envs', VectorEnv=object)
    stub('policies', DQNPolicy=object, DQNIntentionPolicy=object)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import utils
    return utils


def palette_state(rng, C, levels=16):
    """A [96, 96, C] state of values in [0, 1] and a few outside, drawn from a small palette in 8 x 8 blocks (so that the file compresses)."""
    palette = rng.uniform(-0.25, 1.25, levels).astype(np.float32)
    palette[:3] = (0.0, 1.0, 0.5)
    idx = rng.randint(0, levels, (12, 12, C))
    return palette[np.kron(idx, np.ones((8, 8, 1), np.int64))]


def smooth_output(rng, n, scale=1.0, levels=96):
    """A Q-map-like [n, 96, 96] output: low-frequency waves plus noise, quantised to a palette of fp32 values, negative ones included."""
    i, j = np.mgrid[0:96, 0:96] / 96.0
    out = np.stack([np.sin(2 * np.pi * (rng.uniform(0.5, 2) * i + rng.uniform(0.5, 2) * j + rng.uniform())) + 0.01 * rng.randn(96, 96) +
                    rng.uniform(-1, 1) for _ in range(n)])
    palette = np.sort(rng.uniform(out.min(), out.max(), levels)).astype(np.float32)
    return (scale * palette[np.clip(np.searchsorted(palette, out), 0, levels - 1)]).astype(np.float32)


def cases():
    rng = np.random.RandomState(14)
    yield 'c1_n1', palette_state(rng, 1), smooth_output(rng, 1), 0.5
    yield 'c2_n2', palette_state(rng, 2), smooth_output(rng, 2), 0.5
    yield 'c3_n3', palette_state(rng, 3), smooth_output(rng, 3, scale=37.5), 0.5
    yield 'c5_n4', palette_state(rng, 5), smooth_output(rng, 4, scale=1e-3), 0.5
    # train.py:300-303: the ground-truth intention (the state's last channel) over the predicted one
    s = palette_state(rng, 4)
    s[:, :, -1] = np.clip(s[:, :, -1], 0, 1)
    pred = np.clip(0.5 + 0.5 * smooth_output(rng, 1)[0], 0, 1).astype(np.float32)
    yield 'intention', s, np.stack((s[:, :, -1], pred), axis=0), 0.5
    yield 'constant', palette_state(rng, 3), np.full((2, 96, 96), 0.25, np.float32), 0.5
    out = smooth_output(rng, 3)
    out[1] *= np.float32(1000.0)
    yield 'dominant_channel', palette_state(rng, 3), out, 0.5
    yield 'near_tie', palette_state(rng, 1), oracle.near_tie_output(), 0.5
    yield 'alpha_0.3', palette_state(rng, 3), smooth_output(rng, 2), 0.3


def reference_image(utils, state, output, alpha):
    if alpha == 0.5:
        return utils.get_state_output_visualization(state, output)
    bar = np.zeros((state.shape[1], 1, 3), dtype=np.float32)
    panels = [utils.get_state_visualization(state), bar]
    overhead = utils.get_overhead_image(state)
    levels = utils.to_uint8_image(utils.scale_min_max(output))
    for q, channel in enumerate(levels):
        panels.append(utils.get_output_visualization(overhead, channel, alpha=alpha))
        if q < len(levels) - 1:
            panels.append(bar)
    return np.concatenate(panels, axis=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'visualization.npz'))
    args = ap.parse_args()
    assert int(np.__version__.split('.')[0]) >= 2, 'numpy >= 2: under numpy 1 the reference promotes its scalars to float64'
    utils = import_reference(os.path.abspath(args.reference))
    jet = utils.JET
    assert jet.dtype == np.float32 and jet.shape == (256, 3)
    arrays = {'jet': jet, 'numpy_version': np.asarray(np.__version__)}
    names, alphas = [], []
    for k, (name, state, output, alpha) in enumerate(cases()):
        want = reference_image(utils, state, output, alpha)
        got = oracle.state_output_visualization(state, output, jet, alpha)
        assert want.dtype == got.dtype == np.float32 and want.shape == got.shape == (96, oracle.image_width(len(output)), 3), (name, want.dtype)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), name
        assert np.array_equal(oracle.state_visualization(state), utils.get_state_visualization(state))
        assert np.array_equal(oracle.to_uint8_image(oracle.scale_min_max(output)), utils.to_uint8_image(utils.scale_min_max(output)))
        arrays['state_%d' % k], arrays['output_%d' % k], arrays['panel_%d' % k] = state, output, np.ascontiguousarray(want)
        names.append(name)
        alphas.append(alpha)
    arrays['names'], arrays['alpha'] = np.asarray(names), np.asarray(alphas, np.float64)
    np.savez_compressed(args.out, **arrays)
    near = oracle.near_tie_count(oracle.near_tie_output())
    print('%s: %d triples, %d bytes (numpy %s); near_tie: %d pixels within an ulp of k + 0.5, %d / %d exactly on an even / odd one'
          % (args.out, len(names), os.path.getsize(args.out), np.__version__, *near))
    assert os.path.getsize(args.out) < 1 << 20


if __name__ == '__main__':
    main()
