"""numpy restatement of the reference's Q-map visualisation (utils.py:97-131), used by the visualisation tests.

The reference works in float32 throughout under numpy >= 2, where a python float that meets a float32 array or scalar becomes float32
first: ``scale_min_max`` subtracts the minimum of the WHOLE output and divides by (max - min) + 1e-6; ``to_uint8_image`` rounds 255 * x
half to even and casts to uint8; ``get_output_visualization`` blends (1 - alpha) * overhead + alpha * JET[k], the factor 1 - alpha formed
as a python float (a double) before it is rounded to float32.  Every function here writes those float32 roundings out explicitly, so it
gives the same bits under any numpy.  The colour map is an argument: the fixtures store the reference's table.
"""
import numpy as np

WIDTH = 96
F = np.float32


def image_width(n):
    return WIDTH + 1 + WIDTH * n + (n - 1)


def scale_min_max(image):
    """utils.py:100-101: one minimum and one maximum for all channels."""
    image = np.asarray(image, F)
    mn, mx = image.min(), image.max()
    d = F(F(mx - mn) + F(1e-6))
    return ((image - mn).astype(F) / d).astype(F)


def scaled_levels(image):
    """255 * scale_min_max(image) in float32, before the rounding of to_uint8_image."""
    return (F(255.0) * scale_min_max(image)).astype(F)


def to_uint8_image(image):
    """utils.py:97-98: np.round is half to even."""
    return np.round((F(255.0) * np.asarray(image, F)).astype(F)).astype(np.uint8)


def state_channels(C):
    """The state channels get_state_visualization (utils.py:103-108) shows as red, green, blue."""
    return (0, 0, 0) if C == 1 else ((1, 0, 0) if C == 2 else (1, 0, C - 1))


def state_visualization(state):
    return np.stack([state[:, :, c] for c in state_channels(state.shape[2])], axis=2)


def output_visualization(overhead, levels, jet, alpha=0.5):
    """utils.py:113-114 for one channel of uint8 levels; overhead: [96, 96, 3]."""
    a = (F(1 - alpha) * overhead).astype(F)
    b = (F(alpha) * jet[levels, :]).astype(F)
    return (a + b).astype(F)


def state_output_visualization(state, output, jet, alpha=0.5):
    """utils.py:116-131: [96, W, 3] float32."""
    state, output = np.asarray(state, F), np.asarray(output, F)
    bar = np.zeros((state.shape[1], 1, 3), F)
    overhead = np.stack([state[:, :, 0]] * 3, axis=2)
    levels = to_uint8_image(scale_min_max(output))
    panels = [state_visualization(state), bar]
    for q, channel in enumerate(levels):
        panels.append(output_visualization(overhead, channel, jet, alpha))
        if q < len(levels) - 1:
            panels.append(bar)
    return np.concatenate(panels, axis=1)


def near_tie_output(seed=5, top=3.7):
    """An output [1, 96, 96] with minimum 0 and maximum `top` in which, for every level k = 0 .. 254, the float32 neighbours of
    (k + 0.5) / 255 * d are planted wherever 255 * x lands within one ulp of k + 0.5 (on it included): the pixels at which half-even
    rounding, a division that is not correctly rounded, or a fused 255 * (v / d) would pick the neighbouring colour.  The rest is random."""
    rng = np.random.RandomState(seed)
    out = rng.uniform(0.0, top, (1, WIDTH, WIDTH)).astype(F)
    out[0, 0, 0], out[0, 0, 1] = 0.0, top
    d = F(F(F(top) - F(0.0)) + F(1e-6))
    planted = []
    for k in range(255):
        centre = F(np.float64(k + 0.5) / 255.0 * np.float64(d))
        v = centre
        for _ in range(3):
            v = np.nextafter(v, F(0.0))
        for _ in range(7):
            t = F(F(255.0) * F(v / d))
            if 0 < v < F(top) and abs(np.float64(t) - (k + 0.5)) <= np.float64(np.spacing(t)):
                planted.append(v)
            v = np.nextafter(v, F(np.inf))
    flat = out.reshape(-1)
    flat[2:2 + len(planted)] = np.asarray(planted, F)
    return out


def near_tie_count(output):
    """(pixels whose 255 * x lies within one ulp of some k + 0.5, pixels exactly on one with k even, with k odd)."""
    t = scaled_levels(output).astype(np.float64).reshape(-1)
    half = np.floor(t) + 0.5
    ulp = np.spacing(scaled_levels(output).reshape(-1)).astype(np.float64)
    near = np.abs(t - half) <= ulp
    exact = t == half
    k = np.floor(t).astype(np.int64)
    return int(near.sum()), int((exact & (k % 2 == 0)).sum()), int((exact & (k % 2 == 1)).sum())


def load_fixture(path):
    """tests/golden/visualization.npz -> (jet [256, 3], [{'name', 'state', 'output', 'alpha', 'want'}], numpy version of the writer)."""
    z = np.load(path)
    cases = [{'name': str(name), 'state': z['state_%d' % k], 'output': z['output_%d' % k], 'alpha': float(z['alpha'][k]),
              'want': z['panel_%d' % k]} for k, name in enumerate(z['names'])]
    return z['jet'], cases, str(z['numpy_version'])
