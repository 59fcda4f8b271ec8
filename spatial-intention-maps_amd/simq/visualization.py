"""Q-map visualisations on the GPU: the state and output panels of the reference's ``utils.get_state_output_visualization``.

The reference's training loop (train.py:292-304) takes a random replay state and the Q-map ``policy.step(..., debug=True)`` returned, and
draws, with numpy on the host, one image per robot group for tensorboard: the state as an RGB panel, then every channel of the output
scaled to [0, 1] over the whole output, quantised to 256 levels, coloured with matplotlib's jet map and blended over the state's overhead
channel (utils.py:97-131); ``enjoy.py --debug`` does the same on every step.  ``simq_state_output_visualizations``
(csrc/visualization.hip) draws the images of many (state, output) pairs in one launch, bit for bit equal to that sequence under
numpy >= 2, reading the states where they lie (a batch row, a slice of ``DeviceReplayBuffer.states``) and the outputs where the network
left them (``FCN.forward_nhwc``).  The colour map is the caller's: ``jet_table`` builds the reference's from matplotlib.
"""
import ctypes

import numpy as np
import torch

from . import _batch
from ._lib import SimqError, lib, ptr, stream_ptr

WIDTH = 96                       # Mapper.LOCAL_MAP_PIXEL_WIDTH (envs.py:2010)
MAX_OUTPUTS = 4                  # SIMQ_VISUALIZATION_MAX_OUTPUTS
MAX_CHANNELS = 64                # SIMQ_LOCAL_MAX_CHANNELS


class VisualizationProblem(ctypes.Structure):
    """simq_visualization_problem of include/simq.h."""
    _fields_ = [('d_state', ctypes.c_void_p), ('d_output', ctypes.c_void_p), ('out_offset', ctypes.c_int64), ('n', ctypes.c_int32),
                ('channels', ctypes.c_int32)]


def image_width(n):
    """Columns of the image of an output with n channels: the state panel, a bar, n panels with a bar between two of them."""
    return WIDTH + 1 + WIDTH * n + (n - 1)


def jet_table():
    """The reference's colour map (utils.py:95): the RGB of matplotlib's jet at its 256 levels, float32 [256, 3]."""
    try:
        from matplotlib import cm
    except ImportError as e:
        raise SimqError('simq.jet_table takes the colour map from matplotlib.cm.jet, as the reference\'s utils.JET does, and matplotlib is '
                        'not importable here (%s); pass jet= a float32 [256, 3] table of your own' % e) from None
    return np.ascontiguousarray(cm.jet(np.arange(256))[:, :3], dtype=np.float32)


_JET = {}                        # device -> the reference's table there (uploaded once)


def _on_device(x, dev, what, rank):
    """A contiguous float32 tensor on `dev`: a device tensor as it is (read in place), anything on the host uploaded."""
    if hasattr(x, 'device_row'):                 # an observation of a replay ring (a record's state, a pool handle): its row, in place
        x = x.device_row()
        if x.dtype == torch.bfloat16:            # a ring of bf16 states: widened exactly (simq_states_to_f32), then everything as for fp32 --
            from .fcn import to_f32              # the panels are the fp32 panels of the rounded state
            x = to_f32(x.contiguous())
    if isinstance(x, np.ndarray):
        if x.dtype != np.float32:
            raise ValueError('%s must be float32, got %s' % (what, x.dtype))
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != rank:
        raise ValueError('%s must be a %d-D float32 numpy array or tensor, got %s' % (
            what, rank, '%s %s' % (x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__))
    if x.device != dev:
        x = x.to(dev)
    if not x.is_contiguous():
        raise ValueError('%s must be contiguous (it is read in place), got strides %s for shape %s' % (what, x.stride(), tuple(x.shape)))
    return x


def _rows(x, dev, what, rank):
    """The problems of one argument: a [P, ...] tensor / array is P rows of it, a list is taken item by item."""
    if isinstance(x, (np.ndarray, torch.Tensor)):
        x = _on_device(x, dev, what, rank + 1)
        return [x[k] for k in range(x.shape[0])]
    return [_on_device(v, dev, '%s[%d]' % (what, k), rank) for k, v in enumerate(x)]


def _jet_on(jet, dev):
    if jet is None:
        if dev not in _JET:
            _JET[dev] = torch.from_numpy(jet_table()).to(dev)
        return _JET[dev]
    jet = _on_device(jet, dev, 'jet', 2)
    if tuple(jet.shape) != (256, 3):
        raise ValueError('jet must be a [256, 3] table, got %s' % (tuple(jet.shape),))
    return jet


def _prepare(states, outputs, jet, alpha, chw, out):
    """The argument tuple of simq_state_output_visualizations, the images it will hold and the device tensors the call reads
    (tools/visualization_rate.py times the library call alone with it)."""
    dev = _batch.device('visualisations')
    states = _rows(states, dev, 'states', 3)
    outputs = _rows(outputs, dev, 'outputs', 3)
    P = len(states)
    if P < 1 or len(outputs) != P:
        raise ValueError('%d states for %d outputs (at least one pair)' % (P, len(outputs)))
    probs = (VisualizationProblem * P)()
    shapes, offset = [], 0
    for p, (s, o) in enumerate(zip(states, outputs)):
        if tuple(s.shape[:2]) != (WIDTH, WIDTH) or not 1 <= s.shape[2] <= MAX_CHANNELS:
            raise ValueError('states[%d] must be [96, 96, C] with 1 <= C <= %d, got %s' % (p, MAX_CHANNELS, tuple(s.shape)))
        if tuple(o.shape[1:]) != (WIDTH, WIDTH) or not 1 <= o.shape[0] <= MAX_OUTPUTS:
            raise ValueError('outputs[%d] must be [n, 96, 96] with 1 <= n <= %d, got %s' % (p, MAX_OUTPUTS, tuple(o.shape)))
        n = o.shape[0]
        probs[p] = VisualizationProblem(s.data_ptr(), o.data_ptr(), offset, n, s.shape[2])
        shapes.append((3, WIDTH, image_width(n)) if chw else (WIDTH, image_width(n), 3))
        offset += 3 * WIDTH * image_width(n)
    uniform = all(sh == shapes[0] for sh in shapes)
    if out is None:
        out = torch.empty(offset, dtype=torch.float32, device=dev)
    elif not _batch.out_fits(out, torch.float32, dev, at_least=offset):
        raise ValueError('out must be a contiguous float32 tensor of at least %d elements on %s' % (offset, dev))
    flat = out.view(-1)
    result = flat[:offset].view((P,) + shapes[0]) if uniform else _batch.views(flat, shapes)
    jet = _jet_on(jet, dev)
    d_probs = torch.empty(ctypes.sizeof(VisualizationProblem) * P, dtype=torch.uint8, device=dev)
    args = (probs, P, ptr(d_probs), ptr(jet), ctypes.c_double(float(alpha)), int(bool(chw)), ptr(out), ctypes.c_int64(out.numel()),
            stream_ptr(dev))
    return args, result, (states, outputs, jet, d_probs, out)


def state_output_visualizations(states, outputs, jet=None, alpha=0.5, chw=False, out=None):
    """utils.get_state_output_visualization (utils.py:116-131) of P (state, output) pairs in one launch.

    states: a [P, 96, 96, C] float32 tensor / array, or a list of P [96, 96, C] ones (C may differ between them).  Device tensors are
    read in place -- a batch, ``ring.states[k]`` of a DeviceReplayBuffer -- and must be contiguous; host arrays are uploaded.  An item
    of the list may also be an observation of a replay ring (``record.state``, a handle of ``reserve`` / ``adopt``): its row, in place.
    outputs: a [P, n, 96, 96] float32 tensor / array, or a list of P [n, 96, 96] ones, 1 <= n <= 4: the Q-maps ``FCN.forward_nhwc``
    returned (device, read in place), ``info['output'][i][j]`` of ``policy.step(debug=True)`` (host, uploaded), or the stacked ground
    truth and predicted intention of train.py:300-303.
    jet: the float32 [256, 3] colour map; None: the reference's (jet_table(), uploaded once per device).  alpha: the weight of the colour
    in the blend (utils.py:113-114; the reference always draws with 0.5).  chw: images as [3, 96, W], the transpose((2, 0, 1)) of
    train.py:297 that SummaryWriter.add_image takes.
    out: a contiguous float32 device tensor of at least the images' total size to write into.

    Returns a device tensor [P, 96, W, 3] (chw: [P, 3, 96, W]), W = 96 + 1 + 96 n + (n - 1), when every output has the same n, else a list
    of P such images, views of one buffer.  Bit for bit what the reference computes under numpy >= 2 for finite outputs."""
    args, result, keep = _prepare(states, outputs, jet, alpha, chw, out)
    lib.call('simq_state_output_visualizations', *args)
    del keep                                     # (uploaded inputs / descriptors: alive until the launch is queued)
    if not isinstance(states, (np.ndarray, torch.Tensor)):
        for pool in {id(v.pool): v.pool for v in states if getattr(v, 'pool', None) is not None}.values():
            pool.note_read()                     # (a pool slot read in place: whoever rewrites it once it is released waits for this launch)
    return result


def state_output_visualization(state, output):
    """Drop-in for utils.get_state_output_visualization (utils.py:116-131): the float32 [96, W, 3] numpy image of one state [96, 96, C]
    and one output [n, 96, 96] (numpy, or device tensors read in place)."""
    return state_output_visualizations([state], [output])[0].cpu().numpy()


def state_visualization(state):
    """Drop-in for utils.get_state_visualization (utils.py:103-108): the float32 [96, 96, 3] numpy panel of one state -- the first 96
    columns of the image the kernel draws for it (with an output of zeros)."""
    dev = _batch.device('visualisations')
    image = state_output_visualizations([state], [torch.zeros((1, WIDTH, WIDTH), dtype=torch.float32, device=dev)])
    return np.ascontiguousarray(image[0, :, :WIDTH].cpu().numpy())
