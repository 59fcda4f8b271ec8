"""What the wrappers of the batched map operators share (grid_paths, grid_queries, waypoints, occupancy, observation, local_maps, intention_drawing,
visualization): the device, the argument checks, the packed upload, the `out` check and the status read-back.  Nothing here knows an
operator: the helpers check and report, the operators word their own errors."""
import numpy as np
import torch

from ._lib import SimqError


def device(what):
    """The current device; `what` is the operator's plural noun ('occupancy maps').  The operators call it after their argument
    checks, which need no device."""
    if not torch.cuda.is_available():
        raise SimqError('simq %s need an MI355X (torch.cuda.is_available() is False); no CPU path' % what)
    return torch.device('cuda', torch.cuda.current_device())


def check_grid(grid, what='grid'):
    """A 2-D C-contiguous uint8 array, as the reference's `unsigned char[:, ::1]` (numpy), or a contiguous uint8 torch tensor."""
    if isinstance(grid, torch.Tensor):
        if grid.dtype != torch.uint8 or grid.dim() != 2 or not grid.is_contiguous():
            raise ValueError('%s must be a 2-D contiguous uint8 tensor, got %s %s' % (what, grid.dtype, tuple(grid.shape)))
        return grid
    if not isinstance(grid, np.ndarray) or grid.dtype != np.uint8 or grid.ndim != 2 or not grid.flags['C_CONTIGUOUS']:
        desc = ('%s %s%s' % (grid.dtype, grid.shape, '' if grid.flags['C_CONTIGUOUS'] else ' non-contiguous')
                if isinstance(grid, np.ndarray) else type(grid).__name__)
        raise ValueError('%s must be a 2-D C-contiguous uint8 numpy array (unsigned char[:, ::1]), got %s' % (what, desc))
    return grid


def check_map(m, what, dtype=np.float32):
    """A 2-D array of the numpy type `dtype` (made C-contiguous here) or a contiguous tensor of that type."""
    if isinstance(m, torch.Tensor):
        if m.dtype != getattr(torch, dtype.__name__) or m.dim() != 2 or not m.is_contiguous():
            raise ValueError('%s must be a 2-D contiguous %s tensor, got %s %s' % (what, dtype.__name__, m.dtype, tuple(m.shape)))
        return m
    if not isinstance(m, np.ndarray) or m.dtype != dtype or m.ndim != 2:
        raise ValueError('%s must be a 2-D %s numpy array or tensor, got %s' % (
            what, dtype.__name__, '%s %s' % (m.dtype, m.shape) if isinstance(m, np.ndarray) else type(m).__name__))
    return np.ascontiguousarray(m)


def as_maps(maps, what, check=check_grid, expects=None):
    """The 2-D maps of a sequence or of one [G, rows, cols] array / tensor, each passed through check(map, 'what[k]'), and that array
    itself when it is one contiguous block (`pack` uploads it with one copy instead of G), else None.  expects: the operator's words for
    what it takes ('a sequence of 2-D uint8 maps or one [G, rows, cols] array'); with it an array of another rank and an argument that
    is no sequence are a ValueError in those words."""
    whole = None
    if isinstance(maps, (np.ndarray, torch.Tensor)):
        if maps.ndim == 3:
            if maps.is_contiguous() if isinstance(maps, torch.Tensor) else maps.flags['C_CONTIGUOUS']:
                whole = maps
        elif expects is not None:
            raise ValueError('%s is %s, got %d dimensions' % (what, expects, maps.ndim))
    try:
        maps = list(maps)
    except TypeError:
        if expects is None:
            raise
        raise ValueError('%s is %s, got %s' % (what, expects, type(maps).__name__)) from None
    return [check(m, '%s[%d]' % (what, k)) for k, m in enumerate(maps)], whole


def problem_index(index, n_items, n_problems, unequal, out_of_range):
    """The item (grid, room mask, map) of every problem as a list of ints: `index`, or problem p -> item p when it is None.  The two
    messages are the caller's: `unequal` for no index with other than one item per problem, `out_of_range` for a wrong length or entry."""
    if index is None:
        if n_items != n_problems:
            raise ValueError(unequal)
        index = range(n_problems)
    index = [int(k) for k in index]
    if len(index) != n_problems or any(k < 0 or k >= n_items for k in index):
        raise ValueError(out_of_range)
    return index


def pack(arrays, dtype, dev, align=1):
    """One device buffer of `dtype` holding `arrays` (numpy arrays or tensors of any shape, of `dtype` or of another type of its element
    size, whose bits are kept) one behind the other, each at a multiple of `align` elements, and the list of their element offsets.

    The host arrays go through one staging array that covers their span; the arrays that are on `dev` already are written with a
    device copy each AFTER it, because the span may cover them.  When none is on the host nothing of the host is touched: no staging
    array, no torch.from_numpy.  With align > 1 the padding reads as zero (and the buffer is never empty)."""
    offsets, total = [], 0
    for a in arrays:
        offsets.append(total)
        total += (_size(a) + align - 1) // align * align
    buf = torch.zeros(max(total, 1), dtype=dtype, device=dev) if align > 1 else torch.empty(total, dtype=dtype, device=dev)
    on_dev = [isinstance(a, torch.Tensor) and a.device == dev for a in arrays]
    host = [(o, a.cpu().numpy() if isinstance(a, torch.Tensor) else a) for o, a, d in zip(offsets, arrays, on_dev) if not d]
    if host:
        np_dtype = _NUMPY[dtype]
        lo = min(o for o, a in host)
        hi = max(o + a.size for o, a in host)
        staging = np.zeros(hi - lo, np_dtype)
        for o, a in host:
            staging[o - lo:o - lo + a.size] = a.reshape(-1).view(np_dtype)
        buf[lo:hi].copy_(torch.from_numpy(staging))
    for o, a, d in zip(offsets, arrays, on_dev):
        if d:
            buf[o:o + a.numel()].copy_(a.reshape(-1).view(dtype))
    return buf, offsets


_NUMPY = {torch.uint8: np.uint8, torch.int32: np.int32, torch.float32: np.float32}


def _size(a):
    return a.numel() if isinstance(a, torch.Tensor) else a.size


def out_fits(out, dtype, dev, shape=None, at_least=0):
    """`out` is a contiguous `dtype` tensor on `dev` of exactly `shape` or, without one (problems of mixed shapes share a flat buffer),
    of at least `at_least` elements."""
    return isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == dev and out.is_contiguous() and \
        (tuple(out.shape) == tuple(shape) if shape is not None else out.numel() >= at_least)


def views(flat, shapes):
    """The per-problem views of a flat buffer that holds arrays of `shapes` one behind the other."""
    out, o = [], 0
    for shape in shapes:
        n = int(np.prod(shape))
        out.append(flat[o:o + n].view(shape))
        o += n
    return out


def bad_problems(status, ok=(0,)):
    """The problems whose status is none of `ok` and their codes, as two numpy arrays; a device tensor is read back here (the one
    synchronisation of a call)."""
    st = status.cpu().numpy() if isinstance(status, torch.Tensor) else status
    wrong = st != ok[0]
    for code in ok[1:]:
        wrong &= st != code
    bad = np.flatnonzero(wrong)
    return bad, st[bad]
