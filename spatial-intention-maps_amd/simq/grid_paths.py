"""Shortest-path distance images on the GPU: the distance half of the reference's ``shortest_paths.GridGraph``.

The reference (shortest_paths.pyx:26-114) builds an 8-connected graph over the free cells (``grid != 0``) of a uint8 grid and runs
SPFA from a source pixel; ``OccupancyMap`` rebuilds it on every map update (envs.py:2459) and ``Mapper`` asks it for two distance
images per robot per step (envs.py:2287-2300).  ``simq_grid_distance_images`` (csrc/grid_paths.hip) computes such images for many
(grid, source) problems in one launch, bit for bit equal to SPFA's distances: every update is fl32(d[u] + w) accepted when strictly
smaller, iterated to the fixed point, whose value does not depend on the visiting order.  SPFA's parents -- the waypoints of
``GridGraph.shortest_path`` -- do depend on its queue order, so this module produces distances only; ``simq.waypoints`` emulates the
search itself and has the waypoints (``simq.WaypointGraph``, ``simq.grid_dense_paths``, ``simq.shortest_paths``).
"""
import ctypes

import numpy as np
import torch

from . import _batch
from ._lib import SimqError, lib, ptr, stream_ptr


class GridProblem(ctypes.Structure):
    """simq_grid_problem of include/simq.h."""
    _fields_ = [('grid_offset', ctypes.c_int64), ('out_offset', ctypes.c_int64), ('rows', ctypes.c_int32), ('cols', ctypes.c_int32),
                ('src_i', ctypes.c_int32), ('src_j', ctypes.c_int32)]


def pixel(px):
    try:
        i, j = px
        return int(i), int(j)
    except (TypeError, ValueError):
        raise ValueError('a pixel is a pair (i, j), got %r' % (px,)) from None


def index_grids(grid_index, n_grids, n_sources):
    """grid_index of grid_distance_images / grid_dense_paths as a list of ints (problem p uses grid p when it is None)."""
    return _batch.problem_index(grid_index, n_grids, n_sources,
                                '%d grids but %d sources (grid_index shares grids between problems)' % (n_grids, n_sources),
                                'grid_index must name one of the %d grids for each of the %d sources' % (n_grids, n_sources))


class SnappedProblem(ctypes.Structure):
    """simq_grid_snapped_problem of include/simq.h."""
    _fields_ = [('grid_offset', ctypes.c_int64), ('closest_offset', ctypes.c_int64), ('out_offset', ctypes.c_int64), ('rows', ctypes.c_int32),
                ('cols', ctypes.c_int32), ('src_i', ctypes.c_int32), ('src_j', ctypes.c_int32), ('upstream', ctypes.c_int32),
                ('reserved_', ctypes.c_int32)]


SNAPPED_FILL = 0.0               # SIMQ_GRID_SNAPPED_FILL of include/simq.h
SNAPPED_PROBLEM = np.dtype(SnappedProblem)                       # the descriptor table as a numpy structured array


def check_closest(c, what='closest'):
    """An int32 [2, rows, cols] block of closest cells (scipy's return_indices layout): numpy, or a contiguous device tensor."""
    if isinstance(c, torch.Tensor):
        if c.dtype != torch.int32 or c.dim() != 3 or c.shape[0] != 2 or not c.is_contiguous():
            raise ValueError('%s must be a contiguous int32 [2, rows, cols] tensor, got %s %s' % (what, c.dtype, tuple(c.shape)))
        return c
    if not isinstance(c, np.ndarray) or c.dtype != np.int32 or c.ndim != 3 or c.shape[0] != 2:
        raise ValueError('%s must be an int32 [2, rows, cols] array, got %s' % (
            what, '%s %s' % (c.dtype, c.shape) if isinstance(c, np.ndarray) else type(c).__name__))
    return np.ascontiguousarray(c)


def _place(items, used, dtype, dev):
    """Where the problems read the items of `used`: (address, elements, {item: element offset}, what to keep alive).  Items that are
    views of one allocation on `dev` (the rows of one tensor, the maps of a simq.BatchedMapper) are read where they lie, as offsets
    from the lowest of them; anything else goes into one packed buffer that holds each used item once."""
    first = items[used[0]]
    if all(isinstance(items[k], torch.Tensor) and items[k].device == dev for k in used) and \
            all(items[k].untyped_storage().data_ptr() == first.untyped_storage().data_ptr() for k in used):
        size = first.element_size()
        base = min(items[k].data_ptr() for k in used)
        if all((items[k].data_ptr() - base) % size == 0 for k in used):
            end = max(items[k].data_ptr() + size * items[k].numel() for k in used)
            return base, (end - base) // size, {k: (items[k].data_ptr() - base) // size for k in used}, [items[k] for k in used]
    packed, offsets = _batch.pack([items[k] for k in used], dtype, dev)
    return packed.data_ptr(), packed.numel(), dict(zip(used, offsets)), packed


def _enqueue(grids, sources, pixels_per_meter=None, unreachable_to_max=False, scale=None, out=None, grid_index=None, closest=None,
             closest_index=None, upstream=None, upstream_index=None):
    """grid_distance_images without its status read-back: checks, uploads and queues the launch, and returns (out, status, uniform,
    shapes, name) with `status` the int32 device tensor the launch writes and `name` the entry point it went to.  upstream: an int32
    device tensor of status words of the stage that produced `closest` (simq_occupancy_maps' d_status), upstream_index: for every
    problem its word (omitted: the problem's closest block's index); a problem whose word is nonzero is not searched (include/simq.h).
    Both need `closest`."""
    grids, _ = _batch.as_maps(grids, 'grids')
    srcs = [pixel(s) for s in sources]
    if not grids or not srcs:
        raise ValueError('grid_distance_images needs at least one grid and one source')
    grid_index = index_grids(grid_index, len(grids), len(srcs))
    P = len(srcs)
    shapes = [tuple(grids[k].shape) for k in grid_index]
    if closest is None:
        if closest_index is not None or upstream is not None or upstream_index is not None:
            raise ValueError('closest_index, upstream and upstream_index need closest=')
    else:
        try:
            closest = [check_closest(c, 'closest[%d]' % k) for k, c in enumerate(closest)]
        except TypeError:
            raise ValueError('closest is a sequence of int32 [2, rows, cols] blocks or one [G, 2, rows, cols] array, got %s'
                             % type(closest).__name__) from None
        if closest_index is None and len(closest) == len(grids):
            closest_index = grid_index
        closest_index = _batch.problem_index(
            closest_index, len(closest), P, '%d closest blocks but %d sources (closest_index shares blocks between problems)' % (len(closest), P),
            'closest_index must name one of the %d closest blocks for each of the %d sources' % (len(closest), P))
        for p, k in enumerate(closest_index):
            if tuple(closest[k].shape[1:]) != shapes[p]:
                raise ValueError('problem %d: a grid of %s but closest[%d] is %s' % (p, shapes[p], k, tuple(closest[k].shape)))
        if upstream is not None:
            if not isinstance(upstream, torch.Tensor) or upstream.dtype != torch.int32 or upstream.dim() != 1 or not upstream.is_contiguous():
                raise ValueError('upstream must be a contiguous 1-D int32 device tensor of status words')
            upstream_index = _batch.problem_index(
                closest_index if upstream_index is None else upstream_index, upstream.numel(), P, '',
                'upstream_index must name one of the %d words of upstream for each of the %d sources' % (upstream.numel(), P))
        elif upstream_index is not None:
            raise ValueError('upstream_index needs upstream=')
    dev = _batch.device('grid distance images')
    if upstream is not None and upstream.device != dev:
        raise ValueError('upstream must be a contiguous 1-D int32 device tensor of status words')

    # one packed uint8 buffer holding each grid the problems use once (the snapped entry reads views of one device allocation in place)
    used = sorted(set(grid_index))
    if closest is None:
        packed, offsets = _batch.pack([grids[k] for k in used], torch.uint8, dev)
        goff = dict(zip(used, offsets))
    else:
        g_at, g_bytes, goff, keep_grids = _place(grids, used, torch.uint8, dev)
        c_at, c_ints, coff, keep_closest = _place(closest, sorted(set(closest_index)), torch.int32, dev)

    uniform = len(set(shapes)) == 1
    n_out = sum(r * c for r, c in shapes)
    want = (P,) + shapes[0] if uniform else (n_out,)
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=dev)
    elif not _batch.out_fits(out, torch.float32, dev, want if uniform else None, n_out):
        raise ValueError('out must be a contiguous float32 tensor on %s of %s' % (
            dev, 'shape %s' % (want,) if uniform else 'at least %d elements' % n_out))
    probs = (GridProblem * P)() if closest is None else (SnappedProblem * P)()
    o = 0
    for p, (k, (r, c), (i, j)) in enumerate(zip(grid_index, shapes, srcs)):
        if closest is None:
            probs[p] = GridProblem(goff[k], o, r, c, i, j)
        else:
            probs[p] = SnappedProblem(goff[k], coff[closest_index[p]], o, r, c, i, j, -1 if upstream is None else upstream_index[p], 0)
        o += r * c
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    ppm = 1.0 if pixels_per_meter is None else float(pixels_per_meter)
    sc = 1.0 if scale is None else float(scale)
    if closest is None:
        name = 'simq_grid_distance_images'
        lib.call(name, ptr(packed), ctypes.c_int64(packed.numel()), probs, P, ptr(d_probs), ptr(out), ctypes.c_int64(out.numel()),
                 ctypes.c_float(ppm), int(bool(unreachable_to_max)), ctypes.c_float(sc), ptr(status), stream_ptr(dev))
    else:
        name = 'simq_grid_distance_images_snapped'
        lib.call(name, ctypes.c_void_p(g_at), ctypes.c_int64(g_bytes), ctypes.c_void_p(c_at), ctypes.c_int64(c_ints), probs, P, ptr(d_probs),
                 ptr(out), ctypes.c_int64(out.numel()), ctypes.c_float(ppm), int(bool(unreachable_to_max)), ctypes.c_float(sc), ptr(upstream),
                 0 if upstream is None else upstream.numel(), ptr(status), stream_ptr(dev))
        del keep_grids, keep_closest
    return out, status, uniform, shapes, name


def grid_distance_images(grids, sources, pixels_per_meter=None, unreachable_to_max=False, scale=None, out=None, grid_index=None,
                         closest=None, closest_index=None):
    """Distance images of P (grid, source) problems in one launch.

    grids: a sequence of 2-D uint8 grids (numpy arrays or uint8 device tensors), or one [G, rows, cols] array / tensor; a cell is free
    where its grid is nonzero.  sources: P pixels (i, j).  grid_index: P indices into `grids` (several problems may share one grid);
    omitted, problem p uses grid p.  Each image follows Mapper._create_global_shortest_path_map (envs.py:2294-2299) applied to
    OccupancyMap.shortest_path_image (envs.py:2513-2516): d (-1 where unreachable) / pixels_per_meter; with unreachable_to_max the
    negative values replaced by the image max; * scale.  None skips a step.

    closest: the closest free cells of the grids -- int32 [2, rows, cols] blocks (numpy or device tensors) or one [G, 2, rows, cols]
    array / tensor, what simq.occupancy_maps returns as closest_cspace_indices.  With it every source goes through
    closest[:, i, j] on the device before its search (OccupancyMap._closest_valid_cspace_indices, envs.py:2522-2523), and grids and
    closest blocks that are views of one device allocation each (the rows of one tensor) are read where they lie.  closest_index: P indices into `closest`;
    omitted, a problem uses the block of its grid's index (as many blocks as grids) or block p.

    Returns a float32 device tensor [P, rows, cols] when every problem has the same shape (written into `out` when given: a
    contiguous float32 tensor of that shape on the device), otherwise a list of P [rows_p, cols_p] views into one packed buffer (`out`:
    a contiguous float32 device tensor of at least sum(rows_p * cols_p) elements).  Raises SimqError for an out-of-range source or an
    oversized grid (the library checks before it launches anything), when a problem hit the library's pass cap and, with `closest`,
    for the problems whose snapped pixel is no free cell of their grid (status 3; their images hold 0)."""
    out, status, uniform, shapes, name = _enqueue(grids, sources, pixels_per_meter, unreachable_to_max, scale, out, grid_index, closest,
                                                  closest_index)
    bad, codes = _batch.bad_problems(status)
    if bad.size:
        if closest is not None and (codes == 3).all():
            raise SimqError('%s: the closest cell of %d source(s) is no free cell of their grid (status 3 at problems %s)'
                            % (name, bad.size, bad[:8].tolist()))
        raise SimqError('%s: %d problem(s) did not converge (status %s at problems %s)'
                        % (name, bad.size, codes[:8].tolist(), bad[:8].tolist()))
    return out if uniform else _batch.views(out.view(-1), shapes)


class GridGraph:
    """Drop-in for the distance half of shortest_paths.GridGraph (shortest_paths.pyx:10-162).

    GridGraph(grid): grid is a 2-D C-contiguous uint8 numpy array (the reference's `unsigned char[:, ::1]`); it is copied here, so
    later changes to the caller's array do not change the distances (the reference builds its edges at construction).  Results are
    cached per source, as _spfa_with_cache does; shortest_path_images computes every uncached source of a list in one launch."""

    def __init__(self, grid):
        if isinstance(grid, torch.Tensor):
            raise ValueError('GridGraph takes a 2-D C-contiguous uint8 numpy array (unsigned char[:, ::1]), got a tensor')
        self.grid = _batch.check_grid(grid).copy()
        self.num_rows, self.num_cols = self.grid.shape
        self.cache = {}
        self._dev_grid = None

    def _pixel_in_grid(self, px, what):
        i, j = pixel(px)
        if not (0 <= i < self.num_rows and 0 <= j < self.num_cols):
            raise SimqError('%s (%d, %d) outside the %d x %d grid' % (what, i, j, self.num_rows, self.num_cols))
        return i, j

    def shortest_path_images(self, sources):
        """float32 [rows, cols] distance images (-1: unreachable) of every source; the uncached ones computed in one launch."""
        keys = [self._pixel_in_grid(s, 'source') for s in sources]
        todo = list(dict.fromkeys(k for k in keys if k not in self.cache))
        if todo:
            if self._dev_grid is None:
                self._dev_grid = torch.from_numpy(self.grid).to(_batch.device('grid distance images'))
            imgs = grid_distance_images([self._dev_grid], todo, grid_index=[0] * len(todo))
            for k, img in zip(todo, imgs.cpu().numpy()):
                self.cache[k] = img
        return [self.cache[k] for k in keys]

    def shortest_path_image(self, source):
        """The float32 [rows, cols] distance image from `source` (shortest_paths.pyx:160-162): the cached array itself, as there."""
        return self.shortest_path_images([source])[0]

    def shortest_path_distance(self, source, target):
        """Distance from `source` to `target` as a Python float, -1.0 when unreachable (shortest_paths.pyx:150-158)."""
        ti, tj = self._pixel_in_grid(target, 'target')
        return float(self.shortest_path_image(source)[ti, tj])

    def shortest_path(self, source, target):
        raise NotImplementedError('simq.GridGraph computes distances only: the waypoints of shortest_path follow the parents SPFA '
                                  'records, and those depend on the order it visits cells wherever equal-length paths tie, which no '
                                  'parallel relaxation reproduces; simq.WaypointGraph emulates the search itself and has them')
