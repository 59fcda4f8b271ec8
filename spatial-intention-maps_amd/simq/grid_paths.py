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


def grid_distance_images(grids, sources, pixels_per_meter=None, unreachable_to_max=False, scale=None, out=None, grid_index=None):
    """Distance images of P (grid, source) problems in one launch.

    grids: a sequence of 2-D uint8 grids (numpy arrays or uint8 device tensors), or one [G, rows, cols] array / tensor; a cell is free
    where its grid is nonzero.  sources: P pixels (i, j).  grid_index: P indices into `grids` (several problems may share one grid);
    omitted, problem p uses grid p.  Each image follows Mapper._create_global_shortest_path_map (envs.py:2294-2299) applied to
    OccupancyMap.shortest_path_image (envs.py:2513-2516): d (-1 where unreachable) / pixels_per_meter; with unreachable_to_max the
    negative values replaced by the image max; * scale.  None skips a step.

    Returns a float32 device tensor [P, rows, cols] when every problem has the same shape (written into `out` when given: a
    contiguous float32 tensor of that shape on the device), otherwise a list of P [rows_p, cols_p] views into one packed buffer (`out`:
    a contiguous float32 device tensor of at least sum(rows_p * cols_p) elements).  Raises SimqError for an out-of-range source or an
    oversized grid (the library checks before it launches anything) and when a problem hit the library's pass cap."""
    grids, _ = _batch.as_maps(grids, 'grids')
    srcs = [pixel(s) for s in sources]
    if not grids or not srcs:
        raise ValueError('grid_distance_images needs at least one grid and one source')
    grid_index = index_grids(grid_index, len(grids), len(srcs))
    dev = _batch.device('grid distance images')

    # one packed uint8 buffer holding each grid the problems use once
    used = sorted(set(grid_index))
    packed, offsets = _batch.pack([grids[k] for k in used], torch.uint8, dev)
    goff = dict(zip(used, offsets))

    shapes = [tuple(grids[k].shape) for k in grid_index]
    uniform = len(set(shapes)) == 1
    n_out = sum(r * c for r, c in shapes)
    want = (len(srcs),) + shapes[0] if uniform else (n_out,)
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=dev)
    elif not _batch.out_fits(out, torch.float32, dev, want if uniform else None, n_out):
        raise ValueError('out must be a contiguous float32 tensor on %s of %s' % (
            dev, 'shape %s' % (want,) if uniform else 'at least %d elements' % n_out))
    probs = (GridProblem * len(srcs))()
    o = 0
    for p, (k, (r, c), (i, j)) in enumerate(zip(grid_index, shapes, srcs)):
        probs[p] = GridProblem(goff[k], o, r, c, i, j)
        o += r * c
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    status = torch.empty(len(srcs), dtype=torch.int32, device=dev)
    ppm = 1.0 if pixels_per_meter is None else float(pixels_per_meter)
    sc = 1.0 if scale is None else float(scale)
    lib.call('simq_grid_distance_images', ptr(packed), ctypes.c_int64(packed.numel()), probs, len(srcs), ptr(d_probs), ptr(out),
             ctypes.c_int64(out.numel()), ctypes.c_float(ppm), int(bool(unreachable_to_max)), ctypes.c_float(sc), ptr(status),
             stream_ptr(dev))
    bad, codes = _batch.bad_problems(status)
    if bad.size:
        raise SimqError('simq_grid_distance_images: %d problem(s) did not converge (status %s at problems %s)'
                        % (bad.size, codes[:8].tolist(), bad[:8].tolist()))
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
