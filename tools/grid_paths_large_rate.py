"""Rate of simq_grid_paths_large on the GPU -- the search of simq_grid_paths with its state in global memory: one JSON line.

    python tools/grid_paths_large_rate.py [--reps 20]

Two measurements, both with HIP events around `reps` back-to-back launches after two warm-up launches, every status checked; each
problem is a whole search plus its walk, no image is written; the descriptor upload the C-ABI makes on the launch stream is inside.
  under_the_cap   the same problems through simq_grid_paths and simq_grid_paths_large, P = 1, 64, 1 024: the cluttered 232 x 232
                  Mapper-style configuration spaces of tools/grid_waypoints_rate.py (a 92 x 92 room, so the window fits LDS), distinct
                  random free sources and targets over 8 grids.  The ratio is the price of the state in global memory.
  over_the_cap    232 x 232 grids that are free up to their border, so that the window is the whole grid (54 756 cells with the halo,
                  543 840 bytes of workspace a problem): open, and cluttered with 10 % of the cells blocked at random; P = 1, 8, 64,
                  256 through simq_grid_paths_large, which is the only entry point that takes them.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gen_grid_paths_golden import cluttered  # noqa: E402

CAP = 512


def free_box(g):
    ii, jj = np.nonzero(g)
    return int(ii.min()), int(jj.min()), int(ii.max() - ii.min() + 1), int(jj.max() - jj.min() + 1)


def timed(launch, status, reps):
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    assert not status.any().item()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    assert not status.any().item()
    return e0.elapsed_time(e1) / reps


def measure(entry, grids, P, rng, reps, dev):
    """ms per launch of `entry` over P problems spread over `grids` (all of one shape), random free sources and targets."""
    from simq import _lib
    from simq.waypoints import GridPathLargeProblem, GridPathProblem
    R, C = grids[0].shape
    packed = torch.from_numpy(np.concatenate([g.reshape(-1) for g in grids])).to(dev)
    boxes = [free_box(g) for g in grids]
    free = [np.argwhere(g != 0) for g in grids]
    large = entry == 'simq_grid_paths_large'
    need = [_lib.lib.c.simq_grid_paths_large_work_bytes(boxes[p % len(grids)][2], boxes[p % len(grids)][3]) for p in range(P)]
    at = np.concatenate([[0], np.cumsum(need)]).tolist()
    kind = GridPathLargeProblem if large else GridPathProblem
    probs = (kind * P)()
    for p in range(P):
        k = p % len(grids)
        a, b = rng.randint(len(free[k]), size=2)
        probs[p] = kind(k * R * C, -1, -1, p * CAP, -1, -1, *([at[p]] if large else []), CAP, R, C, int(free[k][a][0]), int(free[k][a][1]),
                        int(free[k][b][0]), int(free[k][b][1]), *boxes[k], 0)
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
    paths = torch.empty((P * CAP, 2), dtype=torch.int32, device=dev)
    lengths, status = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
    ends = torch.zeros((P, 4), dtype=torch.int32, device=dev)
    work = torch.empty(at[-1], dtype=torch.uint8, device=dev) if large else None
    extra = (_lib.ptr(work), ctypes.c_int64(at[-1])) if large else ()
    stream = _lib.stream_ptr(dev)

    def launch():
        _lib.lib.call(entry, _lib.ptr(packed), ctypes.c_int64(packed.numel()), None, ctypes.c_int64(0), probs, P, _lib.ptr(d_probs),
                      _lib.ptr(paths), ctypes.c_int64(P * CAP), _lib.ptr(lengths), _lib.ptr(ends), None, ctypes.c_int64(0), None,
                      ctypes.c_int64(0), _lib.ptr(status), *extra, stream)

    return timed(launch, status, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('grid_paths_large_rate.py needs a GPU')
    dev = torch.device('cuda', 0)
    result = {'metric': 'grid_paths_large', 'unit': 'ms per launch', 'reps': args.reps, 'under_the_cap': [], 'over_the_cap': []}
    room = [cluttered(232, 232, 92, 92, 10, 100 + k) for k in range(8)]
    for P in (1, 64, 1024):
        ms = {}
        for entry in ('simq_grid_paths', 'simq_grid_paths_large'):
            ms[entry] = measure(entry, room, P, np.random.RandomState(P), args.reps, dev)       # (the same problems for both)
        result['under_the_cap'].append({'grid': [232, 232], 'window': list(free_box(room[0])[2:]), 'P': P,
                                        'lds_ms': round(ms['simq_grid_paths'], 4), 'hbm_ms': round(ms['simq_grid_paths_large'], 4),
                                        'ratio': round(ms['simq_grid_paths_large'] / ms['simq_grid_paths'], 2)})
    whole = {'open': [np.ones((232, 232), np.uint8)] * 8,
             'cluttered': [(np.random.RandomState(200 + k).rand(232, 232) >= 0.1).astype(np.uint8) for k in range(8)]}
    for kind, grids in whole.items():
        for g in grids:
            g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 1                                          # the window is the whole grid
        for P in (1, 8, 64, 256):
            ms = measure('simq_grid_paths_large', grids, P, np.random.RandomState(P), args.reps, dev)
            result['over_the_cap'].append({'grid': [232, 232], 'kind': kind, 'P': P, 'ms_per_launch': round(ms, 4),
                                           'ms_per_search': round(ms / P, 4), 'searches_per_s': round(P / ms * 1e3, 1)})
    print(json.dumps(result))


if __name__ == '__main__':
    main()
