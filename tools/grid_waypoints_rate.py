"""Rate of simq_grid_paths on the GPU, and of simq.shortest_paths with its two exact simplifiers: one JSON line with per-launch
latency and searches/s, and per-call latency of shortest_paths.

    python tools/grid_waypoints_rate.py [--reps 10] [--no-searches]

Workloads: those of tools/grid_paths_rate.py -- Mapper-style configuration spaces (184 x 232 small, 232 x 232 large), open and
cluttered, P = 1, 8, 64, 256, 1024 problems per launch (distinct random free sources and targets, the P problems spread over 8
grids).  Each problem is a whole search plus its walk; no image is written.  Timed with HIP events around `reps` back-to-back launches
after a warm-up, every status checked.  Includes the 96-byte-per-problem descriptor upload the C-ABI makes on the launch stream.

shortest_paths rows ('shortest_paths' in the result): the cluttered grids of both rooms as device-resident configuration spaces (the
grid is its own thin map, every cell its own closest cell), the same P, two rows each: simplify=simq.approximate_polygon_exact (dense
paths and map boxes to the host, simplification and pruning there) and simplify='exact' (simq_grid_waypoints behind the search, one
small read-back).  Whole calls on a host clock with the device synchronised at both ends: the median of 10 after 2 warm-ups.
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

from gen_grid_paths_golden import cluttered, padded_room  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default='1,8,64,256,1024')
    ap.add_argument('--no-searches', action='store_true', help='only the shortest_paths rows')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('grid_waypoints_rate.py needs a GPU')
    from simq import _lib
    from simq.waypoints import GridPathProblem
    dev = torch.device('cuda', 0)
    rooms = {'small': (184, 232, 44, 92), 'large': (232, 232, 92, 92)}
    result = {'metric': 'grid_paths', 'unit': 'ms per launch / searches per s', 'reps': args.reps, 'rows': []}
    rng = np.random.RandomState(0)
    cap = 512
    for room, (R, C, rr, rc) in rooms.items():
        for kind in ('open', 'cluttered'):
            grids = [padded_room(R, C, rr, rc) if kind == 'open' else cluttered(R, C, rr, rc, 10, 100 + k) for k in range(8)]
            packed = torch.from_numpy(np.concatenate([g.reshape(-1) for g in grids])).to(dev)
            boxes = []
            for g in grids:
                ii, jj = np.nonzero(g)
                boxes.append((int(ii.min()), int(jj.min()), int(ii.max() - ii.min() + 1), int(jj.max() - jj.min() + 1)))
            for P in [] if args.no_searches else [int(x) for x in args.sizes.split(',')]:
                probs = (GridPathProblem * P)()
                for p in range(P):
                    k = p % 8
                    ii, jj = np.nonzero(grids[k])
                    a, b = rng.randint(ii.size, size=2)
                    probs[p] = GridPathProblem(k * R * C, -1, -1, p * cap, -1, -1, cap, R, C, int(ii[a]), int(jj[a]), int(ii[b]), int(jj[b]),
                                               *boxes[k], 0)
                d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
                paths = torch.empty((P * cap, 2), dtype=torch.int32, device=dev)
                lengths, status = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
                ends = torch.zeros((P, 4), dtype=torch.int32, device=dev)
                stream = _lib.stream_ptr(dev)

                def launch():
                    _lib.lib.call('simq_grid_paths', _lib.ptr(packed), ctypes.c_int64(packed.numel()), None, ctypes.c_int64(0), probs, P,
                                  _lib.ptr(d_probs), _lib.ptr(paths), ctypes.c_int64(P * cap), _lib.ptr(lengths), _lib.ptr(ends), None,
                                  ctypes.c_int64(0), None, ctypes.c_int64(0), _lib.ptr(status), stream)

                for _ in range(2):
                    launch()
                torch.cuda.synchronize()
                assert not status.any().item()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                assert not status.any().item()
                ms = e0.elapsed_time(e1) / args.reps
                result['rows'].append({'room': room, 'grid': [R, C], 'kind': kind, 'P': P, 'ms_per_launch': round(ms, 4),
                                       'us_per_search': round(1e3 * ms / P, 3), 'searches_per_s': round(P / ms * 1e3, 1)})
    result['shortest_paths'] = shortest_paths_rows(dev, rooms, [int(x) for x in args.sizes.split(',')])
    print(json.dumps(result))


def shortest_paths_rows(dev, rooms, sizes):
    import statistics
    import time
    import simq
    from simq.waypoints import pixel_indices_to_position
    rows = []
    rng = np.random.RandomState(1)
    for room, (R, C, rr, rc) in rooms.items():
        grids = [cluttered(R, C, rr, rc, 10, 100 + k) for k in range(8)]
        cspace = torch.from_numpy(np.stack(grids)).to(dev)
        ii, jj = np.meshgrid(np.arange(R, dtype=np.int32), np.arange(C, dtype=np.int32), indexing='ij')
        closest = torch.from_numpy(np.stack([np.stack([ii, jj])] * 8)).to(dev)
        free = [np.argwhere(g != 0) for g in grids]
        for P in sizes:
            index = [p % 8 for p in range(P)]
            ends = [[pixel_indices_to_position(*[int(x) for x in free[k][rng.randint(len(free[k]))]], (R, C)) + (0.0,) for k in index]
                    for _ in range(2)]
            want = None
            for label, simplify in (('host', simq.approximate_polygon_exact), ('exact', 'exact')):
                times = []
                for rep in range(12):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = simq.shortest_paths(cspace, cspace, closest, ends[0], ends[1], map_index=index, simplify=simplify)
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                assert want is None or got == want
                want = got
                ms = 1e3 * statistics.median(times[2:])
                rows.append({'room': room, 'grid': [R, C], 'P': P, 'simplify': label, 'ms_per_call': round(ms, 3),
                             'us_per_path': round(1e3 * ms / P, 2), 'bent': sum(len(q) > 2 for q in got)})
    return rows


if __name__ == '__main__':
    main()
