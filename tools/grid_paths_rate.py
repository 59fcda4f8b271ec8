"""Rate of simq_grid_distance_images on the GPU: one JSON line with per-launch latency and images/s.

    python tools/grid_paths_rate.py [--reps 20]

Workloads: Mapper-style configuration spaces (tools/gen_grid_paths_golden.py's padded rooms: 184 x 232 small, 232 x 232 large), open
and cluttered, P = 1, 8, 64, 256, 1024 problems per launch (distinct random free sources, the P problems spread over 8 grids as a
step's robots would be).  Timed with HIP events around `reps` back-to-back launches after a warm-up; the images are checked
against one un-timed launch first.  Includes the 32-byte-per-problem descriptor upload the C-ABI makes on the launch stream.
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='1,8,64,256,1024')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('grid_paths_rate.py needs a GPU')
    import simq
    from simq import _lib
    from simq.grid_paths import GridProblem
    dev = torch.device('cuda', 0)
    rooms = {'small': (184, 232, 44, 92), 'large': (232, 232, 92, 92)}
    result = {'metric': 'grid_distance_images', 'unit': 'ms per launch / images per s', 'reps': args.reps, 'rows': []}
    rng = np.random.RandomState(0)
    for room, (R, C, rr, rc) in rooms.items():
        for kind in ('open', 'cluttered'):
            grids = [padded_room(R, C, rr, rc) if kind == 'open' else cluttered(R, C, rr, rc, 10, 100 + k) for k in range(8)]
            packed = torch.from_numpy(np.concatenate([g.reshape(-1) for g in grids])).to(dev)
            for P in [int(x) for x in args.sizes.split(',')]:
                idx = [p % 8 for p in range(P)]
                srcs = []
                for k in idx:
                    ii, jj = np.nonzero(grids[k])
                    q = rng.randint(ii.size)
                    srcs.append((int(ii[q]), int(jj[q])))
                check = simq.grid_distance_images(grids, srcs, grid_index=idx)
                probs = (GridProblem * P)(*[GridProblem(k * R * C, p * R * C, R, C, i, j) for p, (k, (i, j)) in enumerate(zip(idx, srcs))])
                out = torch.empty(P, R, C, device=dev)
                d_probs = torch.empty(32 * P, dtype=torch.uint8, device=dev)
                status = torch.zeros(P, dtype=torch.int32, device=dev)
                stream = _lib.stream_ptr(dev)

                def launch():
                    _lib.lib.call('simq_grid_distance_images', _lib.ptr(packed), ctypes.c_int64(packed.numel()), probs, P, _lib.ptr(d_probs),
                                  _lib.ptr(out), ctypes.c_int64(out.numel()), ctypes.c_float(1.0), 0, ctypes.c_float(1.0), _lib.ptr(status), stream)

                for _ in range(3):
                    launch()
                torch.cuda.synchronize()
                assert torch.equal(out.view(torch.int32), check.view(torch.int32)) and not status.any().item()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                assert not status.any().item()
                ms = e0.elapsed_time(e1) / args.reps
                result['rows'].append({'room': room, 'grid': [R, C], 'kind': kind, 'P': P, 'ms_per_launch': round(ms, 4),
                                       'us_per_image': round(1e3 * ms / P, 3), 'images_per_s': round(P / ms * 1e3, 1)})
    print(json.dumps(result))


if __name__ == '__main__':
    main()
