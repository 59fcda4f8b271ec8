"""Rate of simq_occupancy_maps on the GPU: one JSON line with per-launch latency and maps/s.

    python tools/occupancy_maps_rate.py [--reps 50] [--runs 3]

Workloads: the two padded rooms of the reference (184 x 232 and 232 x 232) with walls and a few boxes seen, dilation radius 6 and
thin radius 3, P = 1, 8, 64, 256, 1024 maps per launch sharing one room mask.  `library`: HIP events around `reps` back-to-back
library calls after a warm-up, the 40-byte-per-problem descriptor upload the C-ABI makes on the launch stream included; the median
and the spread of `runs` such windows.  `python`: the whole simq.occupancy_maps call on device-resident maps (packing, descriptor
build, launch, status readback), a host clock around calls that end in a device synchronise.  The results are checked against the
numpy oracle (tests/occupancy_maps_oracle.py) on a sample of the maps before anything is timed.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import occupancy_maps_oracle as oracle  # noqa: E402


def room(rows, cols, room_rows, room_cols):
    mask = np.zeros((rows, cols), np.uint8)
    i0, j0 = rows // 2 - room_rows // 2, cols // 2 - room_cols // 2
    mask[i0:i0 + room_rows, j0:j0 + room_cols] = 1
    return mask, (i0, j0)


def seen_map(mask, origin, room_rows, room_cols, boxes, seed):
    """An occupancy map after some steps: the walls around the room and `boxes` small obstacles."""
    rng = np.random.RandomState(seed)
    i0, j0 = origin
    occ = np.zeros_like(mask)
    occ[i0 - 3:i0 + room_rows + 3, j0 - 3:j0 + room_cols + 3] = 1
    occ[mask != 0] = 0
    for _ in range(boxes):
        i, j = i0 + rng.randint(room_rows - 4), j0 + rng.randint(room_cols - 4)
        occ[i:i + 4, j:j + 4] = 1
    return occ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--sizes', default='1,8,64,256,1024')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('occupancy_maps_rate.py needs a GPU')
    import simq
    from simq import _lib
    from simq.occupancy import OccupancyProblem
    dev = torch.device('cuda', 0)
    radius, thin = 6, 3
    result = {'metric': 'occupancy_maps', 'unit': 'ms per launch / maps per s', 'reps': args.reps, 'runs': args.runs, 'radius': radius,
              'thin_radius': thin, 'rows': []}
    for name, (R, C, rr, rc) in {'small': (184, 232, 44, 92), 'large': (232, 232, 92, 92)}.items():
        mask, origin = room(R, C, rr, rc)
        for P in [int(x) for x in args.sizes.split(',')]:
            occ = np.stack([seen_map(mask, origin, rr, rc, 2 + p % 9, 100 + p) for p in range(P)])
            d_occ = torch.from_numpy(occ).to(dev)
            d_mask = torch.from_numpy(mask).to(dev)
            check = simq.occupancy_maps(d_occ, [d_mask], radius, thin, room_index=[0] * P)
            for p in sorted({0, P // 2, P - 1}):
                for got, want in zip(check, oracle.update(occ[p], mask, radius, thin)):
                    assert np.array_equal(got[p].cpu().numpy(), want), (name, P, p)
            n = R * C
            packed = torch.cat([d_occ.view(-1), d_mask.view(-1)])
            probs = (OccupancyProblem * P)(*[OccupancyProblem(p * n, P * n, p * n, R, C, radius, thin) for p in range(P)])
            d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=dev)
            cs, th = torch.empty(P, R, C, dtype=torch.uint8, device=dev), torch.empty(P, R, C, dtype=torch.uint8, device=dev)
            near = torch.empty(P, 2, R, C, dtype=torch.int32, device=dev)
            status = torch.zeros(P, dtype=torch.int32, device=dev)
            stream = _lib.stream_ptr(dev)

            def launch():
                _lib.lib.call('simq_occupancy_maps', _lib.ptr(packed), ctypes.c_int64(packed.numel()), probs, P, _lib.ptr(d_probs), _lib.ptr(cs),
                              _lib.ptr(th), ctypes.c_int64(cs.numel()), _lib.ptr(near), ctypes.c_int64(near.numel()), _lib.ptr(status), stream)

            for _ in range(3):
                launch()
            torch.cuda.synchronize()
            assert torch.equal(cs, check[0]) and torch.equal(th, check[1]) and torch.equal(near, check[2]) and not status.any().item()
            lib_ms, py_ms = [], []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                lib_ms.append(e0.elapsed_time(e1) / args.reps)
                py_reps = max(3, args.reps // 10)
                t0 = time.perf_counter()
                for _ in range(py_reps):
                    simq.occupancy_maps(d_occ, [d_mask], radius, thin, room_index=[0] * P, out=(cs, th, near))
                torch.cuda.synchronize()
                py_ms.append(1e3 * (time.perf_counter() - t0) / py_reps)
            assert not status.any().item()
            ms = float(np.median(lib_ms))
            result['rows'].append({'room': name, 'map': [R, C], 'P': P, 'library_ms_per_launch': round(ms, 4),
                                   'library_ms_min_max': [round(min(lib_ms), 4), round(max(lib_ms), 4)], 'us_per_map': round(1e3 * ms / P, 3),
                                   'maps_per_s': round(P / ms * 1e3, 1), 'python_ms_per_call': round(float(np.median(py_ms)), 4),
                                   'python_ms_min_max': [round(min(py_ms), 4), round(max(py_ms), 4)]})
    print(json.dumps(result))


if __name__ == '__main__':
    main()
