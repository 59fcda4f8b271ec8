"""Rate of simq_grid_distance_queries on the GPU, beside the route the same queries had to take before it: one JSON line.

    python tools/grid_queries_rate.py [--reps 20] [--runs 3]

Workloads: the two padded rooms of the reference (184 x 232 and 232 x 232) with walls and a few boxes seen (tools/
occupancy_maps_rate.py's maps), their configuration spaces and closest cells left on the device by simq.occupancy_maps; P = 1, 8, 64,
256 problems (one map, one receptacle each) with Q = 10, 20 cube positions each, as a step's partial rewards ask.  Per (room, P, Q):
  library   HIP events around `reps` back-to-back simq_grid_distance_queries calls after a warm-up, the descriptor and target upload
            the C-ABI makes on the launch stream included; median and spread of `runs` windows
  python    the whole simq.shortest_path_distances call (pixels, packing, launch, the one read-back, the float64 division), host clock
  images    the route without this operator: closest.cpu(), the snap on the host, simq.grid_distance_images for the snapped
            receptacles, the images read back, host indexing and division -- host clock, same inputs, same machine
The two routes' results are compared bit for bit before anything is timed.  No pass or fail threshold.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from occupancy_maps_rate import room, seen_map  # noqa: E402


def images_route(simq, cspace, closest, receptacles, cubes):
    """The same distances through simq.grid_distance_images: what a caller had before simq.shortest_path_distances."""
    from simq.local_maps import position_to_pixel_indices
    near = closest.cpu().numpy()
    shape = tuple(cspace.shape[1:])
    sources = [tuple(int(x) for x in near[p][(slice(None),) + position_to_pixel_indices(r[0], r[1], shape)]) for p, r in enumerate(receptacles)]
    images = simq.grid_distance_images(cspace, sources).cpu().numpy()
    out = []
    for p, cs in enumerate(cubes):
        px = np.asarray([position_to_pixel_indices(c[0], c[1], shape) for c in cs]).reshape(-1, 2)
        si, sj = near[p, 0, px[:, 0], px[:, 1]], near[p, 1, px[:, 0], px[:, 1]]
        out.append(images[p, si, sj].astype(np.float64) / 96.0)
    return out


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--sizes', default='1,8,64,256')
    ap.add_argument('--targets', default='10,20')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('grid_queries_rate.py needs a GPU')
    import simq
    from simq import _lib
    from simq.grid_queries import GridQueryProblem
    from simq.local_maps import position_to_pixel_indices
    dev = torch.device('cuda', 0)
    result = {'metric': 'grid_distance_queries', 'unit': 'ms per launch / ms per call', 'reps': args.reps, 'runs': args.runs, 'rows': []}
    rng = np.random.RandomState(0)
    for name, (R, C, rr, rc) in {'small': (184, 232, 44, 92), 'large': (232, 232, 92, 92)}.items():
        mask, origin = room(R, C, rr, rc)
        half_x, half_y = rc / 2 / 96.0, rr / 2 / 96.0
        for P in [int(x) for x in args.sizes.split(',')]:
            occ = np.stack([seen_map(mask, origin, rr, rc, 2 + p % 9, 100 + p) for p in range(P)])
            maps = simq.occupancy_maps(torch.from_numpy(occ).to(dev), [torch.from_numpy(mask).to(dev)], 6, 3, room_index=[0] * P)
            cspace, closest = maps.configuration_space, maps.closest_cspace_indices
            receptacles = [(half_x - 0.08, half_y - 0.08, 0.0)] * P                  # a corner of the room, as in the reference
            for Q in [int(x) for x in args.targets.split(',')]:
                cubes = [[(rng.uniform(-half_x, half_x), rng.uniform(-half_y, half_y), 0.02) for _ in range(Q)] for _ in range(P)]
                got = simq.shortest_path_distances(cspace, closest, receptacles, cubes)
                want = images_route(simq, cspace, closest, receptacles, cubes)
                assert all(np.array_equal(g.view(np.int64), w.view(np.int64)) for g, w in zip(got, want)), (name, P, Q)

                n = R * C
                src = position_to_pixel_indices(receptacles[0][0], receptacles[0][1], (R, C))
                probs = (GridQueryProblem * P)(*[GridQueryProblem(p * n, 2 * p * n, p * n, p * Q, Q, R, C, src[0], src[1], 0) for p in range(P)])
                flat = np.asarray([position_to_pixel_indices(c[0], c[1], (R, C)) for cs in cubes for c in cs], np.int32)
                desc = torch.empty(ctypes.sizeof(probs) + 8 * P * Q, dtype=torch.uint8, device=dev)
                work = torch.empty(P * n, dtype=torch.float32, device=dev)
                out = torch.empty(P * Q, dtype=torch.float32, device=dev)
                status = torch.zeros(P, dtype=torch.int32, device=dev)
                stream = _lib.stream_ptr(dev)

                def launch():
                    _lib.lib.call('simq_grid_distance_queries', _lib.ptr(cspace), ctypes.c_int64(cspace.numel()), _lib.ptr(closest),
                                  ctypes.c_int64(closest.numel()), probs, P, flat.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(P * Q),
                                  _lib.ptr(desc), _lib.ptr(work), ctypes.c_int64(work.numel()), 0, _lib.ptr(out), ctypes.c_int64(P * Q),
                                  _lib.ptr(status), stream)

                for _ in range(3):
                    launch()
                torch.cuda.synchronize()
                assert not status.any().item()
                assert np.array_equal((out.cpu().numpy().astype(np.float64) / 96.0).view(np.int64), np.concatenate(got).view(np.int64))
                lib_ms, py_ms, img_ms = [], [], []
                slow_reps = max(2, args.reps // 5)
                for _ in range(args.runs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        launch()
                    e1.record()
                    torch.cuda.synchronize()
                    lib_ms.append(e0.elapsed_time(e1) / args.reps)
                    py_ms.append(host_ms(lambda: simq.shortest_path_distances(cspace, closest, receptacles, cubes), slow_reps))
                    img_ms.append(host_ms(lambda: images_route(simq, cspace, closest, receptacles, cubes), slow_reps))
                assert not status.any().item()

                def stat(v):
                    return round(float(np.median(v)), 4), [round(min(v), 4), round(max(v), 4)]
                row = {'room': name, 'map': [R, C], 'P': P, 'Q': Q}
                for key, v in (('library_ms_per_launch', lib_ms), ('python_ms_per_call', py_ms), ('images_route_ms_per_call', img_ms)):
                    row[key], row[key.replace('_per_launch', '').replace('_per_call', '') + '_min_max'] = stat(v)
                row['us_per_query'] = round(1e3 * row['library_ms_per_launch'] / (P * Q), 3)
                result['rows'].append(row)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
