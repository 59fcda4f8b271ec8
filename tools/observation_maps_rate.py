"""Rate of simq_observation_update on the GPU: one JSON line with per-launch latency and frames/s.

    python tools/observation_maps_rate.py [--reps 40] [--runs 3]

Workloads: frames of the overhead camera (156 x 156) and of the forward-facing camera (156 x 277) into the two padded rooms of the
reference (184 x 232 and 232 x 232), P = 1, 8, 64, 256, 1024 frames per launch, each on its own pair of device-resident maps.
`library`: HIP events around back-to-back iterations after a warm-up, an iteration being the upload of the P frames (depth, ids and
pixel tables, from one pinned host buffer, on the launch stream) and the library call with its descriptor upload; the median and the
spread of `runs` such windows (fewer iterations per window for the large P, whose upload dominates).  `python`: the whole
simq.observation_update call on numpy frames (packing, descriptor build, upload, launch, status readback), a host clock.  The maps are
checked against the numpy oracle (tests/observation_maps_oracle.py) on a sample of the problems before anything is timed.
"""
import argparse
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

import observation_maps_oracle as oracle  # noqa: E402

CAMERAS = {'overhead': (0.1, 10, 1), 'forward': (0.001, 1, 16.0 / 9)}
RANGES = oracle.IdRanges(3, 9, 10, 11, 20)


def frame(kind, rng, shape):
    """A frame at a random pose inside the room: a floor with a few raised blocks (overhead) or depth up to the far plane (forward)."""
    near, far, aspect = CAMERAS[kind]
    heading = rng.uniform(-np.pi, np.pi)
    x, y = rng.uniform(-0.4, 0.4), rng.uniform(-0.2, 0.2)
    if kind == 'overhead':
        g = oracle.camera_geometry((x, y, 1), (x, y, 0), (np.cos(heading), np.sin(heading), 0), near, far, aspect, 156)
        height = np.zeros((156, 156))
        ids = np.zeros((156, 156), np.int32)
        for k in range(8):
            i, j, h = rng.randint(0, 140), rng.randint(0, 140), (0.044, 0.1, 0.2)[k % 3]
            height[i:i + 12, j:j + 12] = h
            ids[i:i + 12, j:j + 12] = (11 + k, 3 + k % 7, 5)[k % 3]
        buffer = ((far - far * near / (1.0 - height)) / (far - near)).astype(np.float32)
    else:
        c, s = np.cos(np.radians(60)), np.sin(np.radians(60))
        g = oracle.camera_geometry((x, y, 0.08), (x + 0.14 * np.cos(heading), y + 0.14 * np.sin(heading), 0),
                                   (c * np.cos(heading), c * np.sin(heading), s), near, far, aspect, 156)
        buffer = np.where(rng.rand(156, 277) < 0.2, 1.0, rng.uniform(0.99, 1.0, (156, 277))).astype(np.float32)
        ids = np.asarray([-1, 0, 0, 0, 4, 10, 12], np.int32)[rng.randint(0, 7, (52, 93))].repeat(3, 0).repeat(3, 1)[:156, :277]
    return buffer, np.ascontiguousarray(ids), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--sizes', default='1,8,64,256,1024')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('observation_maps_rate.py needs a GPU')
    import simq
    from simq import _lib, observation
    dev = torch.device('cuda', 0)
    ranges = observation.IdRanges(*RANGES)
    result = {'metric': 'observation_maps', 'unit': 'ms per launch / frames per s', 'reps': args.reps, 'runs': args.runs, 'rows': []}
    for kind in CAMERAS:
        for shape in ((184, 232), (232, 232)):
            rng = np.random.RandomState(3)
            pool = [frame(kind, rng, shape) for _ in range(16)]
            for P in [int(x) for x in args.sizes.split(',')]:
                depth = np.stack([pool[p % 16][0] for p in range(P)])
                ids = np.stack([pool[p % 16][1] for p in range(P)])
                geoms = [observation.CameraGeometry(*pool[k][2]) for k in range(16)]
                geoms = [geoms[p % 16] for p in range(P)]
                over = torch.zeros((P,) + shape, dtype=torch.float32, device=dev)
                occ = torch.zeros((P,) + shape, dtype=torch.uint8, device=dev)
                simq.observation_update(depth, ids, geoms, ranges, over, occ)
                for p in sorted({0, P // 2, P - 1}):
                    want = np.zeros(shape, np.float32), np.zeros(shape, np.uint8)
                    assert oracle.update(want[0], want[1], depth[p], ids[p], pool[p % 16][2], RANGES) == 0
                    assert np.array_equal(over[p].cpu().numpy().view(np.int32), want[0].view(np.int32)) and np.array_equal(occ[p].cpu().numpy(), want[1])
                # the call's own packed frame buffer, refilled from pinned host memory every iteration
                call_args, status, keep = observation._prepare(depth, ids, geoms, ranges, over, occ)
                frames = keep[0]
                pinned = torch.empty(frames.numel(), dtype=torch.int32).pin_memory()
                pinned.copy_(frames.cpu())

                def launch():
                    frames.copy_(pinned, non_blocking=True)
                    _lib.lib.call('simq_observation_update', *call_args)

                for _ in range(3):
                    launch()
                torch.cuda.synchronize()
                assert not status.any().item()
                reps = max(4, args.reps // max(1, P // 64))
                lib_ms, py_ms = [], []
                for _ in range(args.runs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        launch()
                    e1.record()
                    torch.cuda.synchronize()
                    lib_ms.append(e0.elapsed_time(e1) / reps)
                    py_reps = max(2, reps // 4)
                    t0 = time.perf_counter()
                    for _ in range(py_reps):
                        simq.observation_update(depth, ids, geoms, ranges, over, occ)
                    torch.cuda.synchronize()
                    py_ms.append(1e3 * (time.perf_counter() - t0) / py_reps)
                ms = float(np.median(lib_ms))
                result['rows'].append({'camera': kind, 'map': list(shape), 'P': P, 'library_ms_per_launch': round(ms, 4),
                                       'library_ms_min_max': [round(min(lib_ms), 4), round(max(lib_ms), 4)], 'us_per_frame': round(1e3 * ms / P, 3),
                                       'frames_per_s': round(P / ms * 1e3, 1), 'python_ms_per_call': round(float(np.median(py_ms)), 4),
                                       'python_ms_min_max': [round(min(py_ms), 4), round(max(py_ms), 4)]})
    print(json.dumps(result))


if __name__ == '__main__':
    main()
