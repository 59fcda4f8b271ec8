"""Rate of simq_intention_maps on the GPU: one JSON line with per-launch latency and maps/s.

    python tools/intention_maps_rate.py [--reps 50]

Workload: the 'ramp' intention map of a four-robot environment for P = 1, 8, 64, 256 robots per launch in both room sizes (184 x 232
and 232 x 232 global maps): every map draws the paths of the three other robots, four waypoints each (nine segments per map), line
thickness 2.  `ms_per_launch`: HIP events around `reps` back-to-back library calls after a warm-up -- the descriptor upload the C-ABI
makes on the launch stream included, the Python side's descriptor building not; `host_ms_per_call`: wall time of simq.intention_maps
itself, device-synchronised; `chain_ms`: intention_maps followed by local_state_images of the maps, one ('map', k) channel per robot.
`mixed`: P maps of each room shape drawn by one simq_intention_maps_shapes call (`one_call_ms`) against the two simq_intention_maps
calls it replaces (`two_calls_ms`, the sum of the two): the median, minimum and maximum over `--blocks` blocks of `reps` calls.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--sizes', default='1,8,64,256')
    ap.add_argument('--blocks', type=int, default=10, help='blocks of `reps` calls per way of the mixed form: their spread is reported')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('intention_maps_rate.py needs a GPU')
    import simq
    from simq import _lib, intention_drawing as im
    rng = np.random.RandomState(0)
    result = {'metric': 'intention_maps', 'unit': 'ms per launch / maps per s', 'encoding': 'ramp', 'line_thickness': 2, 'reps': args.reps, 'rows': []}
    for rows, cols, half in ((184, 232, (0.2, 0.45)), (232, 232, (0.45, 0.45))):
        for P in [int(x) for x in args.sizes.split(',')]:
            n_env = (P + 3) // 4
            point = lambda: (rng.uniform(-half[1], half[1]), rng.uniform(-half[0], half[0]), 0.0)
            envs = [[[point() for _ in range(4)] for _ in range(4)] for _ in range(n_env)]
            paths = [[envs[p // 4][r] for r in range(4) if r != p % 4] for p in range(P)]
            poses = [((envs[p // 4][p % 4][0][0], envs[p // 4][p % 4][0][1]), rng.uniform(-math.pi, math.pi)) for p in range(P)]
            check = simq.intention_maps(paths, (rows, cols), 'ramp')
            call, out, keep = im._prepare(paths, (rows, cols), 'ramp', 1.0, 2, None)
            for _ in range(5):
                _lib.lib.call('simq_intention_maps', *call)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), check.view(torch.int32)) and float(out.max()) == 1.0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                _lib.lib.call('simq_intention_maps', *call)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.reps
            t0 = time.perf_counter()
            for _ in range(5):
                simq.intention_maps(paths, (rows, cols), 'ramp', out=out)
            torch.cuda.synchronize()
            host_ms = 1e3 * (time.perf_counter() - t0) / 5
            channels = [[('map', p)] for p in range(P)]
            simq.local_state_images(out, channels, poses)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                simq.local_state_images(simq.intention_maps(paths, (rows, cols), 'ramp', out=out), channels, poses)
            torch.cuda.synchronize()
            chain_ms = 1e3 * (time.perf_counter() - t0) / 3
            result['rows'].append({'maps': [rows, cols], 'P': P, 'segments': call[1], 'ms_per_launch': round(ms, 4),
                                   'us_per_map': round(1e3 * ms / P, 3), 'maps_per_s': round(P / ms * 1e3, 1),
                                   'host_ms_per_call': round(host_ms, 3), 'chain_ms': round(chain_ms, 3)})
    # both room shapes in one call (simq_intention_maps_shapes) against the two calls it replaces: P maps of each shape, the library
    # calls alone, `blocks` blocks of `reps` back-to-back calls each, the two ways alternating block by block
    result['mixed'] = []
    rooms = ((184, 232, (0.2, 0.45)), (232, 232, (0.45, 0.45)))
    for P in [int(x) for x in args.sizes.split(',')]:
        paths, shapes = [], []
        for rows, cols, half in rooms:
            point = lambda: (rng.uniform(-half[1], half[1]), rng.uniform(-half[0], half[0]), 0.0)
            envs = [[[point() for _ in range(4)] for _ in range(4)] for _ in range((P + 3) // 4)]
            paths.append([[envs[p // 4][r] for r in range(4) if r != p % 4] for p in range(P)])
            shapes.append((rows, cols))
        two = [im._prepare(paths[k], shapes[k], 'ramp', 1.0, 2, None) for k in range(2)]
        one = im._prepare_shapes(paths[0] + paths[1], [shapes[0]] * P + [shapes[1]] * P, 'ramp', 1.0, 2, None)

        def two_calls():
            for call, _, _ in two:
                _lib.lib.call('simq_intention_maps', *call)

        def one_call():
            _lib.lib.call('simq_intention_maps_shapes', *one[0])
        for _ in range(5):
            two_calls()
            one_call()
        torch.cuda.synchronize()
        for k in range(2):                                       # the mixed call's views are the two calls' tensors
            assert all(torch.equal(v.view(torch.int32), t.view(torch.int32)) for v, t in zip(one[1][k * P:(k + 1) * P], two[k][1]))
        times = {'two_calls': [], 'one_call': []}
        for _ in range(args.blocks):
            for name, fn in (('two_calls', two_calls), ('one_call', one_call)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.reps)
        result['mixed'].append(dict({'P_per_shape': P, 'segments': one[0][1], 'blocks': args.blocks},
                                    **{'%s_ms%s' % (name, tag): round(float(f(ms)), 4) for name, ms in times.items()
                                       for tag, f in (('', np.median), ('_min', min), ('_max', max))}))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
