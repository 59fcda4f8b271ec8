"""Rate of simq_local_state_images on the GPU: one JSON line with per-launch latency and states/s.

    python tools/local_maps_rate.py [--reps 20]

Workload: the 4-channel state of BASELINE configs[1] (overhead map, robot map, shortest path to the receptacle, shortest path from the
robot) for P = 1, 8, 64, 256 robots per launch in both room sizes (184 x 232 and 232 x 232 global maps); four robots per environment,
every robot one problem, each environment with its own overhead map and receptacle image and each robot with its own distance image,
all resident on the device as simq.grid_distance_images leaves them.  `ms_per_launch`: HIP events around `reps` back-to-back library
calls after a warm-up -- the descriptor upload the C-ABI makes on the launch stream included, the Python side's descriptor building
(rotation matrices from scipy.special) not; `host_ms_per_call`: wall time of simq.local_state_images itself, device-synchronised.
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='1,8,64,256')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('local_maps_rate.py needs a GPU')
    import simq
    from simq import _lib, local_maps as lm
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(0)
    masks = np.zeros((2, 96, 96), np.float32)
    masks[0, 42:54, 43:53] = 1
    masks[1, 36:54, 43:53] = 1
    result = {'metric': 'local_state_images', 'unit': 'ms per launch / states per s', 'channels': 4, 'reps': args.reps, 'rows': []}
    for rows, cols, half in ((184, 232, (0.2, 0.45)), (232, 232, (0.45, 0.45))):
        for P in [int(x) for x in args.sizes.split(',')]:
            n_env = (P + 3) // 4
            overhead = torch.rand(n_env, rows, cols, device=dev) * 0.5
            to_receptacle = torch.rand(n_env, rows, cols, device=dev)
            from_robot = torch.rand(P, rows, cols, device=dev)
            maps = list(overhead) + list(to_receptacle) + list(from_robot)
            envs = [[lm.RobotStamp((rng.uniform(-half[1], half[1]), rng.uniform(-half[0], half[0])), rng.uniform(-math.pi, math.pi), r % 2,
                                   0.625 + 0.125 * (r % 2), 1.0, 0) for r in range(4)] for _ in range(n_env)]
            poses = [(envs[p // 4][p % 4].position, envs[p // 4][p % 4].heading) for p in range(P)]
            robots = [envs[p // 4] for p in range(P)]
            channels = [[('overhead', p // 4), 'robots', ('distance', n_env + p // 4), ('distance', 2 * n_env + p)] for p in range(P)]
            d_masks = torch.from_numpy(masks).to(dev)
            check = simq.local_state_images(maps, channels, poses, robots=robots, masks=d_masks)
            call, out, keep = lm._prepare(maps, channels, poses, robots, d_masks, None, None)
            for _ in range(3):
                _lib.lib.call('simq_local_state_images', *call)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), check.view(torch.int32))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                _lib.lib.call('simq_local_state_images', *call)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.reps
            t0 = time.perf_counter()
            for _ in range(5):
                simq.local_state_images(maps, channels, poses, robots=robots, masks=d_masks, out=out)
            torch.cuda.synchronize()
            host_ms = 1e3 * (time.perf_counter() - t0) / 5
            result['rows'].append({'maps': [rows, cols], 'P': P, 'ms_per_launch': round(ms, 4), 'us_per_state': round(1e3 * ms / P, 3),
                                   'states_per_s': round(P / ms * 1e3, 1), 'host_ms_per_call': round(host_ms, 3)})
    print(json.dumps(result))


if __name__ == '__main__':
    main()
