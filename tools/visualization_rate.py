"""Rate of simq_state_output_visualizations on the GPU: one JSON line with per-launch latency and images/s.

    python tools/visualization_rate.py [--reps 20]

Workload: the image of train.py:292-304 for a 4-channel state and a 2-channel Q-map (BASELINE configs[1]), [96, 290, 3] fp32, for
P = 1, 8, 64 (state, output) pairs per launch, states and Q-maps resident on the device.  `ms_per_launch`: HIP events around `reps`
back-to-back library calls after a warm-up -- the descriptor upload the C-ABI makes on the launch stream included;
`host_ms_per_call`: wall time of simq.state_output_visualizations itself, device-synchronised.  No threshold: the tool reports.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='1,8,64')
    ap.add_argument('--channels', type=int, default=4)
    ap.add_argument('--outputs', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('visualization_rate.py needs a GPU')
    import simq
    from simq import _lib, visualization as vz
    dev = torch.device('cuda', 0)
    # a stand-in colour map (a ramp): the rate does not depend on the table, and matplotlib need not be installed to measure
    jet = torch.from_numpy(np.repeat(np.linspace(0, 1, 256, dtype=np.float32)[:, None], 3, axis=1)).to(dev)
    result = {'metric': 'state_output_visualizations', 'unit': 'ms per launch / images per s', 'channels': args.channels,
              'outputs': args.outputs, 'image': [96, vz.image_width(args.outputs), 3], 'reps': args.reps, 'rows': []}
    for P in [int(x) for x in args.sizes.split(',')]:
        states = torch.rand(P, 96, 96, args.channels, device=dev)
        outputs = torch.randn(P, args.outputs, 96, 96, device=dev)
        check = simq.state_output_visualizations(states, outputs, jet=jet)
        call, out, keep = vz._prepare(states, outputs, jet, 0.5, False, None)
        for _ in range(3):
            _lib.lib.call('simq_state_output_visualizations', *call)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), check.view(torch.int32))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            _lib.lib.call('simq_state_output_visualizations', *call)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        t0 = time.perf_counter()
        for _ in range(5):
            simq.state_output_visualizations(states, outputs, jet=jet, out=out)
        torch.cuda.synchronize()
        host_ms = 1e3 * (time.perf_counter() - t0) / 5
        result['rows'].append({'P': P, 'ms_per_launch': round(ms, 4), 'us_per_image': round(1e3 * ms / P, 3),
                               'images_per_s': round(P / ms * 1e3, 1), 'host_ms_per_call': round(host_ms, 3)})
        del keep
    print(json.dumps(result))


if __name__ == '__main__':
    main()
