"""Rate of simq.BatchedMapper on the GPU, beside the same work through the hand-written chain of the public functions: one JSON line.

    python tools/mapper_rate.py [--reps 10] [--sizes 1,8,64,256] [--reference-ms-per-state MS]

Workload: the two recorded episodes (tests/golden/mapper_*.npz, rooms 184 x 232 and 232 x 232), the full channel set with spatial
intention channels (9 channels), environments of three robots replicated until M = 1, 8, 64, 256 mappers are named; every repetition is
one environment step: `update` with a fresh frame per mapper, then `get_states`.  Per room and M, for the object and for the chain
(tests/mapper_chain.py: observation_update, occupancy_maps, a host-side snap, grid_distance_images, intention_maps three times,
local_state_images):
  host_ms      a host clock around update + get_states, each of which ends in its status read-back, so the device has finished;
               the inputs of the step (frames as numpy arrays, robot states) are formed inside the clock, as a caller forms them
  update_host_ms   the part of it up to the end of update: forming the inputs, the upload of M depth and id frames, two launches
  library_ms   the sum of the device time between a HIP event before and one after every library call of the step (the calls are
               wrapped for the measurement, the events are read after the step): the descriptor upload each entry makes on the
               launch stream and its kernel, without what the host does between the calls
both the median over `reps` steps after two warm-up steps.  `launches`: library launches per step.  The states of the first step are
checked against the golden (M <= 3) before anything is timed.  The reference Mapper's host time per state is what
tools/gen_mapper_golden.py prints (it needs the reference checkout); --reference-ms-per-state repeats that figure in the line
(`reference_host_ms_per_state`, null when not given): it is not measured here.
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

import mapper_oracle as oracle  # noqa: E402
from mapper_chain import Chain  # noqa: E402


class LibraryClock:
    """Wraps lib.call: a HIP event before and after every library call on the current stream."""

    def __init__(self, lib):
        self.lib, self.real, self.spans = lib, lib.call, []

    def __enter__(self):
        def timed(name, *args, **kw):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.real(name, *args, **kw)
            b.record()
            self.spans.append((name, a, b))
        self.lib.call = timed
        return self

    def __exit__(self, *exc):
        del self.lib.call                                            # (the instance attribute: the class's static method is back)
        return False

    def take(self):
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for _, a, b in self.spans)
        n = len(self.spans)
        self.spans = []
        return ms, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default='1,8,64,256')
    ap.add_argument('--reference-ms-per-state', type=float, default=None,
                    help='the host time per state tools/gen_mapper_golden.py printed for the reference Mapper, repeated in the line')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mapper_rate.py needs a GPU')
    import simq
    from simq import _lib
    from simq.observation import CameraGeometry, IdRanges
    cfg = oracle.configurations()['full_spatial']
    flags = {f: cfg[f] for f in oracle.FLAGS}
    rest = {k: v for k, v in cfg.items() if k not in oracle.FLAGS}
    result = {'tool': 'mapper_rate', 'device': torch.cuda.get_device_name(0), 'channels': len(oracle.channel_names(cfg, 3)), 'reps': args.reps,
              'reference_host_ms_per_state': args.reference_ms_per_state, 'rooms': {}}
    for fname in ('mapper_184x232.npz', 'mapper_232x232.npz'):
        fx = oracle.load_fixture(os.path.join(ROOT, 'tests', 'golden', fname))
        masks = {name: fx['masks'][k] for k, name in enumerate(fx['mask_names'])}
        rounds = fx['rounds']
        rows = {}
        for M in [int(x) for x in args.sizes.split(',')]:
            E = (M + 2) // 3
            ms = list(range(M))
            bm = simq.BatchedMapper(fx['room_width'], fx['room_length'], [fx['types']] * E, masks, [fx['groups']] * E, fx['receptacle_position'],
                                    **flags, **rest)
            chain = Chain(simq, fx['room_width'], fx['room_length'], [fx['types']] * E, fx['masks'], fx['mask_names'], fx['receptacle_position'])

            def step_inputs(t):
                rnd = rounds[t % len(rounds)]
                f = [rnd['frames'][m % 3] for m in ms]
                frames = ([x['depth'] for x in f], [x['ids'] for x in f], [CameraGeometry(*x['geometry']) for x in f], [IdRanges(*x['ranges']) for x in f])
                states = [[simq.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'],
                                           r['history_path']) for r in rnd['robots']]] * E
                return frames, states, [rnd['robots']] * E

            split = []                                               # host clock after the update of the last step (it ends in a read-back)

            def object_step(t):
                frames, states, _ = step_inputs(t)
                bm.update(*frames, mappers=ms)
                split.append(time.perf_counter())
                return bm.get_states(states, mappers=ms)

            def chain_step(t):
                frames, _, envs = step_inputs(t)
                chain.update(*frames, mappers=ms)
                split.append(time.perf_counter())
                return chain.get_states(cfg, envs, mappers=ms)['states']

            # the first step against the golden, and the two ways against each other
            a, b = object_step(0), chain_step(0)
            assert torch.equal(a, b), (fname, M)
            want = np.stack([oracle.expected_state(cfg, rounds[0]['images'], m % 3, 3) for m in ms])
            assert np.array_equal(a.cpu().numpy().view(np.int32), want.view(np.int32)), (fname, M)
            row = {}
            for name, step in (('object', object_step), ('chain', chain_step)):
                host, library, update, launches = [], [], [], 0
                with LibraryClock(_lib.lib) as clock:
                    for t in range(1, 3 + args.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        step(t)
                        torch.cuda.synchronize()
                        dt = 1e3 * (time.perf_counter() - t0)
                        ms_lib, launches = clock.take()
                        if t >= 3:
                            host.append(dt)
                            library.append(ms_lib)
                            update.append(1e3 * (split[-1] - t0))
                row[name] = {'host_ms': round(float(np.median(host)), 3), 'update_host_ms': round(float(np.median(update)), 3),
                             'library_ms': round(float(np.median(library)), 3), 'launches': launches,
                             'host_ms_per_state': round(float(np.median(host)) / M, 4)}
            rows[str(M)] = row
        result['rooms'][fname[len('mapper_'):-4]] = rows
    print(json.dumps(result))


if __name__ == '__main__':
    main()
