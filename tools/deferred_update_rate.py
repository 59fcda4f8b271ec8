"""K camera frames per mapper two ways on the GPU -- K successive BatchedMapper.update calls, and K defer calls with one flush: one JSON line.

    python tools/deferred_update_rate.py [--reps 10] [--sizes 1,8,64,256] [--frames 1,2,4,8] [--budget-s 0]

Workload: the recorded episodes (tests/golden/mapper_*.npz, rooms 184 x 232 and 232 x 232), environments of three robots replicated
until M mappers are named; frame k of mapper m is the recorded frame of round k % 3, robot m % 3 (overhead camera, 156 x 156).  Per
room, M and K, the same frames
  successive   K `update` calls of all M mappers: K uploads from pageable memory, 2 K launches, K status read-backs
  deferred     K `defer` calls of all M mappers and one `flush`: the frames copied into pinned memory, one upload per staging block,
               2 launches, one read-back
on two objects of equal construction, the two forms alternating repetition by repetition in one process.  The clock is the host's,
with the device synchronised before it starts and after the last call (both forms end in a status read-back anyway); the inputs -- the
frames as numpy arrays in lists -- exist before the clock starts.  `ms`: the median over `reps` repetitions after two warm-up
repetitions, `min` / `max` its spread; `defer_ms`: the part of `deferred` spent in the K defer calls (the copies), median.  The maps of
the two objects are compared bit for bit once per (room, M, K) before anything is timed.  --budget-s stops starting new (M, K) cells
after that many seconds and says which were left out (`skipped`); 0: no limit.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default='1,8,64,256')
    ap.add_argument('--frames', default='1,2,4,8')
    ap.add_argument('--budget-s', type=float, default=0.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('deferred_update_rate.py needs a GPU')
    import simq
    from simq.observation import CameraGeometry, IdRanges
    started = time.perf_counter()
    result = {'tool': 'deferred_update_rate', 'device': torch.cuda.get_device_name(0), 'hip': torch.version.hip, 'reps': args.reps, 'warmup': 2,
              'rooms': {}, 'skipped': []}
    for fname in ('mapper_184x232.npz', 'mapper_232x232.npz'):
        fx = oracle.load_fixture(os.path.join(ROOT, 'tests', 'golden', fname))
        masks = {name: fx['masks'][k] for k, name in enumerate(fx['mask_names'])}
        rows = {}
        for M in [int(x) for x in args.sizes.split(',')]:
            E = (M + 2) // 3
            ms = list(range(M))
            pair = [simq.BatchedMapper(fx['room_width'], fx['room_length'], [fx['types']] * E, masks, [fx['groups']] * E, fx['receptacle_position'])
                    for _ in range(2)]
            rounds = []
            for rnd in fx['rounds']:
                f = [rnd['frames'][m % 3] for m in ms]
                rounds.append(([x['depth'] for x in f], [x['ids'] for x in f], [CameraGeometry(*x['geometry']) for x in f], [IdRanges(*x['ranges']) for x in f]))

            def successive(bm, K):
                for k in range(K):
                    bm.update(*rounds[k % len(rounds)], mappers=ms)
                return 0.0

            def deferred(bm, K):
                t0 = time.perf_counter()
                for k in range(K):
                    bm.defer(*rounds[k % len(rounds)], mappers=ms)
                t1 = time.perf_counter()
                bm.flush()
                return (t1 - t0) * 1e3

            for K in [int(x) for x in args.frames.split(',')]:
                cell = '%s M=%d K=%d' % (fname[7:-4], M, K)
                if args.budget_s and time.perf_counter() - started > args.budget_s:
                    result['skipped'].append(cell)
                    continue
                for bm in pair:
                    bm.reset()
                successive(pair[0], K)
                deferred(pair[1], K)
                for kind in ('overhead', 'occupancy', 'configuration_space', 'cspace_thin', 'closest_cspace_indices'):
                    a, b = getattr(pair[0], kind), getattr(pair[1], kind)
                    assert all(torch.equal(x, y) for x, y in zip(a, b)), (cell, kind)
                times = {'successive': [], 'deferred': []}
                copies = []
                for rep in range(args.reps + 2):
                    for name, fn, bm in (('successive', successive, pair[0]), ('deferred', deferred, pair[1])):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        part = fn(bm, K)
                        torch.cuda.synchronize()
                        if rep >= 2:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                            if name == 'deferred':
                                copies.append(part)
                row = {}
                for name, t in times.items():
                    row[name] = {'ms': round(float(np.median(t)), 3), 'min': round(min(t), 3), 'max': round(max(t), 3)}
                row['deferred']['defer_ms'] = round(float(np.median(copies)), 3)
                row['speedup'] = round(row['successive']['ms'] / row['deferred']['ms'], 2)
                rows.setdefault('M=%d' % M, {})['K=%d' % K] = row
            del pair
            torch.cuda.empty_cache()
        result['rooms'][fname[7:-4]] = rows
    print(json.dumps(result))


if __name__ == '__main__':
    main()
