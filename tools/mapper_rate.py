"""Rate of simq.BatchedMapper on the GPU, beside the same work through the hand-written chain of the public functions: one JSON line.

    python tools/mapper_rate.py [--reps 10] [--sizes 1,8,64,256] [--rooms small|large|both] [--reference-ms-per-state MS] [--profile]

Workload: the two recorded episodes (tests/golden/mapper_*.npz, rooms 184 x 232 and 232 x 232), the full channel set with spatial
intention channels (9 channels), environments of three robots replicated until M = 1, 8, 64, 256 mappers are named; every repetition is
one environment step: `update` with a fresh frame per mapper, then `get_states`.  Per room and M, for the object with the robots as
lists of RobotState (`object`), for the same object with the robots as a simq.RobotArrays (`arrays`: the arrays of a round exist before
the clock starts, as they do for a caller who steps his environments in arrays; the RobotArrays is made from them inside it) and for
the chain (tests/mapper_chain.py: observation_update, occupancy_maps, a host-side snap, grid_distance_images, intention_maps three
times, local_state_images), the three alternating step by step in one process:
  host_ms      a host clock around update + get_states, each of which ends in its status read-back, so the device has finished;
               the inputs of the step (frames as numpy arrays, robot states) are formed inside the clock, as a caller forms them
  update_host_ms   the part of it up to the end of update: forming the inputs, the upload of M depth and id frames, two launches
  library_ms   the sum of the device time between a HIP event before and one after every library call of the step (the calls are
               wrapped for the measurement, the events are read after the step): the descriptor upload each entry makes on the
               launch stream and its kernel, without what the host does between the calls
  states_host_ms   host_ms without update_host_ms: get_states alone
all medians over `reps` steps after two warm-up steps; host_ms_min / host_ms_max: the spread of host_ms over those steps.  `launches`:
library launches per step.  `new_tuple`: after the steps, `reps` times one get_states of the array form with the object's plans dropped
before it (`states_host_ms`: a `mappers` tuple met for the first time) and at once the same call again (`same_tuple_again_ms`), host
clock, median and minimum / maximum -- the timed steps above all use one tuple, so none of them builds a plan.  --profile prints no timings but, per M, a cProfile breakdown by function of one get_states in the list
form and of one in the array form (room 184 x 232, after two warm-up calls; cProfile's own overhead inflates Python-heavy code).  The states of the first step are
checked against the golden (M <= 3) before anything is timed.  The reference Mapper's host time per state is what
tools/gen_mapper_golden.py prints (it needs the reference checkout); --reference-ms-per-state repeats that figure in the line
(`reference_host_ms_per_state`, null when not given): it is not measured here.
--rooms small / large times one room alone; --rooms both the two rooms in one object (both_rooms below).
"""
import argparse
import cProfile
import io
import json
import os
import pstats
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


def both_rooms(args, simq, _lib):
    """--rooms both: the two recorded episodes in one object, environments of the two rooms alternating, M = 3 * E mappers (E even).
    Per M four ways of the same step alternate in one process: the list form and the array form, each on an object that draws the maps
    of the two room shapes with one simq_intention_maps launch per shape (`per_shape`, the default) and on one made with
    one_drawing_launch=True (`one_launch`: one simq_intention_maps_shapes launch).  The fields are main()'s; host_ms_all lists the
    host_ms of every repetition."""
    from simq.observation import CameraGeometry, IdRanges
    cfg = oracle.configurations()['full_spatial']
    flags = {f: cfg[f] for f in oracle.FLAGS}
    rest = {k: v for k, v in cfg.items() if k not in oracle.FLAGS}
    fxs = [oracle.load_fixture(os.path.join(ROOT, 'tests', 'golden', f)) for f in ('mapper_184x232.npz', 'mapper_232x232.npz')]
    masks = {name: fxs[0]['masks'][k] for k, name in enumerate(fxs[0]['mask_names'])}
    n_rounds = len(fxs[0]['rounds'])
    result = {'tool': 'mapper_rate', 'rooms': 'both', 'device': torch.cuda.get_device_name(0), 'channels': len(oracle.channel_names(cfg, 3)),
              'reps': args.reps, 'rows': {}}
    for M in [int(x) for x in args.sizes.split(',')]:
        E = max(2, 2 * ((M + 5) // 6))
        M = 3 * E
        ms = list(range(M))
        of = [fxs[e % 2] for e in range(E)]
        objects = {name: simq.BatchedMapper([f['room_width'] for f in of], [f['room_length'] for f in of], [f['types'] for f in of], masks,
                                            [f['groups'] for f in of], [f['receptacle_position'] for f in of], **flags, **rest,
                                            one_drawing_launch=flag) for name, flag in (('per_shape', False), ('one_launch', True))}

        def step_inputs(t):
            rnds = [f['rounds'][t % n_rounds] for f in of]
            f = [rnds[m // 3]['frames'][m % 3] for m in ms]
            frames = ([x['depth'] for x in f], [x['ids'] for x in f], [CameraGeometry(*x['geometry']) for x in f], [IdRanges(*x['ranges']) for x in f])
            states = [[simq.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'],
                                       r['history_path']) for r in rnd['robots']] for rnd in rnds]
            return frames, states

        arrays = {}
        for t in range(n_rounds):
            ra = simq.RobotArrays.from_states(objects['per_shape'], step_inputs(t)[1])
            arrays[t] = (ra.position, ra.heading, ra.lifting, ra.idle, ra.target, ra.intention_path, ra.history_path)
        split = []

        def step(bm, as_arrays):
            def run(t):
                frames, states = step_inputs(t)
                bm.update(*frames, mappers=ms)
                split.append(time.perf_counter())
                return bm.get_states(simq.RobotArrays(*arrays[t % n_rounds]) if as_arrays else states, mappers=ms)
            return run
        forms = [('%s_%s' % (form, name), step(bm, form == 'arrays')) for form in ('object', 'arrays') for name, bm in objects.items()]
        first = [run(0) for _, run in forms]
        want = np.stack([oracle.expected_state(cfg, of[m // 3]['rounds'][0]['images'], m % 3, 3) for m in ms])
        for got in first:
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), M
        taken = {name: ([], [], [], []) for name, _ in forms}
        with LibraryClock(_lib.lib) as clock:
            for t in range(1, 3 + args.reps):
                for name, run in forms:                              # the forms alternate step by step
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(t)
                    torch.cuda.synchronize()
                    dt = 1e3 * (time.perf_counter() - t0)
                    ms_lib, launches = clock.take()
                    if t >= 3:
                        host, library, update, counts = taken[name]
                        host.append(dt)
                        library.append(ms_lib)
                        update.append(1e3 * (split[-1] - t0))
                        counts.append(launches)
        row = {}
        for name, (host, library, update, counts) in taken.items():
            states = np.asarray(host) - np.asarray(update)
            row[name] = {'host_ms': round(float(np.median(host)), 3), 'host_ms_min': round(min(host), 3), 'host_ms_max': round(max(host), 3),
                         'states_host_ms': round(float(np.median(states)), 3), 'states_host_ms_min': round(float(states.min()), 3),
                         'states_host_ms_max': round(float(states.max()), 3), 'library_ms': round(float(np.median(library)), 3),
                         'library_ms_min': round(min(library), 3), 'library_ms_max': round(max(library), 3), 'launches': counts[-1],
                         'host_ms_all': [round(x, 3) for x in host]}
        result['rows'][str(M)] = row
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default=None, help='the numbers of mappers (default 1,8,64,256; with --rooms both 6,48,192)')
    ap.add_argument('--rooms', choices=('small', 'large', 'both'), default=None,
                    help='small / large: the 184 x 232 / 232 x 232 room alone; both: the two rooms in one object, its drawn maps with one launch '
                         'per room shape and with one launch for both (one_drawing_launch); omitted: each room on its own, one after the other')
    ap.add_argument('--reference-ms-per-state', type=float, default=None,
                    help='the host time per state tools/gen_mapper_golden.py printed for the reference Mapper, repeated in the line')
    ap.add_argument('--profile', action='store_true', help='print a cProfile breakdown of one get_states per form and M instead of the timings')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mapper_rate.py needs a GPU')
    import simq
    from simq import _lib
    from simq.observation import CameraGeometry, IdRanges
    if args.sizes is None:
        args.sizes = '6,48,192' if args.rooms == 'both' else '1,8,64,256'
    if args.rooms == 'both':
        if args.profile:
            raise SystemExit('--profile is for one room at a time')
        return both_rooms(args, simq, _lib)
    cfg = oracle.configurations()['full_spatial']
    flags = {f: cfg[f] for f in oracle.FLAGS}
    rest = {k: v for k, v in cfg.items() if k not in oracle.FLAGS}
    result = {'tool': 'mapper_rate', 'device': torch.cuda.get_device_name(0), 'channels': len(oracle.channel_names(cfg, 3)), 'reps': args.reps,
              'reference_host_ms_per_state': args.reference_ms_per_state, 'rooms': {}}
    for fname in {'small': ('mapper_184x232.npz',), 'large': ('mapper_232x232.npz',)}.get(args.rooms, ('mapper_184x232.npz', 'mapper_232x232.npz')):
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

            arrays = {}                                              # the robots of a round as arrays, made once: what an array caller holds

            def step_inputs(t):
                rnd = rounds[t % len(rounds)]
                f = [rnd['frames'][m % 3] for m in ms]
                frames = ([x['depth'] for x in f], [x['ids'] for x in f], [CameraGeometry(*x['geometry']) for x in f], [IdRanges(*x['ranges']) for x in f])
                states = [[simq.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'],
                                           r['history_path']) for r in rnd['robots']]] * E
                return frames, states, [rnd['robots']] * E

            for t in range(len(rounds)):
                ra = simq.RobotArrays.from_states(bm, step_inputs(t)[1])
                arrays[t] = (ra.position, ra.heading, ra.lifting, ra.idle, ra.target, ra.intention_path, ra.history_path)

            split = []                                               # host clock after the update of the last step (it ends in a read-back)

            def object_step(t):
                frames, states, _ = step_inputs(t)
                bm.update(*frames, mappers=ms)
                split.append(time.perf_counter())
                return bm.get_states(states, mappers=ms)

            def arrays_step(t):
                frames, _, _ = step_inputs(t)
                bm.update(*frames, mappers=ms)
                split.append(time.perf_counter())
                return bm.get_states(simq.RobotArrays(*arrays[t % len(rounds)]), mappers=ms)

            def chain_step(t):
                frames, _, envs = step_inputs(t)
                chain.update(*frames, mappers=ms)
                split.append(time.perf_counter())
                return chain.get_states(cfg, envs, mappers=ms)['states']

            # the first step against the golden, and the three ways against each other
            a, b, c = object_step(0), chain_step(0), arrays_step(0)
            assert torch.equal(a, b) and torch.equal(a, c), (fname, M)
            want = np.stack([oracle.expected_state(cfg, rounds[0]['images'], m % 3, 3) for m in ms])
            assert np.array_equal(a.cpu().numpy().view(np.int32), want.view(np.int32)), (fname, M)
            if args.profile:
                if fname.startswith('mapper_184'):
                    for form, robots in (('list form', step_inputs(1)[1]), ('array form', simq.RobotArrays(*arrays[1]))):
                        for _ in range(2):
                            bm.get_states(robots, mappers=ms)
                        prof = cProfile.Profile()
                        prof.enable()
                        bm.get_states(robots, mappers=ms)
                        prof.disable()
                        text = io.StringIO()
                        pstats.Stats(prof, stream=text).sort_stats('tottime').print_stats(14)
                        print('---- M = %d, %s: one get_states by function (tottime)' % (M, form))
                        print('\n'.join(line for line in text.getvalue().splitlines() if line.strip())[:6000])
                continue
            forms = (('object', object_step), ('arrays', arrays_step), ('chain', chain_step))
            taken = {name: ([], [], [], []) for name, _ in forms}
            with LibraryClock(_lib.lib) as clock:
                for t in range(1, 3 + args.reps):
                    for name, step in forms:                         # the forms alternate step by step
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        step(t)
                        torch.cuda.synchronize()
                        dt = 1e3 * (time.perf_counter() - t0)
                        ms_lib, launches = clock.take()
                        if t >= 3:
                            host, library, update, counts = taken[name]
                            host.append(dt)
                            library.append(ms_lib)
                            update.append(1e3 * (split[-1] - t0))
                            counts.append(launches)
            # the array form with a `mappers` tuple the object has no plan for, beside the same call again: what a caller pays whose
            # tuple changes from step to step (the object keeps the plans of eight tuples; here they are dropped before the call)
            robots, miss, hit = simq.RobotArrays(*arrays[0]), [], []
            for _ in range(args.reps):
                for times in (miss, hit):
                    if times is miss:
                        bm._plans.clear()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    bm.get_states(robots, mappers=ms)
                    torch.cuda.synchronize()
                    times.append(1e3 * (time.perf_counter() - t0))
            row = {'new_tuple': {'states_host_ms': round(float(np.median(miss)), 3), 'states_host_ms_min': round(min(miss), 3),
                                 'states_host_ms_max': round(max(miss), 3), 'same_tuple_again_ms': round(float(np.median(hit)), 3),
                                 'same_tuple_again_ms_min': round(min(hit), 3), 'same_tuple_again_ms_max': round(max(hit), 3)}}
            for name, (host, library, update, counts) in taken.items():
                row[name] = {'host_ms': round(float(np.median(host)), 3), 'host_ms_min': round(min(host), 3), 'host_ms_max': round(max(host), 3),
                             'update_host_ms': round(float(np.median(update)), 3),
                             'states_host_ms': round(float(np.median(np.asarray(host) - np.asarray(update))), 3),
                             'library_ms': round(float(np.median(library)), 3), 'launches': counts[-1],
                             'host_ms_per_state': round(float(np.median(host)) / M, 4)}
            rows[str(M)] = row
        result['rooms'][fname[len('mapper_'):-4]] = rows
    if not args.profile:
        print(json.dumps(result))


if __name__ == '__main__':
    main()
