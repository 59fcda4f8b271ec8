"""Actions to waypoints for P deciding robots, the route that was possible before and `store_new_actions`: one JSON line.

    python tools/store_new_action_rate.py [--reps 10] [--sizes 1,8,64,256] [--room 184x232]

Two routes run in one process, on the same commit, alternating repetition by repetition:
  pair     `BatchedMapper.shortest_paths(positions, targets, simplify='exact')` -- simq_grid_paths and simq_grid_waypoints on packed
           copies of the maps, the boxes reduced and read back -- with Robot.store_new_action's scalar Python around it per robot
  arrays   `BatchedMapper.store_new_actions(actions, RobotArrays)`: one simq_action_waypoints launch on the maps where they lie
Workload: collect_rate.py's -- a recorded episode (tests/golden/mapper_*.npz), environments of three robots replicated until P = 1, 8,
64, 256 robots decide, `update` once before the clock, the robots' poses following the recorded rounds -- with seeded actions.  Per P
and route: host_ms, a host clock around the call with the device synchronised at both ends, the median over `reps` calls after two
warm-up calls with its minimum and maximum, and the number of library calls of one call.  Before anything is timed the two routes are
checked against each other, bit for bit.
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import mapper_oracle as oracle  # noqa: E402

ROUTES = ('pair', 'arrays')


def restrict_heading_range(h):
    return (h + math.pi) % (2 * math.pi) - math.pi


def pair_route(bm, arch, actions, states, ms):
    """Robot.store_new_action (envs.py:856-902) robot by robot around one batched shortest_paths call."""
    own = [(bm.env_of[m], m - bm.env_begin[bm.env_of[m]]) for m in ms]
    out, targets = [], []
    for a, (e, r) in zip(actions, own):
        s, t = states[e][r], bm.robot_types[e][r]
        action = tuple(np.unravel_index(a, (arch.get_num_output_channels(t), arch.STATE_WIDTH, arch.STATE_WIDTH)))
        dx = ((action[2] + 0.5) - arch.STATE_WIDTH / 2) / arch.LOCAL_MAP_PIXELS_PER_METER
        dy = (arch.STATE_WIDTH / 2 - (action[1] + 0.5)) / arch.LOCAL_MAP_PIXELS_PER_METER
        dist = math.sqrt(dx**2 + dy**2)
        theta = s.heading + math.atan2(-dx, dy)
        targets.append((s.position[0] + dist * math.cos(theta), s.position[1] + dist * math.sin(theta), 0))
        out.append([tuple(int(x) for x in action), targets[-1]])
    paths = bm.shortest_paths([states[e][r].position for e, r in own], targets, mappers=ms, simplify='exact')
    for (e, r), way, o in zip(own, paths, out):
        s, t = states[e][r], bm.robot_types[e][r]
        headings = [s.heading]
        for i in range(1, len(way)):
            headings.append(restrict_heading_range(math.atan2(way[i][1] - way[i - 1][1], way[i][0] - way[i - 1][0])))
        signed_dist = math.sqrt((way[-1][0] - way[-2][0])**2 + (way[-1][1] - way[-2][1])**2) - (arch.get_end_effector_location(t) + arch.CUBE_WIDTH / 2)
        way[-1] = (way[-2][0] + signed_dist * math.cos(headings[-1]), way[-2][1] + signed_dist * math.sin(headings[-1]), 0)
        if len(way) > 2 and signed_dist < 0:
            way[-2] = way[-1]
            headings[-2] = restrict_heading_range(math.atan2(way[-2][1] - way[-3][1], way[-2][0] - way[-3][0]))
        o += [way, headings]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default='1,8,64,256')
    ap.add_argument('--room', default='184x232', choices=('184x232', '232x232'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('store_new_action_rate.py needs a GPU')
    import simq
    from simq import arch
    from simq._lib import Lib
    from simq.observation import CameraGeometry, IdRanges
    fx = oracle.load_fixture(os.path.join(ROOT, 'tests', 'golden', 'mapper_%s.npz' % args.room))
    masks = {name: fx['masks'][k] for k, name in enumerate(fx['mask_names'])}
    calls = []
    call = Lib.call
    Lib.call = staticmethod(lambda name, *a, **k: calls.append(name) or call(name, *a, **k))
    result = {'tool': 'store_new_action_rate', 'device': torch.cuda.get_device_name(0), 'room': args.room, 'reps': args.reps, 'sizes': {}}
    rng = np.random.RandomState(11)
    for P in [int(x) for x in args.sizes.split(',')]:
        E = (P + 2) // 3
        bm = simq.BatchedMapper(fx['room_width'], fx['room_length'], [fx['types']] * E, masks, [fx['groups']] * E, fx['receptacle_position'])
        frames = [fx['rounds'][0]['frames'][m % 3] for m in range(bm.num_mappers)]
        bm.update([f['depth'] for f in frames], [f['ids'] for f in frames], [CameraGeometry(*f['geometry']) for f in frames],
                  [IdRanges(*f['ranges']) for f in frames])
        ms = list(range(P))
        rounds = []
        for rnd in fx['rounds']:
            states = [[simq.RobotState(tuple(float(x) for x in r['position'][:2]) + (0,), float(r['heading']), r['type']) for r in rnd['robots']]] * E
            ra = simq.RobotArrays.from_states(bm, states)
            rounds.append((states, (ra.position, ra.heading)))
        channels = [arch.get_num_output_channels(fx['types'][m % 3]) for m in ms]
        times, n_calls, traced = {r: [] for r in ROUTES}, {}, 0
        for t in range(args.reps + 2):                                   # two warm-up calls, then `reps`; the routes alternate
            states, arrays = rounds[t % len(rounds)]
            actions = [int(rng.randint(c * arch.STATE_WIDTH * arch.STATE_WIDTH)) for c in channels]
            got = {}
            for route in ROUTES:
                del calls[:]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if route == 'pair':
                    got[route] = pair_route(bm, arch, actions, states, ms)
                else:
                    new = bm.store_new_actions(actions, simq.RobotArrays(*arrays), mappers=ms)
                torch.cuda.synchronize()
                dt = 1e3 * (time.perf_counter() - t0)
                if t >= 2:
                    times[route].append(dt)
                n_calls[route] = max(n_calls.get(route, 0), len(calls))
            lists = new.as_lists()
            for p in range(P):                                          # the routes against each other, every call
                assert list(lists[p][0]) == list(got['pair'][p][0]) and lists[p][1] == got['pair'][p][1], (P, t, p)
                assert lists[p][2] == got['pair'][p][2] and lists[p][3] == got['pair'][p][3], (P, t, p)
            traced += int((new.status == 0).sum())
        result['sizes'][str(P)] = {route: {'host_ms': round(float(np.median(h)), 3), 'host_ms_min': round(min(h), 3), 'host_ms_max': round(max(h), 3),
                                           'lib_calls': n_calls[route]} for route, h in times.items()}
        result['sizes'][str(P)]['traced_share'] = round(traced / (P * (args.reps + 2)), 3)
        del bm
    print(json.dumps(result))


if __name__ == '__main__':
    main()
