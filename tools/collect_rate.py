"""One collection step with the states on the host in between, and with the states left in the replay pool: one JSON line.

    python tools/collect_rate.py [--reps 10] [--sizes 1,8,64,256] [--room 184x232]

A collection step is what a worker that owns E environments does between two environment steps: `BatchedMapper.get_states` for the M
deciding robots, `DQNPolicy.step_many` on their states, and the `push` of the M transitions that `TransitionTracker` completes.  Four
forms of it run in one process, on the same commit, in alternating repetitions:
  host     get_states -> .cpu().numpy() -> the ndarrays through the tracker, step_many and push (every state crosses the bus twice:
           down after the mapper, up again at push -- and once more for the policy's batch)
  handles  per robot group `h = ring.reserve(P)`, get_states(into=h), the handles through the tracker, step_many and push: the states
           are written where they are sampled from and never leave the device.  One get_states call per robot
           group, because a call writes into one pool and every group has its ring.
  arrays   the handles form with the robots handed to get_states as a simq.RobotArrays instead of lists of
           RobotState; the arrays of a round exist before the clock starts, the RobotArrays is made from them inside it
  pools    the handles form with ONE get_states(into=, pools=rings) per step over all deciding robots: handle p
           comes from the ring of robot p's group, and the states of all groups are written by one chain of launches
Workload: a recorded episode (tests/golden/mapper_*.npz), the full channel set with spatial intention channels (9 channels),
environments of three robots in two robot groups replicated until M = 1, 8, 64, 256 robots decide.  `update` runs once before the
clock; the maps do not change between the steps, the robots' poses follow the recorded rounds.  Per M and form:
  host_ms    a host clock around the step, the device synchronised at both ends
  event_ms   the time between a HIP event recorded on the stream before the step's first call and one after its last
both the median over `reps` steps after two warm-up steps, host_ms with its minimum and maximum over those steps.  Before anything is
timed the forms are checked against each other: the same actions under one seed, and the pool rows of the handles equal to the host
states bit for bit.
"""
import argparse
import json
import os
import random
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import mapper_oracle as oracle  # noqa: E402


FORMS = ('host', 'handles', 'arrays', 'pools')


class Worker:
    """E environments of one room, their BatchedMapper, one policy and per form one ring per robot group and one tracker per environment."""

    def __init__(self, simq, fx, M, policy):
        from simq.observation import CameraGeometry, IdRanges
        self.simq, self.fx, self.M, self.policy = simq, fx, M, policy
        self.E = (M + 2) // 3
        cfg = oracle.configurations()['full_spatial']
        masks = {name: fx['masks'][k] for k, name in enumerate(fx['mask_names'])}
        self.bm = simq.BatchedMapper(fx['room_width'], fx['room_length'], [fx['types']] * self.E, masks, [fx['groups']] * self.E,
                                     fx['receptacle_position'], **{f: cfg[f] for f in oracle.FLAGS},
                                     **{k: v for k, v in cfg.items() if k not in oracle.FLAGS})
        self.C = self.bm.num_channels
        self.groups = sorted(set(fx['groups']))
        self.members = {g: [r for r, x in enumerate(fx['groups']) if x == g] for g in self.groups}      # robots of a group, in env.robots' order
        self.deciding = list(range(M))                                                                # mapper m = (environment m // 3, robot m % 3)
        frames = [fx['rounds'][0]['frames'][m % 3] for m in range(self.bm.num_mappers)]
        self.bm.update([f['depth'] for f in frames], [f['ids'] for f in frames], [CameraGeometry(*f['geometry']) for f in frames],
                       [IdRanges(*f['ranges']) for f in frames])
        capacity = max(64, 2 * M)
        self.rings = {form: [simq.AliasedDeviceReplayBuffer(capacity, self.C, pool_slots=2 * capacity + M + 16) for _ in self.groups]
                      for form in FORMS}
        self.trackers = {form: None for form in FORMS}
        self.arrays = []                                              # the robots of every recorded round as arrays, made once
        for t in range(len(fx['rounds'])):
            ra = simq.RobotArrays.from_states(self.bm, self.robot_states(t))
            self.arrays.append((ra.position, ra.heading, ra.lifting, ra.idle, ra.target, ra.intention_path, ra.history_path))
        self.rng = np.random.RandomState(7)

    def robot_states(self, t):
        rnd = self.fx['rounds'][t % len(self.fx['rounds'])]
        return [[self.simq.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'],
                                      r['history_path']) for r in rnd['robots']]] * self.E

    def nested(self, of_mapper):
        """[environment][group][robot of the group]: of_mapper[m] for a deciding robot, None for the others (VectorEnv.get_state's shape)."""
        return [[[of_mapper.get(3 * e + r) for r in self.members[g]] for g in self.groups] for e in range(self.E)]

    def states_host(self, t):
        host = self.bm.get_states(self.robot_states(t), mappers=self.deciding).cpu().numpy()
        return self.nested({m: host[p] for p, m in enumerate(self.deciding)})

    def states_handles(self, t, form='handles'):
        of_mapper = {}
        robots = self.robot_states(t) if form == 'handles' else self.simq.RobotArrays(*self.arrays[t % len(self.arrays)])
        for i, g in enumerate(self.groups):
            mine = [m for m in self.deciding if self.fx['groups'][m % 3] == g]
            if mine:
                handles = self.bm.get_states(robots, mappers=mine, into=self.rings[form][i].reserve(len(mine)))
                of_mapper.update(zip(mine, handles))
        return self.nested(of_mapper)

    def states_pools(self, t):
        rings = self.rings['pools']
        group_of = [self.fx['groups'][m % 3] for m in self.deciding]
        reserved = {g: iter(rings[i].reserve(group_of.count(g))) for i, g in enumerate(self.groups)}
        handles = [next(reserved[g]) for g in group_of]
        self.bm.get_states(self.robot_states(t), mappers=self.deciding, into=handles, pools=rings)
        return self.nested(dict(zip(self.deciding, handles)))

    def step(self, form, t, eps=0.1):
        """get_states, step_many, push of the completed transitions; returns (states, actions)."""
        states = self.states_host(t) if form == 'host' else self.states_pools(t) if form == 'pools' else self.states_handles(t, form)
        actions = self.policy.step_many(states, exploration_eps=eps)
        if self.trackers[form] is None:                               # the first step of an episode completes no transition
            self.trackers[form] = [self.simq.TransitionTracker(st) for st in states]
        else:
            for e, tracker in enumerate(self.trackers[form]):
                reward = [[0.25 for _ in g] for g in states[e]]
                for i, transitions in enumerate(tracker.update_step_completed(reward, states[e], False)):
                    for transition in transitions:
                        self.rings[form][i].push(*transition)
        for e, tracker in enumerate(self.trackers[form]):
            tracker.update_action(actions[e])
        return states, actions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default='1,8,64,256')
    ap.add_argument('--room', default='184x232', choices=('184x232', '232x232'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('collect_rate.py needs a GPU')
    import simq
    fx = oracle.load_fixture(os.path.join(ROOT, 'tests', 'golden', 'mapper_%s.npz' % args.room))
    C = len(oracle.channel_names(oracle.configurations()['full_spatial'], 3))
    types_of = [fx['types'][fx['groups'].index(g)] for g in sorted(set(fx['groups']))]
    cfg = types.SimpleNamespace(robot_config=[{t: fx['groups'].count(g)} for g, t in zip(sorted(set(fx['groups'])), types_of)],
                                num_input_channels=C, final_exploration=0.01, checkpoint_path=None)
    policy = simq.DQNPolicy(cfg, train=False, random_seed=1)
    for net in policy.policy_nets:
        net.eval()
    result = {'tool': 'collect_rate', 'device': torch.cuda.get_device_name(0), 'room': args.room, 'channels': C, 'reps': args.reps,
              'state_mbytes_each_way': {}, 'sizes': {}}
    for M in [int(x) for x in args.sizes.split(',')]:
        w = Worker(simq, fx, M, policy)
        result['state_mbytes_each_way'][str(M)] = round(M * 96 * 96 * C * 4 / 1e6, 2)
        # the two forms against each other, before any clock: step 0 starts the episode, step 1 pushes M transitions
        for t in (0, 1):
            random.seed(100 + t)
            host_states, host_actions = w.step('host', t)
            for form in FORMS[1:]:
                random.seed(100 + t)
                pool_states, pool_actions = w.step(form, t)
                assert pool_actions == host_actions, (M, t, form)
                for a, b in zip((s for st in host_states for g in st for s in g), (s for st in pool_states for g in st for s in g)):
                    assert (a is None) == (b is None) and (a is None or np.array_equal(a.view(np.int32), np.asarray(b).view(np.int32))), (M, t, form)
        assert all([len(r) for r in w.rings['host']] == [len(r) for r in w.rings[form]] for form in FORMS) and sum(len(r) for r in w.rings['host']) == M
        del host_states, pool_states                                  # (the handles of the form checked last would hold their slots to the end)
        times = {form: ([], []) for form in FORMS}
        for t in range(2, 4 + args.reps):                             # two warm-up steps, then `reps`; the forms alternate
            for form in FORMS:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                w.step(form, t)
                b.record()
                torch.cuda.synchronize()
                dt = 1e3 * (time.perf_counter() - t0)
                if t >= 4:
                    times[form][0].append(dt)
                    times[form][1].append(a.elapsed_time(b))
        for form in FORMS:
            for ring in w.rings[form]:
                ring.sync_ring()
        result['sizes'][str(M)] = {form: {'host_ms': round(float(np.median(h)), 3), 'host_ms_min': round(min(h), 3), 'host_ms_max': round(max(h), 3),
                                          'event_ms': round(float(np.median(e)), 3)} for form, (h, e) in times.items()}
        result['sizes'][str(M)]['resident'] = {form: [r.observations_resident for r in w.rings[form]] for form in FORMS}
        del w
    print(json.dumps(result))


if __name__ == '__main__':
    main()
