"""Rate of simq_occupancy_maps_large and simq_action_waypoints_large on the GPU -- the occupancy maps and the action waypoints of rooms
no LDS holds: one JSON line, also written to profiles/<tag>_large_rooms_rate.json.

    python tools/large_rooms_rate.py [--reps 20] [--tag r11]

Every figure is HIP events around `reps` back-to-back launches after two warm-up launches, every status word checked; the descriptor
upload the C-ABI makes on the launch stream is inside.  There is no pass or fail threshold on these times.
  over_the_cap    both entries at P = 1, 64, 256 on a 290 x 290 map (a 1.6 m room, window 148 x 148) and on a 1 096 x 1 096 map (a 10 m
                  room, window 956 x 956): P robots, each with its own cluttered occupancy map and its own workspace; the action
                  waypoints run on the configuration spaces the occupancy launch left, from random free pixels to random free pixels,
                  no straight-line test, so that every problem is a whole search over the room.
  under_the_cap   the fixture rooms under the caps (tests/golden/occupancy_maps_*.npz: 184 x 232 and 232 x 232), P = 1 and 64, through
                  the LDS entry and through the large one on the same problems: the price of the plane, and of the search state, in
                  global memory.
"""
import argparse
import ctypes
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

WAY_CAPACITY = 64


def timed(launch, status, reps, allowed=(0,)):
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    assert set(status.cpu().tolist()) <= set(allowed), status.cpu().tolist()[:8]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    assert set(status.cpu().tolist()) <= set(allowed), status.cpu().tolist()[:8]
    return e0.elapsed_time(e1) / reps


def cluttered(shape, mask, seed):
    """An occupancy map: the walls just outside the room mask and seeded blocks inside it, about 1 % of the room."""
    rng = np.random.RandomState(seed)
    occ = np.zeros(shape, np.uint8)
    ii, jj = np.nonzero(mask)
    i0, i1, j0, j1 = ii.min(), ii.max() + 1, jj.min(), jj.max() + 1
    occ[i0 - 2:i1 + 2, j0 - 2:j1 + 2] = 1
    occ[i0:i1, j0:j1] = 0
    for _ in range(max(4, (i1 - i0) * (j1 - j0) // 1500)):
        i, j = rng.randint(i0, i1 - 5), rng.randint(j0, j1 - 5)
        occ[i:i + rng.randint(2, 6), j:j + rng.randint(2, 6)] = 1
    return occ


class Maps:
    """P occupancy maps of one shape with one room mask on the device, and the three outputs of the occupancy entries."""

    def __init__(self, occupancy, mask, radius, thin_radius, dev):
        self.P, self.shape, self.radius, self.thin_radius, self.dev = len(occupancy), mask.shape, radius, thin_radius, dev
        self.cells = mask.size
        self.maps = torch.from_numpy(np.concatenate([o.reshape(-1) for o in occupancy] + [mask.reshape(-1)])).to(dev)
        total = self.P * self.cells
        self.cspace = torch.zeros(total, dtype=torch.uint8, device=dev)
        self.thin = torch.zeros(total, dtype=torch.uint8, device=dev)
        self.closest = torch.zeros(2 * total, dtype=torch.int32, device=dev)
        self.status = torch.zeros(self.P, dtype=torch.int32, device=dev)

    def occupancy_launch(self, entry):
        from simq import _lib
        from simq.occupancy import OccupancyLargeProblem, OccupancyProblem
        large = entry == 'simq_occupancy_maps_large'
        need = int(_lib.lib.c.simq_occupancy_maps_large_work_bytes(*self.shape))
        kind = OccupancyLargeProblem if large else OccupancyProblem
        probs = (kind * self.P)(*[kind(p * self.cells, self.P * self.cells, p * self.cells, *([p * need] if large else []), self.shape[0],
                                       self.shape[1], self.radius, self.thin_radius) for p in range(self.P)])
        d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=self.dev)
        work = torch.empty(self.P * need, dtype=torch.uint8, device=self.dev) if large else None
        extra = (_lib.ptr(work), ctypes.c_int64(self.P * need)) if large else ()
        stream = _lib.stream_ptr(self.dev)

        def launch():
            _lib.lib.call(entry, _lib.ptr(self.maps), ctypes.c_int64(self.maps.numel()), probs, self.P, _lib.ptr(d_probs), _lib.ptr(self.cspace),
                          _lib.ptr(self.thin), ctypes.c_int64(self.cspace.numel()), _lib.ptr(self.closest), ctypes.c_int64(self.closest.numel()),
                          _lib.ptr(self.status), *extra, stream)
        launch.keep = (probs, d_probs, work)
        return launch

    def action_launch(self, entry, box, rng):
        """One problem per map on the configuration spaces as they lie: random free source and target pixels, no line test."""
        from simq import _lib
        from simq.actions import ActionWaypointLargeProblem, ActionWaypointProblem
        large = entry == 'simq_action_waypoints_large'
        need = int(_lib.lib.c.simq_action_waypoints_large_work_bytes(box[2], box[3]))
        kind = ActionWaypointLargeProblem if large else ActionWaypointProblem
        cs = self.cspace.view(self.P, *self.shape)
        probs = (kind * self.P)()
        for p in range(self.P):
            free = torch.nonzero(cs[p]).cpu().numpy()
            a, b = rng.randint(len(free), size=2)
            probs[p] = kind(p * self.cells, -1, -1, p * WAY_CAPACITY, *([p * need] if large else []), WAY_CAPACITY, self.shape[0], self.shape[1],
                            int(free[a][0]), int(free[a][1]), int(free[b][0]), int(free[b][1]), *box, -1)
        d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device=self.dev)
        ways = torch.empty((self.P * WAY_CAPACITY, 2), dtype=torch.int32, device=self.dev)
        counts, status = (torch.zeros(self.P, dtype=torch.int32, device=self.dev) for _ in range(2))
        ends = torch.zeros((self.P, 4), dtype=torch.int32, device=self.dev)
        work = torch.empty(self.P * need, dtype=torch.uint8, device=self.dev) if large else None
        extra = (_lib.ptr(work), ctypes.c_int64(self.P * need)) if large else ()
        stream = _lib.stream_ptr(self.dev)

        def launch():
            _lib.lib.call(entry, _lib.ptr(self.cspace), ctypes.c_int64(self.cspace.numel()), None, ctypes.c_int64(0), None, ctypes.c_int64(0),
                          probs, self.P, _lib.ptr(d_probs), _lib.ptr(ways), ctypes.c_int64(self.P * WAY_CAPACITY), _lib.ptr(counts),
                          _lib.ptr(ends), None, 0, _lib.ptr(status), *extra, stream)
        launch.keep = (probs, d_probs, work, ways, counts, ends)
        return launch, status


def free_box(g):
    ii, jj = np.nonzero(g)
    return int(ii.min()), int(jj.min()), int(ii.max() - ii.min() + 1), int(jj.max() - jj.min() + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--tag', default='r11')
    ap.add_argument('--sizes', default='1,64,256')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('large_rooms_rate.py needs a GPU')
    import occupancy_maps_oracle as oracle
    from simq.mapper import padded_room_shape, room_mask
    dev = torch.device('cuda', 0)
    result = {'metric': 'large_rooms', 'unit': 'ms per launch', 'reps': args.reps, 'over_the_cap': [], 'under_the_cap': []}
    for room in (1.6, 10.0):
        shape, mask = padded_room_shape(room, room), room_mask(room, room)
        box = free_box(mask)
        pool = [cluttered(shape, mask, 300 + k) for k in range(4)]
        for P in [int(x) for x in args.sizes.split(',')]:
            maps = Maps([pool[p % 4] for p in range(P)], mask, 6, 3, dev)
            occ_ms = timed(maps.occupancy_launch('simq_occupancy_maps_large'), maps.status, args.reps)
            launch, status = maps.action_launch('simq_action_waypoints_large', box, np.random.RandomState(P))
            act_ms = timed(launch, status, args.reps, allowed=(0, 3))
            result['over_the_cap'].append({'room_m': room, 'map': list(shape), 'window': list(box[2:]), 'P': P,
                                           'occupancy_ms': round(occ_ms, 4), 'occupancy_ms_per_map': round(occ_ms / P, 4),
                                           'action_ms': round(act_ms, 4), 'action_ms_per_search': round(act_ms / P, 4)})
            del maps, launch
            torch.cuda.empty_cache()
    for f in sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'occupancy_maps_*.npz'))):
        fixture = [m for m in oracle.load_fixture(f) if m['configuration_space'].any()]
        mask = fixture[0]['room_mask']
        box = free_box(mask)
        for P in (1, 64):
            maps = Maps([fixture[p % len(fixture)]['occupancy'] for p in range(P)], mask, fixture[0]['radius'], fixture[0]['thin_radius'], dev)
            row = {'map': list(mask.shape), 'window': list(box[2:]), 'P': P}
            for name, entry in (('lds', 'simq_occupancy_maps'), ('hbm', 'simq_occupancy_maps_large')):
                row['occupancy_%s_ms' % name] = round(timed(maps.occupancy_launch(entry), maps.status, args.reps), 4)
            for name, entry in (('lds', 'simq_action_waypoints'), ('hbm', 'simq_action_waypoints_large')):
                launch, status = maps.action_launch(entry, box, np.random.RandomState(P))      # (the same problems for both)
                row['action_%s_ms' % name] = round(timed(launch, status, args.reps, allowed=(0, 3)), 4)
            row['occupancy_ratio'] = round(row['occupancy_hbm_ms'] / row['occupancy_lds_ms'], 2)
            row['action_ratio'] = round(row['action_hbm_ms'] / row['action_lds_ms'], 2)
            result['under_the_cap'].append(row)
    line = json.dumps(result)
    with open(os.path.join(ROOT, 'profiles', '%s_large_rooms_rate.json' % args.tag), 'w') as out:
        out.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
