"""Write tests/golden/store_new_action.npz: what the reference's own Robot.store_new_action leaves in a robot.

    python tools/gen_store_new_action_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and Cython.  The function object envs.Robot.store_new_action is called on stand-in robot / env / mapper
objects: the stand-in mapper's shortest_path is the reference's OccupancyMap.shortest_path on the maps of
tests/golden/occupancy_maps_*.npz with the reference's GridGraph, compiled into a temporary directory as gen_grid_waypoints_golden.py
does; `line` is served by the pinned closed form of tests/intention_maps_oracle.py, `approximate_polygon` by the exact rule of
tests/grid_simplify_oracle.py (what simplify='exact' means).  Nothing compiled is kept, nothing of the reference is copied.

Cases: both rooms, the four robot types in turn, both use_shortest_path_movement settings, seeded poses on free cells with
sub-pixel offsets, headings over (-pi, pi), actions over every channel; drawn until every class of
tests/store_new_action_oracle.CLASSES has at least PER_CLASS cases in each room (a draw is kept while one of its classes is short).
Per case the file holds the inputs and the four attributes as arrays.  The scalar oracle must equal all of it before anything is
written.
"""
import argparse
import os
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import grid_simplify_oracle as so                                       # noqa: E402
import grid_waypoints_oracle as wo                                      # noqa: E402
import store_new_action_oracle as oracle                                # noqa: E402
from gen_grid_waypoints_golden import build_reference                   # noqa: E402

PER_CLASS, PER_PLAIN, MAX_DRAWS = 8, 8, 200000


def import_envs(ref, GridGraph):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    for name in ('anki_vector', 'pybullet', 'pybullet_utils', 'pybullet_utils.bullet_client', 'vector_utils'):
        stub(name)
    unused = lambda *a, **k: None                                       # noqa: E731  (store_new_action reaches none of them)
    stub('skimage.morphology', binary_dilation=unused, dilation=unused)
    stub('skimage.morphology.selem', disk=unused)
    stub('shortest_paths.shortest_paths', GridGraph=GridGraph)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import envs
    return envs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix='store_new_action_ref_')
    try:
        GridGraph, measure = build_reference(os.path.abspath(args.reference), tmp)
        measure.SIMPLIFY[0] = so.exact
        envs = import_envs(os.path.abspath(args.reference), GridGraph)
        classes = {t: envs.Robot.get_robot_cls(t) for t in oracle.ROBOT_TYPES}
        for t, cls in classes.items():
            assert cls.END_EFFECTOR_LOCATION == oracle.END_EFFECTOR_LOCATION[t] and cls.NUM_OUTPUT_CHANNELS == oracle.NUM_OUTPUT_CHANNELS[t], t
        assert envs.VectorEnv.CUBE_WIDTH == oracle.CUBE_WIDTH and envs.Mapper.LOCAL_MAP_PIXEL_WIDTH == oracle.WIDTH

        class Occupancy:                                                # what OccupancyMap.shortest_path reads of its object
            shortest_path = envs.OccupancyMap.shortest_path
            _closest_valid_cspace_indices = envs.OccupancyMap._closest_valid_cspace_indices

        class Controller:
            def reset(self):
                pass

            def new_action(self):
                pass

        rows = []
        for room_index, room in enumerate(oracle.ROOMS):
            cspace, thin, closest = oracle.maps(args.out, room)
            usable = [m for m in range(len(cspace)) if cspace[m].any()]
            occupancy = {}
            for m in usable:
                o = occupancy[m] = Occupancy()
                o.configuration_space, o.cspace_thin, o.closest_cspace_indices = cspace[m], thin[m], closest[m]
                o.grid_graph = GridGraph(np.ascontiguousarray(cspace[m]))
            free = {m: np.argwhere(cspace[m] != 0) for m in usable}
            shape = cspace.shape[1:]
            rng = np.random.RandomState(31 + shape[1])
            have = dict.fromkeys(oracle.CLASSES, 0)
            plain = 0
            for k in range(MAX_DRAWS):
                if min(have.values()) >= PER_CLASS and plain >= PER_PLAIN:
                    break
                m, robot_type, use_sp = usable[k % len(usable)], oracle.ROBOT_TYPES[k % 4], k % 5 != 4
                i, j = free[m][rng.randint(len(free[m]))]
                x, y = wo.pixel_indices_to_position(i + float(rng.uniform(-0.45, 0.45)), j + float(rng.uniform(-0.45, 0.45)), shape)
                position, heading = (float(x), float(y), 0), float(rng.uniform(-np.pi, np.pi))
                a = int(rng.randint(oracle.NUM_OUTPUT_CHANNELS[robot_type] * oracle.WIDTH * oracle.WIDTH))
                robot = types.SimpleNamespace(
                    NUM_OUTPUT_CHANNELS=classes[robot_type].NUM_OUTPUT_CHANNELS, END_EFFECTOR_LOCATION=classes[robot_type].END_EFFECTOR_LOCATION,
                    get_position=lambda position=position: position, get_heading=lambda heading=heading: heading,
                    env=types.SimpleNamespace(use_shortest_path_movement=use_sp),
                    mapper=types.SimpleNamespace(shortest_path=lambda p, q, o=occupancy[m]: returned.append(o.shortest_path(p, q)) or list(returned[-1])),
                    controller=Controller())
                returned = []                                           # the reference's waypoints before store_new_action edits them
                del measure.RECORD[:]
                envs.Robot.store_new_action(robot, a)
                traced = len(measure.RECORD) > 0 and len(robot.waypoint_positions) > 2
                signed_dist = oracle.store_new_action(a, position, heading, robot_type, (lambda p, q: list(returned[-1])) if use_sp else None)[4]
                if use_sp:
                    mine = oracle.kinds(len(robot.waypoint_positions), signed_dist, traced)
                    if all(have[c] >= PER_CLASS for c in mine):
                        continue
                    for c in mine:
                        have[c] += 1
                else:
                    if plain >= PER_PLAIN:
                        continue
                    plain += 1
                want = oracle.store_new_action(a, position, heading, robot_type, oracle.shortest_path_on(args.out, room, m) if use_sp else None)
                got = (robot.action, robot.target_end_effector_position, robot.waypoint_positions, robot.waypoint_headings)
                assert oracle.same_bits(list(got), list(want[:4])), (room, m, a, position, heading, got, want)
                rows.append((room_index, m, k % 4, use_sp, a, position, heading) + got)
            print('%s: %d draws, classes %s, %d without shortest paths' % (room, k, have, plain))
            assert min(have.values()) >= PER_CLASS and plain >= PER_PLAIN, (room, have, plain)
        counts = [len(r[9]) for r in rows]
        arrays = dict(
            room=np.asarray([r[0] for r in rows], np.int32), map=np.asarray([r[1] for r in rows], np.int32),
            robot_type=np.asarray([r[2] for r in rows], np.int32), use_shortest_path_movement=np.asarray([r[3] for r in rows], bool),
            a=np.asarray([r[4] for r in rows], np.int64), position=np.asarray([r[5][:2] for r in rows], np.float64),
            heading=np.asarray([r[6] for r in rows], np.float64), action=np.asarray([r[7] for r in rows], np.int64),
            target=np.asarray([r[8][:2] for r in rows], np.float64),
            waypoint_positions=np.asarray([w[:2] for r in rows for w in r[9]], np.float64),
            offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            waypoint_headings=np.asarray([h for r in rows for h in r[10]], np.float64))
        for r in rows:                                                  # what the arrays leave out is what the reference always writes
            assert r[8][2] == 0 and isinstance(r[8][2], int) and all(w[2] == 0 for w in r[9]) and r[9][0] is r[5]
        path = os.path.join(args.out, 'store_new_action.npz')
        np.savez_compressed(path, **arrays)
        print('%s: %d cases, %d bytes' % (path, len(rows), os.path.getsize(path)))
        assert os.path.getsize(path) < 150000
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
