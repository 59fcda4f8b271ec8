"""Write tests/golden/large_rooms.npz: what the reference's own OccupancyMap.update and Robot.store_new_action leave in rooms whose
maps no LDS holds.

    python tools/gen_large_rooms_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout, scipy and Cython.  The rooms are tests/large_rooms_cases.ROOMS: 0.5 m x 1.3 m (a 184 x 262 map: columns
over SIMQ_OCCUPANCY_MAX_DIM only, the room-mask box under the action cap) and 1.6 m x 1.6 m (290 x 290 with a 148 x 148 box, over both).
envs.py is imported as gen_occupancy_maps_golden.py and gen_store_new_action_golden.py import it, with their stand-ins:
shortest_paths.pyx is compiled into a temporary directory (gen_grid_waypoints_golden.build_reference), `line` is the pinned closed
form of tests/intention_maps_oracle.py, `approximate_polygon` the exact rule of tests/grid_simplify_oracle.py, binary_dilation is
scipy.ndimage's with the disk footprint.  Nothing compiled is kept, nothing of the reference is copied.

Per room: the reference's padded shape and room mask, and per robot class two occupancy maps -- synthetic point clouds through a real
OccupancyMap.update (the scenarios of gen_occupancy_maps_golden.py) -- with the reference's three results.  Then Robot.store_new_action
on stand-in robots over those maps, drawn as gen_store_new_action_golden.py draws them until every class of
store_new_action_oracle.CLASSES has PER_CLASS cases (large_rooms_cases.PER_CLASS_LARGEST in the 1.6 m room: a fixture of straight lines
would let the search go untested).  tests/occupancy_maps_oracle.py and tests/store_new_action_oracle.py must equal every result,
and no configuration space may be empty, before anything is written.
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
import large_rooms_cases as lr                                          # noqa: E402
import occupancy_maps_oracle as occ_oracle                              # noqa: E402
import store_new_action_oracle as oracle                                # noqa: E402
from gen_grid_waypoints_golden import build_reference                   # noqa: E402
from gen_occupancy_maps_golden import OBSTACLE_SEG, ROBOT_CLASSES, cloud, scenarios   # noqa: E402

PER_CLASS = (2, lr.PER_CLASS_LARGEST)                   # per room
PER_PLAIN, MAX_DRAWS = 1, 400000
SCENARIOS = (('clutter_3', 'touching_wall'), ('clutter_4', 'outside_room'), ('clutter_5', 'border_corner'), ('clutter_2', 'walls_only'))


def import_envs(ref, GridGraph):
    from scipy import ndimage

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def absent(*args, **kwargs):
        raise NotImplementedError('not part of the occupancy-map or store_new_action path')

    for name in ('anki_vector', 'pybullet', 'pybullet_utils', 'pybullet_utils.bullet_client', 'vector_utils'):
        stub(name)
    stub('skimage.morphology', binary_dilation=lambda image, selem: ndimage.binary_dilation(image, structure=selem), dilation=absent)
    stub('skimage.morphology.selem', disk=occ_oracle.disk)
    stub('shortest_paths.shortest_paths', GridGraph=GridGraph)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import envs
    return envs


def occupancy_maps(envs, room, rec):
    """Two updated OccupancyMap objects per robot class; their inputs and results go to `rec`."""
    room_width, room_length = room
    rng = np.random.RandomState(11)
    objects = []
    for k, cls in enumerate(ROBOT_CLASSES):
        for name in SCENARIOS[k]:
            m = envs.OccupancyMap(types.SimpleNamespace(RADIUS=getattr(envs, cls).RADIUS, id=k), room_length, room_width)
            radius, thin_radius = m.selem.shape[0] // 2, m.selem_thin.shape[0] // 2
            assert np.array_equal(m.selem, occ_oracle.disk(radius)) and np.array_equal(m.selem_thin, occ_oracle.disk(thin_radius))
            pixels = scenarios(m.room_mask, radius, rng)[name][0]
            points, seg = cloud(m.occupancy_map.shape, pixels, rng)
            m.update(points, seg, OBSTACLE_SEG)
            want = np.zeros(m.occupancy_map.shape, np.uint8)
            want[tuple(np.asarray(sorted(set(pixels))).T)] = 1
            assert np.array_equal(m.occupancy_map, want), (room, name)                        # the cloud landed where it was aimed
            assert m.configuration_space.dtype == m.cspace_thin.dtype == np.uint8 and m.closest_cspace_indices.dtype == np.int32
            assert m.configuration_space.any(), (room, name)                                   # (an empty one has no defined result)
            cs, thin, near = occ_oracle.update(m.occupancy_map, m.room_mask, radius, thin_radius)
            assert np.array_equal(cs, m.configuration_space) and np.array_equal(thin, m.cspace_thin), (room, name)
            assert near.dtype == m.closest_cspace_indices.dtype and np.array_equal(near, m.closest_cspace_indices), (room, name)
            for key, v in (('names', '%s_%s' % (name, cls)), ('robot_type', k), ('occupancy', m.occupancy_map.copy()), ('radius', radius),
                           ('thin_radius', thin_radius), ('configuration_space', m.configuration_space.copy()),
                           ('cspace_thin', m.cspace_thin.copy()), ('closest', m.closest_cspace_indices.copy())):
                rec.setdefault(key, []).append(v)
            objects.append((k, m))
    rec['shape'], rec['room_mask'] = np.asarray(objects[0][1].occupancy_map.shape, np.int32), objects[0][1].room_mask.copy()
    return objects


def action_cases(envs, measure, classes, room_index, objects, rows):
    """Robot.store_new_action on stand-in robots over the updated OccupancyMap objects of one room."""

    class Controller:
        def reset(self):
            pass

        def new_action(self):
            pass

    shape = objects[0][1].occupancy_map.shape
    free = [np.argwhere(m.configuration_space != 0) for _, m in objects]
    caches = [{} for _ in objects]
    rng = np.random.RandomState(31 + shape[1])
    have, plain, per_class = dict.fromkeys(oracle.CLASSES, 0), 0, PER_CLASS[room_index]
    for k in range(MAX_DRAWS):
        if min(have.values()) >= per_class and plain >= PER_PLAIN:
            break
        n = k % len(objects)
        type_index, occupancy = objects[n]
        robot_type, use_sp = oracle.ROBOT_TYPES[type_index], k % 9 != 8
        i, j = free[n][rng.randint(len(free[n]))]
        x, y = wo.pixel_indices_to_position(i + float(rng.uniform(-0.45, 0.45)), j + float(rng.uniform(-0.45, 0.45)), shape)
        position, heading = (float(x), float(y), 0), float(rng.uniform(-np.pi, np.pi))
        a = int(rng.randint(oracle.NUM_OUTPUT_CHANNELS[robot_type] * oracle.WIDTH * oracle.WIDTH))
        returned = []                                               # the reference's waypoints before store_new_action edits them
        robot = types.SimpleNamespace(
            NUM_OUTPUT_CHANNELS=classes[robot_type].NUM_OUTPUT_CHANNELS, END_EFFECTOR_LOCATION=classes[robot_type].END_EFFECTOR_LOCATION,
            get_position=lambda position=position: position, get_heading=lambda heading=heading: heading,
            env=types.SimpleNamespace(use_shortest_path_movement=use_sp),
            mapper=types.SimpleNamespace(shortest_path=lambda p, q, o=occupancy: returned.append(o.shortest_path(p, q)) or list(returned[-1])),
            controller=Controller())
        del measure.RECORD[:]
        envs.Robot.store_new_action(robot, a)
        traced = len(measure.RECORD) > 0 and len(robot.waypoint_positions) > 2
        signed_dist = oracle.store_new_action(a, position, heading, robot_type, (lambda p, q: list(returned[-1])) if use_sp else None)[4]
        if use_sp:
            mine = oracle.kinds(len(robot.waypoint_positions), signed_dist, traced)
            if all(have[c] >= per_class for c in mine):
                continue
            for c in mine:
                have[c] += 1
        else:
            if plain >= PER_PLAIN:
                continue
            plain += 1
        path = (lambda p, q, o=occupancy, cache=caches[n]: wo.occupancy_shortest_path(
            o.configuration_space, o.cspace_thin, o.closest_cspace_indices, p, q, so.exact, cache)) if use_sp else None
        want = oracle.store_new_action(a, position, heading, robot_type, path)
        got = (robot.action, robot.target_end_effector_position, robot.waypoint_positions, robot.waypoint_headings)
        assert oracle.same_bits(list(got), list(want[:4])), (room_index, n, a, position, heading, got, want)
        rows.append((room_index, n, type_index, use_sp, a, position, heading) + got)
    print('room %s: %d draws, classes %s, %d without shortest paths' % (lr.ROOMS[room_index], k, have, plain))
    assert min(have.values()) >= per_class and plain >= PER_PLAIN, (room_index, have, plain)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix='large_rooms_ref_')
    try:
        GridGraph, measure = build_reference(os.path.abspath(args.reference), tmp)
        measure.SIMPLIFY[0] = so.exact
        envs = import_envs(os.path.abspath(args.reference), GridGraph)
        classes = {t: envs.Robot.get_robot_cls(t) for t in oracle.ROBOT_TYPES}
        assert tuple(oracle.ROBOT_TYPES) == lr.ROBOT_TYPES and [c.__name__ for c in classes.values()] == list(ROBOT_CLASSES)
        for t, cls in classes.items():
            assert cls.END_EFFECTOR_LOCATION == oracle.END_EFFECTOR_LOCATION[t] and cls.NUM_OUTPUT_CHANNELS == oracle.NUM_OUTPUT_CHANNELS[t], t
        arrays, rows = {}, []
        for r, room in enumerate(lr.ROOMS):
            rec = {}
            objects = occupancy_maps(envs, room, rec)
            assert tuple(rec['shape']) == lr.SHAPES[r], rec['shape']
            for key, v in rec.items():
                arrays['room%d_%s' % (r, key)] = v if key in ('shape', 'room_mask') else np.asarray(v) if key == 'names' else \
                    np.stack(v).astype(np.int32 if key in ('radius', 'thin_radius', 'closest', 'robot_type') else np.uint8)
            action_cases(envs, measure, classes, r, objects, rows)
        counts = [len(row[9]) for row in rows]
        arrays.update(
            room=np.asarray([row[0] for row in rows], np.int32), map=np.asarray([row[1] for row in rows], np.int32),
            robot_type=np.asarray([row[2] for row in rows], np.int32), use_shortest_path_movement=np.asarray([row[3] for row in rows], bool),
            a=np.asarray([row[4] for row in rows], np.int64), position=np.asarray([row[5][:2] for row in rows], np.float64),
            heading=np.asarray([row[6] for row in rows], np.float64), action=np.asarray([row[7] for row in rows], np.int64),
            target=np.asarray([row[8][:2] for row in rows], np.float64),
            waypoint_positions=np.asarray([w[:2] for row in rows for w in row[9]], np.float64),
            offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            waypoint_headings=np.asarray([h for row in rows for h in row[10]], np.float64))
        for row in rows:                                                # what the arrays leave out is what the reference always writes
            assert row[8][2] == 0 and isinstance(row[8][2], int) and all(w[2] == 0 for w in row[9]) and row[9][0] is row[5]
        path = os.path.join(args.out, 'large_rooms.npz')
        np.savez_compressed(path, **arrays)
        print('%s: %d maps, %d cases, %d bytes' % (path, sum(len(arrays['room%d_names' % r]) for r in range(len(lr.ROOMS))), len(rows),
                                                    os.path.getsize(path)))
        assert os.path.getsize(path) < 1 << 20 and len(rows) >= 20
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
