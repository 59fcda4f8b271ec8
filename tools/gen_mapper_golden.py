"""Write tests/golden/mapper_*.npz: whole update + get_state rounds of the reference's own Mapper and OccupancyMap (envs.py).

    python tools/gen_mapper_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and scipy.  envs.py is imported as it is, with empty stand-in modules for what it imports but this path
never touches (pybullet, anki_vector, vector_utils).  scikit-image is replaced by the stand-ins the other generators use:
skimage.draw.line is the published sequential line algorithm (tests/intention_maps_oracle.py: sequential_line),
skimage.morphology.dilation and binary_dilation are scipy.ndimage.grey_dilation(footprint=selem) and binary_dilation(structure=selem),
selem.disk is the x^2 + y^2 <= r^2 footprint.  shortest_paths.GridGraph, a compiled extension, is replaced by the pinned distance oracle
(tests/grid_paths_oracle.py: distance_image).  env.p.getCameraImage returns this file's synthetic depth buffer and body ids, rendered as
tools/gen_observation_maps_golden.py renders them.  Nothing of the reference is copied or kept.

One episode per room (184 x 232 and 232 x 232): an environment of two lifting robots (group 0) and one pushing robot (group 1), whose
Mapper and OccupancyMap objects are built by the reference's own constructors and then go through ROUNDS rounds of update() on every
robot followed by get_state() on every robot under every channel configuration of tests/mapper_oracle.py: configurations() (the
flags of the environment are switched between the calls; get_state reads them when it is called).  One lifting robot is lifting, and in
every round another robot is idle.  Every map after every update and every state is asserted equal, bit for bit, to
tests/mapper_oracle.py before anything is written.  Stored: the frames, the robots' states and each distinct channel image once (the
overhead channel is the same image under every configuration; this is asserted).  Also prints the reference's host time per state.
"""
import argparse
import math
import os
import sys
import time
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import grid_paths_oracle                                            # noqa: E402
import intention_maps_oracle                                        # noqa: E402
import mapper_oracle as oracle                                      # noqa: E402
import observation_maps_oracle                                      # noqa: E402
from gen_observation_maps_golden import CUBE_IDS, OBSTACLE_IDS, RECEPTACLE_ID, ROBOT_BODY_IDS, Scene, render     # noqa: E402

ROUNDS = 3
TYPES = ('lifting_robot', 'lifting_robot', 'pushing_robot')
GROUPS = (0, 0, 1)
MASK_NAMES = ('lifting_robot', 'lifting_robot_with_cube', 'pushing_robot')
MAX_BYTES = 881687                                                  # the largest fixture of the map operators (local_maps_232x232.npz)


class GridGraph:
    """Stand-in for shortest_paths.GridGraph: the distances of the pinned oracle, cached per source as _spfa_with_cache does."""

    def __init__(self, grid):
        self.grid = np.array(grid, copy=True)
        self.cache = {}

    def shortest_path_image(self, source):
        key = (int(source[0]), int(source[1]))
        if key not in self.cache:
            self.cache[key] = grid_paths_oracle.distance_image(self.grid, key)
        return self.cache[key]


def import_reference(ref):
    from scipy import ndimage

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    for name in ('anki_vector', 'pybullet', 'pybullet_utils', 'pybullet_utils.bullet_client', 'skimage', 'vector_utils', 'shortest_paths'):
        stub(name)
    stub('skimage.draw', line=intention_maps_oracle.sequential_line)
    stub('skimage.morphology', binary_dilation=lambda image, selem: ndimage.binary_dilation(image, structure=selem),
         dilation=lambda image, selem: ndimage.grey_dilation(image, footprint=selem))
    stub('skimage.morphology.selem', disk=intention_maps_oracle.disk)
    stub('shortest_paths.shortest_paths', GridGraph=GridGraph)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import envs
    return envs


def episode(room_width, room_length, rng):
    """(receptacle position, obstacle boxes, per round: (cube boxes, per robot: position, heading, lift_state, idle, intention path,
    history path))."""
    lx, ly = room_length / 2, room_width / 2
    u = lambda a: float(rng.uniform(-a, a))
    obstacles = []
    for k in range(4):
        x, y, w, d = u(lx - 0.15), u(ly - 0.1), float(rng.uniform(0.04, 0.1)), float(rng.uniform(0.04, 0.1))
        obstacles.append((x, x + w, y, y + d, (0.05, 0.1, 0.08, 0.1)[k], OBSTACLE_IDS[4 + k % 3]))
    receptacle = (lx - 0.075, ly - 0.075, 0)
    obstacles.append((lx - 0.15, lx, ly - 0.15, ly, 0.002, RECEPTACLE_ID))
    rounds = []
    pose = [((-0.3, 0.1), 0.4), ((0.1, -0.12), 2.5), ((0.32, 0.05), -1.2)]
    history = [[(p[0], p[1], 0)] for p, _ in pose]
    for t in range(ROUNDS):
        cubes = []
        for k in range(6):
            x, y = u(lx - 0.06), u(ly - 0.06)
            cubes.append((x, x + 0.044, y, y + 0.044, 0.044, CUBE_IDS[k]))
        robots = []
        for r in range(3):
            if t > 0:                                               # a step of up to 8 cm and a turn
                (x, y), h = pose[r]
                x = float(np.clip(x + u(0.08), -lx + 0.07, lx - 0.07))
                y = float(np.clip(y + u(0.08), -ly + 0.07, ly - 0.07))
                pose[r] = ((x, y), float((h + u(1.0) + math.pi) % (2 * math.pi) - math.pi))
                history[r].append((x, y, 0))
            (x, y), h = pose[r]
            way = [(x, y, 0)]
            for _ in range(1 + (r + t) % 3):
                way.append((float(np.clip(way[-1][0] + u(0.3), -lx + 0.03, lx - 0.03)), float(np.clip(way[-1][1] + u(0.2), -ly + 0.03, ly - 0.03)), 0))
            robots.append({'position': (x, y), 'heading': h, 'lift_state': ('lifting' if t != 1 else 'ready') if r == 0 else 'ready' if r == 1 else None,
                           'idle': r == (2 - t) % 3, 'intention_path': way, 'history_path': list(history[r]) if len(history[r]) > 1 else [way[0], way[0]]})
        rounds.append((cubes, robots))
    return receptacle, obstacles, rounds


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    envs = import_reference(os.path.abspath(args.reference))
    Mapper = envs.Mapper
    classes = {'lifting_robot': envs.LiftingRobot, 'pushing_robot': envs.PushingRobot}
    configurations = oracle.configurations()
    seconds, states = {'full': 0.0, 'no_search': 0.0}, {'full': 0, 'no_search': 0}

    for fname, room_width, room_length, seed in (('mapper_184x232.npz', 0.5, 1.0, 41), ('mapper_232x232.npz', 1.0, 1.0, 42)):
        rng = np.random.RandomState(seed)
        receptacle_position, obstacles, rounds = episode(room_width, room_length, rng)
        frame = {}

        def get_camera_image(width, height, view, projection):
            frame['view'] = view
            g = observation_maps_oracle.camera_geometry(*view, frame['camera'].NEAR, frame['camera'].FAR, frame['camera'].ASPECT, height)
            assert g.pixel_x.size == width
            frame['depth'], frame['ids'] = render(frame['scene'], g, frame['camera'].NEAR, frame['camera'].FAR)
            return width, height, None, frame['depth'], frame['ids']

        p = types.SimpleNamespace(computeProjectionMatrixFOV=lambda *a: None, computeViewMatrix=lambda pos, target, up: (pos, target, up),
                                  getCameraImage=get_camera_image)
        now = [dict(s) for s in rounds[0][1]]                       # what the stand-in robots answer with: replaced every round

        def make_robot(r):
            robot = object.__new__(classes[TYPES[r]])
            robot.get_position = lambda: (now[r]['position'][0], now[r]['position'][1], 0.0)
            robot.get_heading = lambda: now[r]['heading']
            robot.is_idle = lambda: now[r]['idle']
            robot.controller = types.SimpleNamespace(get_intention_path=lambda: None if now[r]['idle'] else list(now[r]['intention_path']),
                                                     get_history_path=lambda: None if now[r]['idle'] else list(now[r]['history_path']))
            robot.group_index, robot.id, robot.waypoint_positions = GROUPS[r], r, None
            return robot
        robots = [make_robot(r) for r in range(3)]
        env = types.SimpleNamespace(
            p=p, robots=robots, room_width=room_width, room_length=room_length, robot_config=[{'lifting_robot': 2}, {'pushing_robot': 1}],
            use_partial_observations=False, show_occupancy_maps=False, obstacle_ids=OBSTACLE_IDS, cube_ids=CUBE_IDS, receptacle_id=RECEPTACLE_ID,
            receptacle_position=receptacle_position, **oracle.config(use_distance_to_receptacle_map=True))
        mappers = [Mapper(env, robot) for robot in robots]          # the reference's own constructors (envs.py:2014-2051, 2409-2431)
        ref_masks = mappers[0].robot_masks
        masks = np.stack([ref_masks[envs.LiftingRobot], ref_masks['lifting_robot_with_cube'], ref_masks[envs.PushingRobot]])
        mine = [oracle.Maps(room_width, room_length, t) for t in TYPES]
        shape = mine[0].shape
        receptacle_map = oracle.distance_to_receptacle_map(shape, receptacle_position, env.distance_to_receptacle_map_scale)
        for m, o in zip(mappers, mine):
            assert np.array_equal(m.global_distance_to_receptacle_map.view(np.int32), receptacle_map.view(np.int32))
            assert np.array_equal(m.global_occupancy_map.room_mask, o.room_mask)
            assert (m.global_occupancy_map.selem.shape[0] // 2, m.global_occupancy_map.selem_thin.shape[0] // 2) == (o.radius, o.thin_radius)

        rec = {k: [] for k in ('frame_depth', 'frame_ids', 'frame_vectors', 'frame_pixel_x', 'frame_pixel_y', 'frame_depth_constants', 'frame_id_ranges',
                               'state_position', 'state_heading', 'state_lift', 'state_idle', 'state_target', 'way_round', 'way_robot', 'way_kind', 'way_xyz')}
        images = {}
        for t, (cubes, round_states) in enumerate(rounds):
            for r in range(3):
                now[r] = dict(round_states[r])
                robots[r].lift_state = now[r]['lift_state']
                robots[r].target_end_effector_position = None if now[r]['idle'] else now[r]['intention_path'][-1]
            bodies = [(s['position'][0] - 0.03, s['position'][0] + 0.03, s['position'][1] - 0.03, s['position'][1] + 0.03, 0.07, ROBOT_BODY_IDS[k % 2])
                      for k, s in enumerate(now)]
            # ---- update() of every robot
            for r, (m, o) in enumerate(zip(mappers, mine)):
                frame['camera'] = m.camera
                frame['scene'] = Scene(room_length, room_width, obstacles + cubes + [b for k, b in enumerate(bodies) if k != r])
                m.update()
                cam, depth, ids = m.camera, frame['depth'], frame['ids']
                g = observation_maps_oracle.camera_geometry(*frame['view'], cam.NEAR, cam.FAR, cam.ASPECT, cam.image_pixel_height)
                ranges = observation_maps_oracle.IdRanges(min(OBSTACLE_IDS), max(OBSTACLE_IDS), RECEPTACLE_ID, min(CUBE_IDS), max(CUBE_IDS))
                _, ambiguous, _ = observation_maps_oracle.tied_pixels(shape, depth, ids, g, ranges)
                assert not ambiguous.any(), (fname, t, r, int(ambiguous.sum()))      # (a tie among the highest points: the reference's sort decides)
                assert o.update(depth, ids, g, ranges) == 0
                occ = m.global_occupancy_map
                assert np.array_equal(o.overhead.view(np.int32), m.global_overhead_map_without_robots.view(np.int32)), (fname, t, r)
                assert np.array_equal(o.occupancy, occ.occupancy_map) and np.array_equal(o.configuration_space, occ.configuration_space), (fname, t, r)
                assert np.array_equal(o.cspace_thin, occ.cspace_thin) and np.array_equal(o.closest, occ.closest_cspace_indices), (fname, t, r)
                assert o.configuration_space.any()
                for k, v in zip(('frame_depth', 'frame_ids', 'frame_vectors', 'frame_pixel_x', 'frame_pixel_y', 'frame_depth_constants', 'frame_id_ranges'),
                                (depth, ids, np.stack([g.position, g.principal, g.right, g.up]), g.pixel_x, g.pixel_y,
                                 np.asarray([g.far_near, g.far, g.far_minus_near], np.float32),
                                 np.asarray([ranges.min_obstacle, ranges.max_obstacle, ranges.receptacle, 1, ranges.min_cube, ranges.max_cube], np.int32))):
                    rec[k].append(v)
                s = now[r]
                for k, v in zip(('state_position', 'state_heading', 'state_lift', 'state_idle', 'state_target'),
                                (s['position'], s['heading'], s['lift_state'] or '', s['idle'], (0, 0, 0) if s['idle'] else s['intention_path'][-1])):
                    rec[k].append(v)
                for kind, key in enumerate(('intention_path', 'history_path')):
                    for w in s[key]:
                        rec['way_round'].append(t)
                        rec['way_robot'].append(r)
                        rec['way_kind'].append(kind)
                        rec['way_xyz'].append(w)
            # ---- get_state() of every robot under every configuration
            described = [dict(s, type=TYPES[k], group=GROUPS[k], target=None if s['idle'] else s['intention_path'][-1],
                              intention_path=None if s['idle'] else s['intention_path'], history_path=None if s['idle'] else s['history_path'])
                         for k, s in enumerate(now)]
            for name, cfg in configurations.items():
                for k, v in cfg.items():
                    setattr(env, k, v)
                for m in mappers:
                    m.intention_map_selem = envs.disk(cfg['intention_map_line_thickness'] - 1)      # envs.py:2044
                for r, (m, o) in enumerate(zip(mappers, mine)):
                    t0 = time.perf_counter()
                    want = m.get_state()
                    dt = time.perf_counter() - t0
                    bucket = 'full' if name.startswith('full_') else None if cfg['use_shortest_path_map'] or cfg['use_shortest_path_to_receptacle_map'] else 'no_search'
                    if bucket:
                        seconds[bucket] += dt
                        states[bucket] += 1
                    got = oracle.get_state(cfg, o, described, r, masks, list(MASK_NAMES), receptacle_position, receptacle_map)
                    names = oracle.channel_names(cfg, 3)
                    assert want.dtype == got.dtype == np.float32 and want.shape == got.shape == (96, 96, len(names)), (fname, t, name, r)
                    for c, channel in enumerate(names):
                        plane = np.ascontiguousarray(want[:, :, c])
                        assert np.array_equal(got[:, :, c].view(np.int32), plane.view(np.int32)), (fname, t, name, r, channel)
                        stored = images.setdefault(oracle.image_key(cfg, channel), {})
                        if (t, r) in stored:                        # one image per distinct channel: the same under every configuration
                            assert np.array_equal(stored[(t, r)].view(np.int32), plane.view(np.int32)), (fname, t, name, r, channel)
                        stored[(t, r)] = plane
        arrays = {'room': np.asarray([room_width, room_length], np.float64), 'receptacle_position': np.asarray(receptacle_position, np.float64),
                  'robot_type': np.asarray(TYPES), 'robot_group': np.asarray(GROUPS, np.int32), 'masks': masks, 'mask_names': np.asarray(MASK_NAMES),
                  'rounds': np.asarray(ROUNDS, np.int32)}
        dtypes = {'frame_ids': np.int32, 'frame_id_ranges': np.int32, 'way_round': np.int32, 'way_robot': np.int32, 'way_kind': np.int32,
                  'state_idle': np.bool_, 'state_position': np.float64, 'state_heading': np.float64, 'state_target': np.float64, 'way_xyz': np.float64}
        for k, v in rec.items():
            arrays[k] = np.asarray(v) if k == 'state_lift' else np.asarray(v, dtypes.get(k, np.float32))
        arrays['way_xyz'] = arrays['way_xyz'].reshape(-1, 3)
        for key, stored in images.items():
            arrays['image_' + key] = np.stack([stored[(t, r)] for t in range(ROUNDS) for r in range(3)])
        path = os.path.join(args.out, fname)
        np.savez_compressed(path, **arrays)
        print('%s: %d rounds, %d configurations, %d distinct channel images, %d bytes'
              % (path, ROUNDS, len(configurations), sum(len(s) for s in images.values()), os.path.getsize(path)))
        assert os.path.getsize(path) <= MAX_BYTES, 'record fewer rounds'
    print('reference Mapper on the host (one CPU thread, scipy %s standing in for scikit-image): get_state %.2f ms per '
          'state without shortest-path channels (mean over those configurations); %.2f ms per 9- or 11-channel state of the full set, in which the '
          'two searches run through the numpy stand-in for the compiled GridGraph and so say nothing about the reference\'s SPFA'
          % (__import__('scipy').__version__, 1e3 * seconds['no_search'] / states['no_search'],
             1e3 * seconds['full'] / states['full']))


if __name__ == '__main__':
    main()
