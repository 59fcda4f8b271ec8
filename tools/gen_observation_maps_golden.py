"""Write tests/golden/observation_maps_*.npz: overhead and occupancy maps updated by the reference's own Mapper and OccupancyMap.

    python tools/gen_observation_maps_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and scipy.  envs.py is imported as it is, with the stand-in modules tools/gen_occupancy_maps_golden.py
uses (pybullet, anki_vector, vector_utils, skimage, shortest_paths) and a stand-in `env.p` whose getCameraImage returns this file's
synthetic depth buffer (float32) and body ids (int32): a ray per pixel against a scene of boxes on a floor, rendered here.  The maps
come from the reference's own OverheadCamera.capture_image / ForwardFacingCamera.capture_image, Mapper.update and OccupancyMap.update,
on Mapper objects whose attributes this file sets and real OccupancyMap objects; channel 0 of Mapper.get_state (envs.py:2071-2073) is
stored beside them.  Nothing of the reference is copied or kept.  Before anything is written every result is asserted equal to
tests/observation_maps_oracle.py under the tie condition: a pixel is ambiguous when its highest points carry more than one seg value;
everywhere else the overhead maps agree bit for bit, on an ambiguous pixel the reference holds one of the tied values; ambiguous pixels
occur only in cases named tie_* and are at most 1 % of a file's written pixels; the occupancy maps agree everywhere.  Also prints the
reference's host time per update (one CPU thread): Mapper.update once more on a frame that is handed over ready, that is the capture
arithmetic, the sort and both scatters, without this file's rendering and without the configuration space.
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

import observation_maps_oracle as oracle                            # noqa: E402
from occupancy_maps_oracle import disk                              # noqa: E402

OBSTACLE_IDS, RECEPTACLE_ID, CUBE_IDS = list(range(3, 10)), 10, list(range(11, 21))
ROBOT_BODY_IDS = (1, 2)                                             # bodies of no class: seg 0


def import_reference(ref):
    from scipy import ndimage

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def absent(*args, **kwargs):
        raise NotImplementedError('not part of the observation path')

    for name in ('anki_vector', 'pybullet', 'pybullet_utils', 'pybullet_utils.bullet_client', 'skimage', 'vector_utils', 'shortest_paths'):
        stub(name)
    stub('skimage.draw', line=absent)
    stub('skimage.morphology', binary_dilation=lambda image, selem: ndimage.binary_dilation(image, structure=selem), dilation=absent)
    stub('skimage.morphology.selem', disk=disk)
    stub('shortest_paths.shortest_paths', GridGraph=lambda grid: None)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import envs
    return envs


class Scene:
    """Axis-aligned boxes (x0, x1, y0, y1, height, body id) on a floor (id 0); later boxes cover earlier ones."""

    def __init__(self, room_length, room_width, boxes):
        lx, ly = room_length / 2, room_width / 2
        t = 0.06
        walls = [(-lx - t, lx + t, ly, ly + t, 0.1, 3), (-lx - t, lx + t, -ly - t, -ly, 0.1, 4), (-lx - t, -lx, -ly, ly, 0.1, 5),
                 (lx, lx + t, -ly, ly, 0.1, 6)]
        self.boxes = walls + list(boxes)

    def lookup(self, x, y):
        h = np.zeros(x.shape)
        ident = np.zeros(x.shape, np.int32)
        for x0, x1, y0, y1, height, body in self.boxes:
            inside = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
            h[inside] = height
            ident[inside] = body
        return h, ident


def render(scene, g, near, far):
    """The depth buffer (float32) and body ids (int32, -1 where nothing is hit before the far plane) of a camera with geometry `g`: the
    ray of every pixel meets the floor, takes the height and id of what stands there and ends on that height."""
    px, py = g.pixel_x.astype(np.float64)[None, :], g.pixel_y.astype(np.float64)[:, None]
    d = [float(g.principal[c]) + px * float(g.right[c]) + py * float(g.up[c]) for c in range(3)]
    cam = [float(v) for v in g.position]
    down = d[2] < -1e-6
    t = np.where(down, cam[2] / np.where(down, -d[2], 1.0), np.inf)
    finite = np.isfinite(t) & (t < 1e3)
    x = np.where(finite, cam[0] + np.where(finite, t, 0.0) * d[0], 1e6)
    y = np.where(finite, cam[1] + np.where(finite, t, 0.0) * d[1], 1e6)
    h, ident = scene.lookup(x, y)
    t = np.where(finite, (cam[2] - h) / np.where(down, -d[2], 1.0), np.inf)
    hit = finite & (t <= far)
    t = np.clip(np.where(hit, t, far), near, far)
    buffer = np.clip((far - far * near / t) / (far - near), 0.0, 1.0).astype(np.float32)
    return buffer, np.where(hit, ident, -1).astype(np.int32)


def cases(room_length, room_width, rng):
    """(name, camera, steps) with steps a list of (position, heading, boxes, with_receptacle, store_state)."""
    lx, ly = room_length / 2, room_width / 2
    u = lambda a: float(rng.uniform(-a, a))

    def clutter(n_boxes, n_cubes, receptacle_height=None):
        out = []
        for k in range(n_boxes):
            x, y, w, d = u(lx - 0.1), u(ly - 0.08), float(rng.uniform(0.03, 0.12)), float(rng.uniform(0.03, 0.12))
            out.append((x, x + w, y, y + d, (0.05, 0.15, 0.2, 0.08)[k % 4], OBSTACLE_IDS[4 + k % 3]))
        for k in range(n_cubes):
            x, y = u(lx - 0.06), u(ly - 0.06)
            out.append((x, x + 0.044, y, y + 0.044, 0.044, CUBE_IDS[k % len(CUBE_IDS)]))
        if receptacle_height is not None:
            out.append((lx - 0.15, lx, ly - 0.15, ly, receptacle_height, RECEPTACLE_ID))
        return out

    robots = [(0.1, 0.17, -0.05, 0.02, 0.07, ROBOT_BODY_IDS[0]), (-0.2, -0.13, 0.05, 0.12, 0.07, ROBOT_BODY_IDS[1])]
    out = [
        ('flat_floor', 'overhead', [((0.0, 0.0), 0.0, [], True, True)]),
        ('boxes_cubes', 'overhead', [((0.12, -0.03), 0.7, clutter(6, 8, 0.002), True, True)]),
        ('obstacle_edge', 'overhead', [((-0.2, 0.05), 2.3, [(-0.2513, -0.1487, 0.0131, 0.1077, 0.12, 7), (-0.3, -0.26, -0.02, 0.02, 0.03, 8)], True, True)]),
        ('near_wall_corner', 'overhead', [((-lx - 0.45, ly + 0.5), -2.5, clutter(2, 2, 0.002), True, False)]),
        ('near_wall_edge', 'overhead', [((lx + 0.5, 0.02), -0.6, clutter(2, 2, 0.002), True, False)]),
        ('unknown_ids', 'overhead', [((0.05, 0.0), -0.6, clutter(3, 3, 0.002) + robots, True, True)]),
        ('no_receptacle', 'overhead', [((lx - 0.2, ly - 0.2), 1.1, clutter(3, 4, 0.002), False, True)]),
        ('successive', 'overhead', [((-0.25, -0.05), 0.2, clutter(4, 4, 0.002), True, True), ((0.2, 0.1), 1.9, clutter(4, 4, 0.002), True, True),
                                    ((0.0, -ly + 0.1), -2.2, clutter(4, 6, 0.002), True, True)]),
        ('tie_receptacle_a', 'overhead', [((lx - 0.2, ly - 0.2), 0.0, clutter(2, 2, 0.0), True, True)]),
        ('tie_receptacle_b', 'overhead', [((lx - 0.25, ly - 0.15), math.pi / 2, clutter(2, 2, 0.0), True, True)]),
        ('forward_far', 'forward', [((-lx + 0.15, 0.0), 0.1, clutter(3, 4, 0.002), True, True)]),
        ('forward_wall', 'forward', [((lx - 0.12, ly - 0.15), 0.9, clutter(2, 3, 0.002), True, True)]),
        ('forward_successive', 'forward', [((0.0, 0.0), 2.6, clutter(3, 3, 0.002), True, True), ((0.1, -0.1), -1.8, clutter(3, 3, 0.002), True, True)]),
    ]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    envs = import_reference(os.path.abspath(args.reference))
    Mapper = envs.Mapper
    mask = Mapper._create_robot_mask(envs.PushingRobot)
    seconds = {'overhead': 0.0, 'forward': 0.0, 'remainder': 0.0}
    updates = {'overhead': 0, 'forward': 0}

    for fname, room_width, room_length, seed in (('observation_maps_184x232.npz', 0.5, 1.0, 31), ('observation_maps_232x232.npz', 1.0, 1.0, 32)):
        rng = np.random.RandomState(seed)
        frame = {}

        def get_camera_image(width, height, view, projection):
            if frame.get('replay'):                                 # the timed repeat: the frame just rendered, no rendering
                assert view == frame['view']
                return width, height, None, frame['depth'], frame['ids']
            frame['view'] = view
            g = oracle.camera_geometry(*view, frame['camera'].NEAR, frame['camera'].FAR, frame['camera'].ASPECT, height)
            assert g.pixel_x.size == width
            frame['depth'], frame['ids'] = render(frame['scene'], g, frame['camera'].NEAR, frame['camera'].FAR)
            return width, height, None, frame['depth'], frame['ids']

        p = types.SimpleNamespace(computeProjectionMatrixFOV=lambda *a: None, computeViewMatrix=lambda pos, target, up: (pos, target, up),
                                  getCameraImage=get_camera_image)
        arrays = {}
        names, n_written, n_ambiguous = [], 0, 0
        for name, camera_kind, steps in cases(room_length, room_width, rng):
            pose = {}
            robot = object.__new__(envs.PushingRobot)
            robot.get_position = lambda: (pose['position'][0], pose['position'][1], 0.0)
            robot.get_heading = lambda: pose['heading']
            robot.group_index, robot.id = 0, 0
            env = types.SimpleNamespace(p=p, obstacle_ids=OBSTACLE_IDS, cube_ids=CUBE_IDS, receptacle_id=RECEPTACLE_ID, robots=[robot],
                                        room_width=room_width, room_length=room_length)
            m = object.__new__(Mapper)
            m.env, m.robot, m.robot_masks = env, robot, {envs.PushingRobot: mask}
            m.global_overhead_map_without_robots = Mapper.create_padded_room_zeros(room_width, room_length)
            m.global_occupancy_map = envs.OccupancyMap(robot, room_length, room_width)
            for step, (position, heading, boxes, with_receptacle, store_state) in enumerate(steps):
                env.receptacle_id = RECEPTACLE_ID if with_receptacle else None
                m.camera = (envs.OverheadCamera if camera_kind == 'overhead' else envs.ForwardFacingCamera)(env)   # (ids are read on first use)
                pose['position'], pose['heading'] = position, heading
                frame['camera'], frame['scene'] = m.camera, Scene(room_length, room_width, boxes)
                before = (m.global_overhead_map_without_robots.copy(), m.global_occupancy_map.occupancy_map.copy())
                m.update()
                # timed: the same update again (the same frame gives the same maps), with the stand-in simulator handing back the
                # frame it has just rendered, so that none of this file's ray casting is counted, and with the configuration space of
                # OccupancyMap.update (two dilations, the distance transform, the grid graph) replaced by no-ops,
                # so that OccupancyMap.update costs its own scatter plus three array expressions on the map
                occ = m.global_occupancy_map
                kept = (occ.configuration_space, occ.closest_cspace_indices, occ.cspace_thin, occ.grid_graph)
                real = (envs.binary_dilation, envs.distance_transform_edt)
                nothing = np.zeros(occ.occupancy_map.shape, bool)
                envs.binary_dilation, envs.distance_transform_edt = (lambda image, selem: nothing), (lambda *a, **k: None)
                frame['replay'] = True
                t0 = time.perf_counter()
                m.update()
                seconds[camera_kind] += time.perf_counter() - t0
                updates[camera_kind] += 1
                frame['replay'] = False
                envs.binary_dilation, envs.distance_transform_edt = real
                occ.configuration_space, occ.closest_cspace_indices, occ.cspace_thin, occ.grid_graph = kept
                t0 = time.perf_counter()                            # what the no-ops leave of the configuration space
                for _ in range(10):
                    1 - np.maximum(1 - occ.room_mask, nothing.astype(np.uint8)), 1 - nothing.astype(np.uint8), np.minimum(occ.room_mask, occ.occupancy_map)
                seconds['remainder'] += (time.perf_counter() - t0) / 10
                points, seg = m.camera.capture_image(robot.get_position(), robot.get_heading())
                assert points.dtype == np.float32 and seg.dtype == np.float32
                after = (m.global_overhead_map_without_robots, m.global_occupancy_map.occupancy_map)
                assert after[0].dtype == np.float32 and after[1].dtype == np.uint8

                # the oracle on the same frame, under the tie condition
                cam = m.camera
                g = oracle.camera_geometry(*frame['view'], cam.NEAR, cam.FAR, cam.ASPECT, cam.image_pixel_height)
                r = oracle.IdRanges(min(OBSTACLE_IDS), max(OBSTACLE_IDS), env.receptacle_id, min(CUBE_IDS), max(CUBE_IDS))
                depth, ids = frame['depth'], frame['ids']
                assert np.array_equal(oracle.points_of(depth, g).view(np.int32), points.view(np.int32)), (fname, name, step)
                assert np.array_equal(oracle.segmentation(ids, r).view(np.int32), seg.view(np.int32)), (fname, name, step)
                got = (before[0].copy(), before[1].copy())
                assert oracle.update(got[0], got[1], depth, ids, g, r) == 0
                written, ambiguous, tied = oracle.tied_pixels(got[0].shape, depth, ids, g, r)
                assert np.array_equal(got[0][~ambiguous].view(np.int32), after[0][~ambiguous].view(np.int32)), (fname, name, step)
                assert np.array_equal(got[0][~written].view(np.int32), before[0][~written].view(np.int32))
                for (i, j), values in tied.items():
                    assert float(after[0][i, j]) in values and float(got[0][i, j]) in values, (fname, name, step, i, j)
                assert np.array_equal(got[1], after[1]), (fname, name, step)
                assert name.startswith('tie_') or not ambiguous.any(), (fname, name, step, int(ambiguous.sum()))
                assert not name.startswith('tie_') or ambiguous.any(), (fname, name)
                n_written += int(written.sum())
                n_ambiguous += int(ambiguous.sum())
                if name.startswith('near_wall'):
                    i, j = oracle.pixel_indices(points[:, :, 0], points[:, :, 1], got[0].shape)
                    assert ((i == 0) | (i == got[0].shape[0] - 1) | (j == 0) | (j == got[0].shape[1] - 1)).any(), (fname, name)
                if name == 'forward_far':
                    assert (depth == 1.0).any() and (ids == -1).any()

                key = '%s%s' % (name, '_step%d' % step if len(steps) > 1 else '')
                names.append(key)
                rec = {'depth': depth, 'ids': ids, 'overhead_before': before[0], 'occupancy_before': before[1],
                       'overhead_after': after[0].copy(), 'occupancy_after': after[1].copy(),
                       'camera': np.asarray([list(v) for v in frame['view']], np.float64),
                       'camera_constants': np.asarray([cam.NEAR, cam.FAR, cam.ASPECT, cam.image_pixel_height, envs.Camera.FOV], np.float64),
                       'vectors': np.stack([g.position, g.principal, g.right, g.up]), 'pixel_x': g.pixel_x, 'pixel_y': g.pixel_y,
                       'depth_constants': np.asarray([g.far_near, g.far, g.far_minus_near], np.float32),
                       'id_ranges': np.asarray([r.min_obstacle, r.max_obstacle, -1 if r.receptacle is None else r.receptacle,
                                                0 if r.receptacle is None else 1, r.min_cube, r.max_cube], np.int32),
                       'pose': np.asarray([position[0], position[1], heading], np.float64)}
                if store_state:
                    rec['state0'] = np.asarray(m._get_local_map(m._create_global_overhead_map()), np.float32).copy()
                for k, v in rec.items():
                    arrays['%s/%s' % (key, k)] = v
        occ = m.global_occupancy_map
        arrays.update({'names': np.asarray(names), 'room_mask': occ.room_mask, 'robot_mask': mask,
                       'radius': np.asarray([occ.selem.shape[0] // 2, occ.selem_thin.shape[0] // 2], np.int32),
                       'robot_seg_value': np.asarray(envs.Camera.SEG_VALUES['robot_group_1'], np.float32)})
        assert n_ambiguous > 0 and n_ambiguous <= 0.01 * n_written, (n_ambiguous, n_written)
        path = os.path.join(args.out, fname)
        np.savez_compressed(path, **arrays)
        print('%s: %d frames, %d written pixels, %d ambiguous, %d bytes' % (path, len(names), n_written, n_ambiguous, os.path.getsize(path)))
        assert os.path.getsize(path) < 881687
    for kind in ('overhead', 'forward'):
        print('reference Mapper.update on the host, %s camera: %.2f ms per update (capture arithmetic, sort, overhead scatter and '
              'occupancy scatter; the frame handed over ready, no configuration space; one CPU thread, %d updates)'
              % (kind, 1e3 * seconds[kind] / updates[kind], updates[kind]))
    print('of which the array expressions left of the configuration space: %.3f ms per update'
          % (1e3 * seconds['remainder'] / (updates['overhead'] + updates['forward'])))

if __name__ == '__main__':
    main()
