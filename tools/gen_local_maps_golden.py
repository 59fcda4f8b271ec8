"""Write tests/golden/local_maps_*.npz: local state images computed by the reference's own Mapper (envs.py).

    python tools/gen_local_maps_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and scipy.  envs.py is imported as it is, with empty stand-in modules for what it imports but the local-map
code never touches (pybullet, anki_vector, skimage, vector_utils, shortest_paths); nothing of it is copied or kept.  The expected images
come from Mapper._get_local_map, _get_local_distance_map, _create_global_robot_map and _create_global_overhead_map called on bare
Mapper / robot instances whose attributes this file sets (poses, masks from Mapper._create_robot_mask, Camera.SEG_VALUES); the robot
masks are the reference's too.  Every image is asserted equal, bit for bit, to tests/local_maps_oracle.py before anything is written, and
the float64 rotation matrices / offsets / shapes are stored beside the poses so that a consumer of the fixtures needs no scipy.  Also
prints the reference's host time per state (one CPU thread).
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

import local_maps_oracle as oracle                                  # noqa: E402
from grid_paths_oracle import distance_image, mapper_image          # noqa: E402

CHANNELS = (('map', 0), ('distance', 1), ('overhead', 2), 'robots', ('map', 1), ('constant', -0.3125))
KIND_CODES = {'map': 0, 'distance': 1, 'robots': 2, 'overhead': 3, 'constant': 4}
MASK_NAMES = ('pushing_robot', 'lifting_robot', 'lifting_robot_with_cube', 'throwing_robot', 'rescue_robot')


def import_reference(ref):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def absent(*args, **kwargs):
        raise NotImplementedError('not part of the local-map path')

    for name in ('anki_vector', 'pybullet', 'pybullet_utils', 'pybullet_utils.bullet_client', 'skimage', 'vector_utils', 'shortest_paths'):
        stub(name)
    stub('skimage.draw', line=absent)
    stub('skimage.morphology', binary_dilation=absent, dilation=absent)
    stub('skimage.morphology.selem', disk=absent)
    stub('shortest_paths.shortest_paths', GridGraph=object)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import envs
    return envs


# ---- synthetic global maps -----------------------------------------------------------------------------------------------------
def palette_map(rng, rows, cols):
    """Random fp32 values, negative and > 1 included, drawn from 4096 distinct ones (so that the file compresses)."""
    palette = (rng.uniform(-2.0, 3.0, 4096)).astype(np.float32)
    return palette[rng.randint(0, 4096, (rows, cols))]


def mapper_distance_map(rng, rows, cols, room_rows, room_cols):
    """A Mapper-style shortest-path map: distances in a cluttered room / 96, unreachable -> max, * 0.25 (envs.py:2294-2299)."""
    g = np.zeros((rows, cols), np.uint8)
    i0, j0 = rows // 2 - room_rows // 2, cols // 2 - room_cols // 2
    g[i0:i0 + room_rows, j0:j0 + room_cols] = 1
    for _ in range(5):
        i, j = i0 + rng.randint(room_rows - 8), j0 + rng.randint(room_cols - 8)
        g[i:i + 8, j:j + 8] = 0
    ii, jj = np.nonzero(g)
    k = rng.randint(ii.size)
    return mapper_image(distance_image(g, (int(ii[k]), int(jj[k]))), 96.0, 0.25)


def overhead_base_map(rng, rows, cols, room_rows, room_cols, seg):
    """An overhead map without robots: floor inside the room, obstacle walls around it, a receptacle and cubes (values <= 1)."""
    m = np.zeros((rows, cols), np.float32)
    i0, j0 = rows // 2 - room_rows // 2, cols // 2 - room_cols // 2
    m[i0 - 3:i0 + room_rows + 3, j0 - 3:j0 + room_cols + 3] = seg['obstacle']
    m[i0:i0 + room_rows, j0:j0 + room_cols] = seg['floor']
    m[i0:i0 + 14, j0 + room_cols - 14:j0 + room_cols] = seg['receptacle']
    for _ in range(8):
        i, j = i0 + rng.randint(room_rows - 4), j0 + rng.randint(room_cols - 4)
        m[i:i + 4, j:j + 4] = seg['cube']
    return m


def extreme_position(shape, low_i, low_j):
    """A position whose pixel is the legal extreme (68 or size - 68) along each axis."""
    pi = 68 if low_i else shape[0] - 68
    pj = 68 if low_j else shape[1] - 68
    return (pj + 0.5 - shape[1] / 2) / 96.0, (shape[0] / 2 - pi - 0.5) / 96.0


def environments(rng, shape):
    """Three environments of four robots: (position, heading, class name, group index, lift state)."""
    e1, e2 = extreme_position(shape, True, False), extreme_position(shape, False, True)
    u = lambda: (rng.uniform(-0.4, 0.4), rng.uniform(-0.18, 0.18))
    a = [((0.10, 0.05), 0.0, 'PushingRobot', 0, None), ((0.13, 0.06), math.pi / 2, 'LiftingRobot', 1, 'ready'),       # two overlapping
         ((-0.2, -0.1), -math.pi / 2, 'LiftingRobot', 1, 'lifting'), (e1, math.pi, 'PushingRobot', 0, None)]
    b = [(u(), math.pi / 4, 'ThrowingRobot', 2, None), (u(), -math.pi / 4, 'RescueRobot', 3, None),
         (u(), math.pi / 6, 'LiftingRobot', 0, 'lifting'), (e2, -3 * math.pi / 4, 'LiftingRobot', 0, 'ready')]
    c = [(u(), rng.uniform(-math.pi, math.pi), 'PushingRobot', 0, None), (u(), rng.uniform(-math.pi, math.pi), 'PushingRobot', 0, None),
         (extreme_position(shape, True, True), rng.uniform(-math.pi, math.pi), 'ThrowingRobot', 1, None),
         (extreme_position(shape, False, False), rng.uniform(-math.pi, math.pi), 'LiftingRobot', 2, 'ready')]
    return [a, b, c]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    envs = import_reference(os.path.abspath(args.reference))
    Mapper = envs.Mapper
    seg = envs.Camera.SEG_VALUES
    classes = {n: getattr(envs, n) for n in ('PushingRobot', 'LiftingRobot', 'ThrowingRobot', 'RescueRobot')}
    ref_masks = {cls: Mapper._create_robot_mask(cls) for cls in classes.values()}
    ref_masks['lifting_robot_with_cube'] = Mapper._create_robot_mask(envs.LiftingRobot, show_lifted_cube=True)
    masks = np.stack([ref_masks[envs.PushingRobot], ref_masks[envs.LiftingRobot], ref_masks['lifting_robot_with_cube'],
                      ref_masks[envs.ThrowingRobot], ref_masks[envs.RescueRobot]])
    mask_index = {'PushingRobot': 0, 'LiftingRobot': 1, 'ThrowingRobot': 3, 'RescueRobot': 4}
    camera = types.SimpleNamespace(get_seg_value=lambda body_type: seg[body_type])
    total_images, ref_seconds, ref_states = 0, 0.0, 0

    for fname, room_width, room_length, seed in (('local_maps_184x232.npz', 0.5, 1.0, 21), ('local_maps_232x232.npz', 1.0, 1.0, 22)):
        rng = np.random.RandomState(seed)
        shape = Mapper.create_padded_room_zeros(room_width, room_length).shape
        room = (int(room_width * 96) - 4, int(room_length * 96) - 4)
        maps = np.stack([palette_map(rng, *shape), mapper_distance_map(rng, *shape, *room), overhead_base_map(rng, *shape, *room, seg)])
        rows = {k: [] for k in ('position', 'heading', 'pixel', 'R', 'offset', 'shape', 'env')}
        rob = {k: [] for k in ('env', 'position', 'heading', 'pixel', 'mask', 'seg_mask', 'seg_value', 'map_value', 'R', 'offset', 'shape')}
        states = []
        for e, env_robots in enumerate(environments(rng, shape)):
            robots, stamps = [], []
            for position, heading, cls, group, lift in env_robots:
                r = object.__new__(classes[cls])
                r.get_position = lambda p=position: (p[0], p[1], 0.0)
                r.get_heading = lambda h=heading: h
                r.group_index, r.lift_state = group, lift
                robots.append(r)
                # the oracle's description of the same robot
                lifting = cls == 'LiftingRobot'
                mask = 2 if lifting and lift == 'lifting' else mask_index[cls]
                value = 0.5 if lifting and lift != 'lifting' else 1.0
                pixel = oracle.position_to_pixel_indices(position[0], position[1], shape)
                rot = oracle.mask_rotation(heading)
                stamps.append((pixel, rot, mask, seg['robot_group_%d' % (group + 1)], value, mask_index[cls]))
                for k, v in zip(('env', 'position', 'heading', 'pixel', 'mask', 'seg_mask', 'seg_value', 'map_value', 'R', 'offset', 'shape'),
                                (e, position, heading, pixel, mask, mask_index[cls], seg['robot_group_%d' % (group + 1)], value,
                                 rot[0].reshape(-1), rot[1], rot[2])):
                    rob[k].append(v)
            env = types.SimpleNamespace(robots=robots, room_width=room_width, room_length=room_length)
            for r, (position, heading, _, _, _) in zip(robots, env_robots):
                m = object.__new__(Mapper)
                m.env, m.robot, m.robot_masks, m.camera = env, r, ref_masks, camera
                m.global_overhead_map_without_robots = maps[2]
                t0 = time.perf_counter()
                planes = [m._get_local_map(maps[0]), m._get_local_distance_map(maps[1]), m._get_local_map(m._create_global_overhead_map()),
                          m._get_local_map(m._create_global_robot_map(seg=False)), m._get_local_map(maps[1]),
                          np.float32(CHANNELS[5][1]) * np.ones((96, 96), np.float32)]
                ref_seconds += time.perf_counter() - t0
                ref_states += 1
                want = np.stack([np.asarray(p, np.float32) for p in planes], axis=2)
                pixel = oracle.position_to_pixel_indices(position[0], position[1], shape)
                assert pixel == tuple(int(x) for x in Mapper.position_to_pixel_indices(position[0], position[1], shape))
                rot = oracle.crop_rotation(heading)
                got = oracle.state(maps, CHANNELS, pixel, rot, stamps, masks)
                assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (96, 96, len(CHANNELS))
                for c in range(len(CHANNELS)):
                    assert np.array_equal(got[:, :, c].view(np.int32), np.ascontiguousarray(want[:, :, c]).view(np.int32)), \
                        (fname, e, position, heading, CHANNELS[c])
                states.append(want)
                for k, v in zip(('position', 'heading', 'pixel', 'R', 'offset', 'shape', 'env'),
                                (position, heading, pixel, rot[0].reshape(-1), rot[1], rot[2], e)):
                    rows[k].append(v)
        arrays = {'maps': maps, 'masks': masks, 'mask_names': np.asarray(MASK_NAMES), 'states': np.stack(states),
                  'channel_kind': np.asarray([KIND_CODES[c if isinstance(c, str) else c[0]] for c in CHANNELS], np.int32),
                  'channel_map': np.asarray([0 if isinstance(c, str) or c[0] == 'constant' else c[1] for c in CHANNELS], np.int32),
                  'channel_value': np.asarray([c[1] if not isinstance(c, str) and c[0] == 'constant' else 0 for c in CHANNELS], np.float32)}
        for k, v in rows.items():
            arrays['pose_' + k] = np.asarray(v, np.int32 if k in ('pixel', 'shape', 'env') else np.float64)
        for k, v in rob.items():
            arrays['robot_' + k] = np.asarray(v, np.int32 if k in ('pixel', 'shape', 'env', 'mask', 'seg_mask') else np.float64)
        path = os.path.join(args.out, fname)
        np.savez_compressed(path, **arrays)
        n = len(states) * len(CHANNELS)
        total_images += n
        print('%s: %d states, %d local images, %d bytes' % (path, len(states), n, os.path.getsize(path)))
        assert os.path.getsize(path) < 1 << 20
    print('%d local images; reference Mapper on the host: %.2f ms per %d-channel state (scipy %s, one CPU thread)'
          % (total_images, 1e3 * ref_seconds / ref_states, len(CHANNELS), __import__('scipy').__version__))


if __name__ == '__main__':
    main()
