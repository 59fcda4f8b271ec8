"""numpy restatement of the local-map stage of the reference's Mapper (envs.py:2199-2275), used by the local-map tests.

``scipy.ndimage.rotate(image [n, n], angle, order=0)`` with its defaults maps output index (oi, oj) of the rotated image to the input
coordinate  cc_h = offset[h] + (oi * R[h][0] + oj * R[h][1])  in float64 -- the two products summed first, then the offset -- and
takes input pixel floor(cc_h + 0.5) when 0 <= cc_h <= n - 1, else 0.  R = [[c, s], [-s, c]] with c, s = cosdg(angle), sindg(angle),
the rotated shape is int(ptp(R @ corners) + 0.5) per axis and offset = (n - 1) / 2 - R @ ((shape - 1) / 2).  A rotation is the triple
(R, offset, shape); every function below takes such triples, so a test can feed the doubles a fixture stores and needs no scipy.
Unlike the kernel, which samples robot stamps per local pixel, the robot and overhead maps are materialised here as the reference
materialises them: whole masks rotated, stamped with np.maximum into a global map, then cropped and rotated.
"""
import math

import numpy as np

WIDTH = 96
CROP = 136
PIXELS_PER_METER = 96.0


def rotation(angle, n):
    """The (R, offset, shape) rotate() forms for an [n, n] image, in its own sequence of float64 operations (needs scipy.special)."""
    from scipy import special
    c, s = special.cosdg(angle), special.sindg(angle)
    rot = np.array([[c, s], [-s, c]])
    shape = (np.ptp(rot @ [[0, 0, n, n], [0, n, 0, n]], axis=1) + 0.5).astype(int)
    offset = (np.asarray((n, n)) - 1) / 2 - rot @ ((shape - 1) / 2)
    return rot, offset, shape


def crop_rotation(heading):
    return rotation(90 - math.degrees(heading), CROP)            # envs.py:2202


def mask_rotation(heading):
    return rotation(math.degrees(heading) - 90, WIDTH)           # envs.py:2265


def position_to_pixel_indices(position_x, position_y, image_shape):
    """envs.py:2391-2396."""
    pixel_i = np.floor(image_shape[0] / 2 - position_y * PIXELS_PER_METER).astype(np.int32)
    pixel_j = np.floor(image_shape[1] / 2 + position_x * PIXELS_PER_METER).astype(np.int32)
    return int(np.clip(pixel_i, 0, image_shape[0] - 1)), int(np.clip(pixel_j, 0, image_shape[1] - 1))


def sample(image, rot, oi, oj, offset_first=False):
    """image [n, n] at the rotated-image indices (oi, oj) (float64 arrays of whole numbers): the order-0 rule above.  offset_first:
    the WRONG evaluation order (offset + oi * R0) + oj * R1, kept so that a test can show that its cases tell the two apart."""
    R, offset, _ = rot
    n = image.shape[0]
    if offset_first:
        c0 = (offset[0] + oi * R[0][0]) + oj * R[0][1]
        c1 = (offset[1] + oi * R[1][0]) + oj * R[1][1]
    else:
        c0 = offset[0] + (oi * R[0][0] + oj * R[0][1])
        c1 = offset[1] + (oi * R[1][0] + oj * R[1][1])
    inside = (c0 >= 0) & (c0 <= n - 1) & (c1 >= 0) & (c1 <= n - 1)
    i0 = np.clip(np.floor(c0 + 0.5).astype(int), 0, n - 1)
    i1 = np.clip(np.floor(c1 + 0.5).astype(int), 0, n - 1)
    return np.where(inside, image[i0, i1], np.float32(0)).astype(np.float32)


def rotate_whole(image, rot):
    """rotate(image, angle, order=0): every pixel of the rotated image."""
    shape = rot[2]
    oi, oj = np.meshgrid(np.arange(float(shape[0])), np.arange(float(shape[1])), indexing='ij')
    return sample(image, rot, oi, oj)


def local_map(global_map, pixel, rot, offset_first=False):
    """Mapper._get_local_map (envs.py:2199-2210) for a robot at `pixel` with crop rotation `rot`."""
    pi, pj = pixel
    h = CROP // 2
    assert h <= pi <= global_map.shape[0] - h and h <= pj <= global_map.shape[1] - h, 'the crop leaves the map'
    crop = global_map[pi - h:pi + h, pj - h:pj + h]
    shape = rot[2]
    oi, oj = np.meshgrid(np.arange(float(WIDTH)) + (shape[0] // 2 - WIDTH // 2), np.arange(float(WIDTH)) + (shape[1] // 2 - WIDTH // 2),
                         indexing='ij')
    return sample(crop, rot, oi, oj, offset_first)


def local_distance_map(global_map, pixel, rot):
    """Mapper._get_local_distance_map (envs.py:2212-2215)."""
    m = local_map(global_map, pixel, rot)
    m -= m.min()
    return m


def global_robot_map(shape, robots, masks, seg):
    """Mapper._create_global_robot_map (envs.py:2250-2275).  robots: (pixel, rot, mask index, seg value, map value, seg mask index) per
    robot; seg=True draws seg_value * masks[seg mask] (the class's own mask), seg=False map_value * masks[mask] (with the cube when lifting)."""
    out = np.zeros(shape, np.float32)
    for pixel, rot, mask, seg_value, map_value, seg_mask in robots:
        vis = masks[seg_mask if seg else mask] * np.float32(seg_value if seg else map_value)
        rotated = rotate_whole(vis, rot)
        si, sj = pixel[0] - rotated.shape[0] // 2, pixel[1] - rotated.shape[1] // 2
        assert si >= 0 and sj >= 0 and si + rotated.shape[0] <= shape[0] and sj + rotated.shape[1] <= shape[1], 'the stamp leaves the map'
        out[si:si + rotated.shape[0], sj:sj + rotated.shape[1]] = np.maximum(out[si:si + rotated.shape[0], sj:sj + rotated.shape[1]], rotated)
    return out


def global_overhead_map(base, robots, masks):
    """Mapper._create_global_overhead_map (envs.py:2243-2248)."""
    out = base.copy()
    seg = global_robot_map(base.shape, robots, masks, True)
    out[seg > 0] = seg[seg > 0]
    return out


def state(maps, channels, pixel, rot, robots=(), masks=None, map_shape=None):
    """The [96, 96, C] float32 state of one robot.  channels: (kind, argument) as simq.local_state_images takes them."""
    planes = []
    for spec in channels:
        kind, arg = (spec, None) if isinstance(spec, str) else (spec[0], spec[1] if len(spec) > 1 else None)
        if kind == 'map':
            planes.append(local_map(maps[arg], pixel, rot))
        elif kind == 'distance':
            planes.append(local_distance_map(maps[arg], pixel, rot))
        elif kind == 'robots':
            shape = map_shape if map_shape is not None else maps[0].shape
            planes.append(local_map(global_robot_map(shape, robots, masks, False), pixel, rot))
        elif kind == 'overhead':
            planes.append(local_map(global_overhead_map(maps[arg], robots, masks), pixel, rot))
        elif kind == 'constant':
            planes.append(np.full((WIDTH, WIDTH), np.float32(arg), np.float32))
        else:
            raise ValueError(spec)
    return np.stack(planes, axis=2)


KIND_NAMES = ('map', 'distance', 'robots', 'overhead', 'constant')


def load_fixture(path):
    """A tests/golden/local_maps_*.npz file (tools/gen_local_maps_golden.py) in this module's terms: maps [G, rows, cols], masks,
    the channel list, the expected states [P, 96, 96, C], and per state its pose, pixel, stored crop rotation and environment; per
    environment the robots as global_robot_map takes them (stored mask rotations) and as (position, heading, ...) tuples."""
    z = np.load(path)
    channels = []
    for kind, k, v in zip(z['channel_kind'], z['channel_map'], z['channel_value']):
        name = KIND_NAMES[int(kind)]
        channels.append(name if name == 'robots' else (name, float(v)) if name == 'constant' else (name, int(k)))
    envs, env_poses = {}, {}
    for r in range(len(z['robot_env'])):
        rot = (z['robot_R'][r].reshape(2, 2), z['robot_offset'][r], z['robot_shape'][r])
        e = int(z['robot_env'][r])
        envs.setdefault(e, []).append((tuple(int(x) for x in z['robot_pixel'][r]), rot, int(z['robot_mask'][r]), float(z['robot_seg_value'][r]),
                                       float(z['robot_map_value'][r]), int(z['robot_seg_mask'][r])))
        env_poses.setdefault(e, []).append((tuple(z['robot_position'][r]), float(z['robot_heading'][r]), int(z['robot_mask'][r]),
                                            float(z['robot_seg_value'][r]), float(z['robot_map_value'][r]), int(z['robot_seg_mask'][r])))
    states = []
    for p in range(len(z['pose_env'])):
        states.append({'position': tuple(z['pose_position'][p]), 'heading': float(z['pose_heading'][p]),
                       'pixel': tuple(int(x) for x in z['pose_pixel'][p]),
                       'rot': (z['pose_R'][p].reshape(2, 2), z['pose_offset'][p], z['pose_shape'][p]), 'env': int(z['pose_env'][p])})
    return {'maps': z['maps'], 'masks': z['masks'], 'channels': channels, 'want': z['states'], 'states': states, 'robots': envs,
            'robot_poses': env_poses}
