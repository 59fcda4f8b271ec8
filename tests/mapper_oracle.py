"""numpy restatement of the reference's Mapper.update / Mapper.get_state with OccupancyMap.update (envs.py:2053-2112, 2444-2459) as the
chain of the pinned oracles of its stages, used by the mapper tests and by tools/gen_mapper_golden.py.  Nothing is restated twice: the
scatter is observation_maps_oracle, the configuration space occupancy_maps_oracle, the distances grid_paths_oracle, the drawn maps
intention_maps_oracle and the crop / rotation local_maps_oracle; this file holds the order of the stages, the order of the channels
and the few lines of envs.py that lie between them.

A configuration is a dict: the use_* flags (FLAGS), intention_map_encoding, intention_channel_encoding, intention_map_scale,
intention_map_line_thickness, intention_channel_nonspatial_scale, distance_to_receptacle_map_scale, shortest_path_map_scale.  A robot
is a dict: type, group, position (x, y), heading, lift_state, idle, target, intention_path, history_path.
"""
import math

import numpy as np

import grid_paths_oracle
import intention_maps_oracle
import local_maps_oracle
import observation_maps_oracle
import occupancy_maps_oracle

FLAGS = ('use_robot_map', 'use_distance_to_receptacle_map', 'use_shortest_path_to_receptacle_map', 'use_shortest_path_map', 'use_history_map',
         'use_intention_map', 'use_intention_channels')
NAMES = ('robots', 'distance_to_receptacle', 'shortest_path_to_receptacle', 'shortest_path', 'history', 'intention')
PIXELS_PER_METER = 96.0
HALF_WIDTH = 0.03                                                   # envs.py:803
BASE_LENGTH = {'pushing_robot': 0.065 + 0.005, 'lifting_robot': 0.065, 'throwing_robot': 0.065 + 0.006, 'rescue_robot': 0.065}   # envs.py:805, 1059, 1279
SEG_VALUES = {'floor': 1.0 / 8, 'obstacle': 2.0 / 8, 'receptacle': 3.0 / 8, 'cube': 4.0 / 8, 'robot_group_1': 5.0 / 8, 'robot_group_2': 6.0 / 8,
              'robot_group_3': 7.0 / 8, 'robot_group_4': 8.0 / 8}  # envs.py:1880-1889
DEFAULTS = {'intention_map_encoding': 'ramp', 'intention_channel_encoding': 'spatial', 'intention_map_scale': 1.0, 'intention_map_line_thickness': 2,
            'intention_channel_nonspatial_scale': 0.1, 'distance_to_receptacle_map_scale': 0.25, 'shortest_path_map_scale': 0.25}


def config(**given):
    cfg = dict({f: False for f in FLAGS}, **DEFAULTS)
    assert set(given) <= set(cfg), sorted(set(given) - set(cfg))
    cfg.update(given)
    return cfg


def round_up_to_even(x):
    return 2 * math.ceil(x / 2)                                     # envs.py:2404-2406


def padded_room_shape(room_width, room_length):
    return (round_up_to_even(room_width * PIXELS_PER_METER + math.sqrt(2) * 96), round_up_to_even(room_length * PIXELS_PER_METER + math.sqrt(2) * 96))


def room_mask(room_width, room_length):
    """envs.py:2467-2475."""
    mask = np.zeros(padded_room_shape(room_width, room_length), np.uint8)
    length_pixels = round_up_to_even((room_length - 2 * HALF_WIDTH) * PIXELS_PER_METER)
    width_pixels = round_up_to_even((room_width - 2 * HALF_WIDTH) * PIXELS_PER_METER)
    start_i, start_j = int(mask.shape[0] / 2 - width_pixels / 2), int(mask.shape[1] / 2 - length_pixels / 2)
    mask[start_i:start_i + width_pixels, start_j:start_j + length_pixels] = 1
    return mask


def radii(robot_type):
    """(radius, thin_radius) of the two disks of OccupancyMap.__init__ (envs.py:2420, 2428)."""
    radius = math.sqrt(HALF_WIDTH**2 + (-0.0135 + BASE_LENGTH[robot_type])**2)      # envs.py:804, 807-808
    return math.floor(radius * PIXELS_PER_METER), math.ceil(HALF_WIDTH * PIXELS_PER_METER)


def distance(p1, p2):
    return math.sqrt((p2[0] - p1[0])**2 + (p2[1] - p1[1])**2)       # envs.py:2556-2557


def distance_to_receptacle_map(shape, receptacle_position, scale):
    """envs.py:2277-2285."""
    out = np.zeros(shape, np.float32)
    for i in range(shape[0]):
        for j in range(shape[1]):
            pos_x = ((j + 0.5) - shape[1] / 2) / PIXELS_PER_METER     # envs.py:2398-2402
            pos_y = (shape[0] / 2 - (i + 0.5)) / PIXELS_PER_METER
            out[i, j] = distance((pos_x, pos_y), receptacle_position)
    out *= scale
    return out


def channel_names(cfg, n_robots):
    """The channels of get_state in its order (envs.py:2067-2112)."""
    names = ['overhead'] + [n for f, n in zip(FLAGS[:6], NAMES) if cfg[f]]
    if cfg['use_intention_channels']:
        per = 1 if cfg['intention_channel_encoding'] == 'spatial' else 2
        names += ['intention_channel_%d' % k for k in range(per * (n_robots - 1))]
    return names


class Maps:
    """The persistent maps of one Mapper and its OccupancyMap."""

    def __init__(self, room_width, room_length, robot_type):
        self.shape = padded_room_shape(room_width, room_length)
        self.overhead = np.zeros(self.shape, np.float32)           # envs.py:2025
        self.occupancy = np.zeros(self.shape, np.uint8)            # envs.py:2416
        self.room_mask = room_mask(room_width, room_length)
        self.radius, self.thin_radius = radii(robot_type)
        self.configuration_space = self.cspace_thin = self.closest = None

    def update(self, depth, ids, geometry, ranges):
        """Mapper.update with OccupancyMap.update; returns the status word of the scatter."""
        status = observation_maps_oracle.update(self.overhead, self.occupancy, depth, ids, geometry, ranges)
        self.configuration_space, self.cspace_thin, self.closest = occupancy_maps_oracle.update(self.occupancy, self.room_mask, self.radius,
                                                                                                 self.thin_radius)
        return status

    def shortest_path_map(self, position, scale):
        """envs.py:2287-2299 on envs.py:2513-2516."""
        i, j = local_maps_oracle.position_to_pixel_indices(position[0], position[1], self.shape)
        source = (int(self.closest[0, i, j]), int(self.closest[1, i, j]))
        return grid_paths_oracle.mapper_image(grid_paths_oracle.distance_image(self.configuration_space, source), PIXELS_PER_METER, scale)


def stamps(robots, mask_names, shape, seg_values=SEG_VALUES):
    """The robots of an environment as local_maps_oracle.global_robot_map takes them (envs.py:2250-2275)."""
    out = []
    for r in robots:
        own = mask_names.index(r['type'])
        lifting = r['type'] == 'lifting_robot' and r['lift_state'] == 'lifting'
        out.append((local_maps_oracle.position_to_pixel_indices(r['position'][0], r['position'][1], shape), local_maps_oracle.mask_rotation(r['heading']),
                    mask_names.index('lifting_robot_with_cube') if lifting else own, seg_values['robot_group_%d' % (r['group'] + 1)],
                    0.5 if r['type'] == 'lifting_robot' and not lifting else 1.0, own))
    return out


def drawn(robots, own, encoding):
    """The paths Mapper._create_global_intention_or_history_map reads (envs.py:2303-2317)."""
    key = 'target' if encoding == 'circle' else 'history_path' if encoding == 'history' else 'intention_path'
    return [r[key] for k, r in enumerate(robots) if k != own and not r['idle']]


def channel_images(cfg, maps, robots, own, masks, mask_names, receptacle_position=None, receptacle_map=None):
    """{channel name: float32 [96, 96]} of Mapper.get_state for robot `own` of `robots`, whose maps are `maps`; receptacle_map: the
    precomputed distance_to_receptacle_map (computed here when omitted)."""
    me, shape = robots[own], maps.shape
    pixel = local_maps_oracle.position_to_pixel_indices(me['position'][0], me['position'][1], shape)
    rot = local_maps_oracle.crop_rotation(me['heading'])
    st = stamps(robots, mask_names, shape)
    out = {'overhead': local_maps_oracle.local_map(local_maps_oracle.global_overhead_map(maps.overhead, st, masks), pixel, rot)}
    if cfg['use_robot_map']:
        out['robots'] = local_maps_oracle.local_map(local_maps_oracle.global_robot_map(shape, st, masks, False), pixel, rot)
    if cfg['use_distance_to_receptacle_map']:
        if receptacle_map is None:
            receptacle_map = distance_to_receptacle_map(shape, receptacle_position, cfg['distance_to_receptacle_map_scale'])
        out['distance_to_receptacle'] = local_maps_oracle.local_distance_map(receptacle_map, pixel, rot)
    if cfg['use_shortest_path_to_receptacle_map']:
        out['shortest_path_to_receptacle'] = local_maps_oracle.local_distance_map(
            maps.shortest_path_map(receptacle_position, cfg['shortest_path_map_scale']), pixel, rot)
    if cfg['use_shortest_path_map']:
        out['shortest_path'] = local_maps_oracle.local_distance_map(maps.shortest_path_map(me['position'], cfg['shortest_path_map_scale']), pixel, rot)
    scale, thickness = cfg['intention_map_scale'], cfg['intention_map_line_thickness']
    if cfg['use_history_map']:
        out['history'] = local_maps_oracle.local_map(intention_maps_oracle.global_map(drawn(robots, own, 'history'), shape, 'history', scale, thickness),
                                                     pixel, rot)
    if cfg['use_intention_map']:
        enc = cfg['intention_map_encoding']
        out['intention'] = local_maps_oracle.local_map(intention_maps_oracle.global_map(drawn(robots, own, enc), shape, enc, scale, thickness), pixel, rot)
    if cfg['use_intention_channels']:
        dists = [distance(me['position'], r['position']) for r in robots]
        k = 0
        for i in np.argsort(dists):                                 # envs.py:2350-2358
            other = robots[i]
            if i == own:
                continue
            if cfg['intention_channel_encoding'] == 'spatial':
                gm = intention_maps_oracle.global_map([] if other['idle'] else [other['target']], shape, 'circle', scale, thickness)
                out['intention_channel_%d' % k] = local_maps_oracle.local_map(gm, pixel, rot)
                k += 1
                continue
            relative_position = (0, 0)                              # envs.py:2368-2375
            if not other['idle']:
                dist = distance(me['position'], other['target'])
                theta = me['heading'] - math.atan2(other['target'][1] - me['position'][1], other['target'][0] - me['position'][0])
                relative_position = (dist * math.sin(theta), dist * math.cos(theta))
            for coord in relative_position:
                out['intention_channel_%d' % k] = cfg['intention_channel_nonspatial_scale'] * coord * np.ones((96, 96), np.float32)
                k += 1
    return out


def get_state(cfg, maps, robots, own, masks, mask_names, receptacle_position=None, receptacle_map=None):
    """Mapper.get_state(): float32 [96, 96, C]."""
    images = channel_images(cfg, maps, robots, own, masks, mask_names, receptacle_position, receptacle_map)
    planes = [images[n] for n in channel_names(cfg, len(robots))]
    assert all(p.dtype == np.float32 for p in planes)
    return np.stack(planes, axis=2)


# ---- fixtures (tools/gen_mapper_golden.py) ------------------------------------------------------------------------------------------
ENCODINGS = ('circle', 'ramp', 'binary', 'line', 'history')


def configurations():
    """name -> configuration: the channel configurations that differ in code path.  Every use_* flag alone, the four intention
    encodings, the history map, both kinds of intention channels, and all channels together (with each kind of channels)."""
    out = {'overhead_only': config()}
    for f in FLAGS[:5]:
        out[f] = config(**{f: True})
    for enc in ENCODINGS[:4]:
        out['use_intention_map_' + enc] = config(use_intention_map=True, intention_map_encoding=enc)
    for enc in ('spatial', 'nonspatial'):
        out['use_intention_channels_' + enc] = config(use_intention_channels=True, intention_channel_encoding=enc)
        out['full_' + enc] = config(**dict({f: True for f in FLAGS}, intention_channel_encoding=enc))
    return out


def load_fixture(path):
    """A tests/golden/mapper_*.npz file: the room, the robots of the environment, the masks, and per round the camera frames
    (depth, ids, geometry, id ranges per robot), the robots' states and the expected channel images {name: [R, 96, 96]} -- one image
    per distinct channel (the intention map once per encoding, the intention channels once per kind); a configuration's expected state
    is `expected_state`."""
    z = np.load(path)
    n_robots, n_rounds = len(z['robot_type']), int(z['rounds'])
    mask_names = [str(s) for s in z['mask_names']]
    fx = {'room_width': float(z['room'][0]), 'room_length': float(z['room'][1]), 'receptacle_position': tuple(float(x) for x in z['receptacle_position']),
          'types': [str(s) for s in z['robot_type']], 'groups': [int(g) for g in z['robot_group']], 'masks': z['masks'], 'mask_names': mask_names,
          'rounds': []}
    for t in range(n_rounds):
        robots, frames = [], []
        for r in range(n_robots):
            k = t * n_robots + r
            ways = {}
            for name in ('intention', 'history'):
                sel = (z['way_round'] == t) & (z['way_robot'] == r) & (z['way_kind'] == (0 if name == 'intention' else 1))
                ways[name] = [tuple(float(x) for x in w) for w in z['way_xyz'][sel]]
            idle = bool(z['state_idle'][k])
            robots.append({'type': fx['types'][r], 'group': fx['groups'][r], 'position': tuple(float(x) for x in z['state_position'][k]),
                           'heading': float(z['state_heading'][k]), 'lift_state': str(z['state_lift'][k]) or None, 'idle': idle,
                           'target': None if idle else tuple(float(x) for x in z['state_target'][k]),
                           'intention_path': None if idle else ways['intention'], 'history_path': None if idle else ways['history']})
            v, c, ids = z['frame_vectors'][k], z['frame_depth_constants'][k], z['frame_id_ranges'][k].tolist()
            frames.append({'depth': z['frame_depth'][k], 'ids': z['frame_ids'][k],
                           'geometry': observation_maps_oracle.Geometry(v[0], v[1], v[2], v[3], z['frame_pixel_x'][k], z['frame_pixel_y'][k], c[0], c[1], c[2]),
                           'ranges': observation_maps_oracle.IdRanges(ids[0], ids[1], ids[2] if ids[3] else None, ids[4], ids[5])})
        images = {name[len('image_'):]: z[name][t * n_robots:(t + 1) * n_robots] for name in z.files if name.startswith('image_')}
        fx['rounds'].append({'robots': robots, 'frames': frames, 'images': images})
    return fx


def image_key(cfg, name):
    """The stored image of channel `name` under configuration `cfg`."""
    if name == 'intention':
        return 'intention_' + cfg['intention_map_encoding']
    if name.startswith('intention_channel_'):
        return '%s_%s' % (cfg['intention_channel_encoding'], name)
    return name


def expected_state(cfg, images, robot, n_robots):
    """The expected float32 [96, 96, C] state of `robot` in a round whose stored images are `images`."""
    return np.stack([images[image_key(cfg, n)][robot] for n in channel_names(cfg, n_robots)], axis=2)
