"""Mapper.update / get_state for the robots of the environments of one room written by hand as the chain of simq's public functions, stage by
stage as INTEGRATION.md writes it -- each function with its own checks, uploads and status read-back, and the source pixels of the
distance images moved to their closest free cells by the caller (an indexed read of `closest` that comes back to the host).
tests/test_gpu_mapper.py compares simq.BatchedMapper with it at every stage and tools/mapper_rate.py times the two side by side.
Configurations and robots are those of tests/mapper_oracle.py."""
import math

import numpy as np
import torch

import mapper_oracle as oracle


class Chain:
    """E environments of one room; mapper m = (environment e, robot r) counts through the environments in order."""

    def __init__(self, simq, room_width, room_length, types, masks, mask_names, receptacle_position, device='cuda'):
        self.simq, self.mask_names = simq, list(mask_names)
        self.pairs = [(e, r) for e, env in enumerate(types) for r in range(len(env))]
        self.types = [t for env in types for t in env]
        self.shape = oracle.padded_room_shape(room_width, room_length)
        self.room_mask = oracle.room_mask(room_width, room_length)
        self.radius = [oracle.radii(t)[0] for t in self.types]
        self.thin_radius = oracle.radii(self.types[0])[1]
        self.receptacle_position = receptacle_position
        M = len(self.types)
        self.overhead = torch.zeros((M,) + self.shape, dtype=torch.float32, device=device)
        self.occupancy = torch.zeros((M,) + self.shape, dtype=torch.uint8, device=device)
        self.bank = torch.from_numpy(np.ascontiguousarray(masks)).to(device)
        self.receptacle_map = torch.from_numpy(oracle.distance_to_receptacle_map(self.shape, receptacle_position, 0.25)).to(device)
        self.cspace, self.thin, self.closest = [None] * M, [None] * M, [None] * M

    def update(self, depth, ids, geometries, ranges, mappers=None):
        simq = self.simq
        ms = list(range(len(self.types))) if mappers is None else list(mappers)
        simq.observation_update(depth, ids, geometries, ranges, [self.overhead[m] for m in ms], [self.occupancy[m] for m in ms])
        got = simq.occupancy_maps([self.occupancy[m] for m in ms], [self.room_mask], [self.radius[m] for m in ms], self.thin_radius,
                                  room_index=[0] * len(ms))
        for p, m in enumerate(ms):
            self.cspace[m], self.thin[m], self.closest[m] = got.configuration_space[p], got.cspace_thin[p], got.closest_cspace_indices[p]

    def get_states(self, cfg, envs, mappers=None):
        """{'states': [P, 96, 96, C], 'images': the distance images in the order of the flags, 'history' / 'intention' / 'channels':
        the drawn maps} for the named mappers; envs: per environment its robots (tests/mapper_oracle.py dicts)."""
        simq, shape = self.simq, self.shape
        from simq.local_maps import RobotStamp, position_to_pixel_indices
        ms = list(range(len(self.types))) if mappers is None else list(mappers)
        P = len(ms)
        own = [self.pairs[m] for m in ms]
        out = {'images': [], 'history': None, 'intention': None, 'channels': None}
        maps = [self.overhead[m] for m in ms] + [self.receptacle_map]
        channels = [[('overhead', p)] for p in range(P)]
        if cfg['use_robot_map']:
            for ch in channels:
                ch.append('robots')
        if cfg['use_distance_to_receptacle_map']:
            for ch in channels:
                ch.append(('distance', P))
        pixels = []
        if cfg['use_shortest_path_to_receptacle_map']:
            pixels += [position_to_pixel_indices(self.receptacle_position[0], self.receptacle_position[1], shape)] * P
        if cfg['use_shortest_path_map']:
            pixels += [position_to_pixel_indices(envs[e][r]['position'][0], envs[e][r]['position'][1], shape) for e, r in own]
        if pixels:
            # the host-side snap: OccupancyMap._closest_valid_cspace_indices of every source pixel, read back to form the descriptors
            idx = list(range(P)) * (len(pixels) // P)
            closest = torch.stack([self.closest[m] for m in ms])
            px = torch.tensor(pixels, device=closest.device)
            k = torch.tensor(idx, device=closest.device)
            srcs = closest[k, :, px[:, 0], px[:, 1]].tolist()
            images = simq.grid_distance_images([self.cspace[m] for m in ms], srcs, grid_index=idx, pixels_per_meter=oracle.PIXELS_PER_METER,
                                               unreachable_to_max=True, scale=cfg['shortest_path_map_scale'])
            out['images'] = images
            for d in range(len(pixels) // P):
                for p, ch in enumerate(channels):
                    ch.append(('distance', len(maps) + d * P + p))
            maps += list(images)
        scale, thickness = cfg['intention_map_scale'], cfg['intention_map_line_thickness']
        for flag, name, enc in (('use_history_map', 'history', 'history'), ('use_intention_map', 'intention', cfg['intention_map_encoding'])):
            if cfg[flag]:
                out[name] = simq.intention_maps([oracle.drawn(envs[e], r, enc) for e, r in own], shape, enc, scale, thickness)
                for p, ch in enumerate(channels):
                    ch.append(('map', len(maps) + p))
                maps += list(out[name])
        if cfg['use_intention_channels']:
            order = []
            for e, r in own:
                dists = [oracle.distance(envs[e][r]['position'], other['position']) for other in envs[e]]
                order.append([int(k) for k in np.argsort(dists) if k != r])
            if cfg['intention_channel_encoding'] == 'spatial':
                paths = [[] if envs[e][k]['idle'] else [envs[e][k]['target']] for p, (e, r) in enumerate(own) for k in order[p]]
                out['channels'] = simq.intention_maps(paths, shape, 'circle', scale, thickness)
                at = len(maps)
                for p, ch in enumerate(channels):
                    ch += [('map', at + q) for q in range(len(order[p]))]
                    at += len(order[p])
                maps += list(out['channels'])
            else:
                for p, (e, r) in enumerate(own):
                    me = envs[e][r]
                    for k in order[p]:
                        other, relative_position = envs[e][k], (0, 0)
                        if not other['idle']:
                            dist = oracle.distance(me['position'], other['target'])
                            theta = me['heading'] - math.atan2(other['target'][1] - me['position'][1], other['target'][0] - me['position'][0])
                            relative_position = (dist * math.sin(theta), dist * math.cos(theta))
                        channels[p] += [('constant', float(np.float32(cfg['intention_channel_nonspatial_scale'] * c))) for c in relative_position]
        stamps = {}
        for e in sorted(set(e for e, _ in own)):
            stamps[e] = []
            for r in envs[e]:
                mine = self.mask_names.index(r['type'])
                lifting = r['type'] == 'lifting_robot' and r['lift_state'] == 'lifting'
                stamps[e].append(RobotStamp(r['position'], r['heading'], self.mask_names.index('lifting_robot_with_cube') if lifting else mine,
                                            oracle.SEG_VALUES['robot_group_%d' % (r['group'] + 1)],
                                            0.5 if r['type'] == 'lifting_robot' and not lifting else 1.0, mine))
        out['states'] = simq.local_state_images(maps, channels, [(envs[e][r]['position'], envs[e][r]['heading']) for e, r in own],
                                                robots=[stamps[e] for e, _ in own], masks=self.bank)
        return out
