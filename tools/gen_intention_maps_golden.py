"""Write tests/golden/intention_maps_*.npz: global intention / history maps drawn by the reference's own Mapper (envs.py).

    python tools/gen_intention_maps_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and scipy.  envs.py is imported as it is, with empty stand-in modules for what it imports but this code
never touches (pybullet, anki_vector, vector_utils, shortest_paths).  scikit-image, a third-party package the reference imports, is
replaced by stand-ins of the three names the intention maps use: skimage.draw.line is the published sequential line algorithm
(tests/intention_maps_oracle.py: sequential_line), skimage.morphology.dilation is scipy.ndimage.grey_dilation(image, footprint=selem)
-- the call scikit-image's own dilation makes -- and skimage.morphology.selem.disk is the x^2 + y^2 <= r^2 footprint.  Nothing of the
reference is copied or kept.  The expected maps come from Mapper._create_global_intention_or_history_map, Mapper._get_intention_channels
and Mapper._get_local_map called on bare Mapper instances whose attributes this file sets (robots with poses, targets and waypoint
lists).  Every map is asserted equal, bit for bit, to tests/intention_maps_oracle.py before anything is written, and the float64 ramp
parameters are stored beside the paths.  Also prints the reference's host time per map (one CPU thread, with the scipy stand-in for
scikit-image's dilation).
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

import intention_maps_oracle as oracle                              # noqa: E402


def import_reference(ref):
    from scipy import ndimage

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def absent(*args, **kwargs):
        raise NotImplementedError('not part of the intention-map path')

    for name in ('anki_vector', 'pybullet', 'pybullet_utils', 'pybullet_utils.bullet_client', 'skimage', 'vector_utils', 'shortest_paths'):
        stub(name)
    stub('skimage.draw', line=oracle.sequential_line)
    stub('skimage.morphology', binary_dilation=absent, dilation=lambda image, selem: ndimage.grey_dilation(image, footprint=selem))
    stub('skimage.morphology.selem', disk=oracle.disk)
    stub('shortest_paths.shortest_paths', GridGraph=object)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import envs
    return envs


def robot(position, heading=0.0, intention=None, history=None, target=None, idle=False):
    """What the Mapper reads of a robot; an idle one has no paths (its controller returns None)."""
    p = (position[0], position[1], 0.0)
    controller = types.SimpleNamespace(get_intention_path=lambda: None if idle else list(intention),
                                       get_history_path=lambda: None if idle else list(history))
    return types.SimpleNamespace(get_position=lambda: p, get_heading=lambda: heading, is_idle=lambda: idle, controller=controller,
                                 target_end_effector_position=None if target is None else (target[0], target[1], 0.0),
                                 paths={'intention': intention, 'history': history, 'target': target})


def at(shape, i, j, di=0.5, dj=0.5):
    """A position inside pixel (i, j) of a map of `shape`."""
    return ((j + dj - shape[1] / 2) / 96.0, (shape[0] / 2 - i - di) / 96.0, 0.0)


STAR = [(0, 20), (7, 20), (20, 20), (20, 7), (20, 0), (20, -7), (20, -20), (7, -20), (0, -20), (-7, -20), (-20, -20), (-20, -7), (-20, 0),
        (-20, 7), (-20, 20), (-7, 20)]


def environments(shape):
    """name -> (robots, index of the mapper's own robot)."""
    rows, cols = shape
    ci, cj = rows // 2, cols // 2
    # every octant: steep, shallow, axis-aligned and exact 45-degree segments out of a hub and back, 32 segments whose length passes 1
    star = []
    for di, dj in STAR:
        star += [at(shape, ci + 3, cj - 5), at(shape, ci + 3 + di, cj - 5 + dj)]
    star.append(at(shape, ci + 3, cj - 5))
    octants = [robot(at(shape, ci, cj), math.pi / 6), robot(star[0], 0.0, intention=star, history=star[:9], target=star[-1])]
    # two robots whose paths cross; a waypoint repeated mid-path and at the end; an end far outside the room (clipped to the border)
    a = [at(shape, ci - 25, cj - 40), at(shape, ci - 5, cj - 10, 0.2, 0.7), at(shape, ci - 5, cj - 10, 0.6, 0.1), at(shape, ci + 22, cj + 31),
         at(shape, ci + 22, cj + 31, 0.9, 0.9)]
    b = [at(shape, ci + 30, cj - 35), at(shape, ci + 2, cj + 3), (5.0, 0.1, 0.0)]
    c = [at(shape, ci + 10, cj + 20), (0.3, 5.0, 0.0), (-5.0, 5.0, 0.0)]
    crossing = [robot(a[0], 0.3, intention=a, history=a[::-1][:4], target=a[-1]), robot(at(shape, ci + 4, cj - 6), -2.0),
                robot(b[0], 1.0, intention=b, history=[b[1], b[1], b[0]], target=b[-1]), robot(at(shape, ci, cj + 30), 0.0, idle=True),
                robot(c[0], 2.0, intention=c, history=c[:2], target=c[-1])]
    idle = [robot(at(shape, ci, cj), math.pi / 2), robot(at(shape, ci + 9, cj + 9), 0.0, idle=True), robot(at(shape, ci - 9, cj), 1.0, idle=True)]
    # spatial channels: targets near the mapper's robot, one on the map border, one robot idle
    spatial = [robot(at(shape, ci + 12, cj + 2), 0.0, target=at(shape, ci - 8, cj + 6)), robot(at(shape, ci - 2, cj - 3), -math.pi / 4),
               robot(at(shape, ci - 20, cj + 20), 0.0, idle=True, target=at(shape, ci, cj)),
               robot(at(shape, ci + 3, cj + 4), 0.0, target=at(shape, ci + 5, cj - 9)), robot(at(shape, ci - 30, cj - 30), 0.0, target=(9.0, -9.0, 0.0))]
    return {'octants': (octants, 0), 'crossing': (crossing, 1), 'idle': (idle, 0), 'spatial': (spatial, 1)}


# (environment, encoding, scale, line thickness)
CASES = [('octants', 'ramp', 1.0, 2), ('octants', 'ramp', 0.25, 1), ('octants', 'binary', 0.5, 3), ('octants', 'history', 1.0, 2),
         ('octants', 'line', 1.0, 2), ('crossing', 'ramp', 1.0, 1), ('crossing', 'ramp', 2.0, 3), ('crossing', 'binary', 1.0, 2),
         ('crossing', 'line', 0.75, 1), ('crossing', 'history', 1.0, 3), ('crossing', 'circle', 1.0, 2), ('crossing', 'circle', 0.5, 1),
         ('idle', 'ramp', 1.0, 2), ('idle', 'circle', 1.0, 3), ('spatial', 'circle', 1.0, 2)]
SPATIAL = [('spatial', 1.0, 2), ('spatial', 0.5, 3), ('spatial', 1.0, 1)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    envs = import_reference(os.path.abspath(args.reference))
    Mapper = envs.Mapper
    ref_seconds, ref_maps, total = 0.0, 0, 0

    for fname, room_width, room_length in (('intention_maps_184x232.npz', 0.5, 1.0), ('intention_maps_232x232.npz', 1.0, 1.0)):
        shape = Mapper.create_padded_room_zeros(room_width, room_length).shape
        world = environments(shape)
        prob = {k: [] for k in ('encoding', 'scale', 'thickness', 'idle', 'spatial', 'position', 'heading', 'tag')}
        robot_prob, way_robot, way_xyz = [], [], []
        seg = {k: [] for k in ('prob', 'px', 'mode', 'drop_last', 'value', 'start', 'stop', 'step')}
        maps, local = [], []

        def mapper(name, scale, thickness):
            robots, own = world[name]
            m = object.__new__(Mapper)
            m.env = types.SimpleNamespace(robots=robots, room_width=room_width, room_length=room_length, intention_map_scale=scale,
                                          intention_map_line_thickness=thickness, intention_channel_encoding='spatial')
            m.robot = robots[own]
            m.intention_map_selem = envs.disk(thickness - 1)                      # envs.py:2044
            return m, robots, own

        def record(name, encoding, scale, thickness, drawn, n_idle, spatial, m, want_map, want_local):
            """One problem: `drawn` is what simq.intention_maps takes for it."""
            p = len(maps)
            got = oracle.global_map(drawn, shape, encoding, scale, thickness)
            assert got.dtype == want_map.dtype == np.float32 and got.shape == want_map.shape == shape
            assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want_map).view(np.int32)), (fname, name, encoding, scale, thickness)
            for k, v in zip(('encoding', 'scale', 'thickness', 'idle', 'spatial', 'position', 'heading', 'tag'),
                            (oracle.ENCODINGS.index(encoding), scale, thickness, n_idle, spatial, m.robot.get_position()[:2], m.robot.get_heading(), name)):
                prob[k].append(v)
            for path in drawn:
                r = len(robot_prob)
                robot_prob.append(p)
                for w in ([path] if encoding == 'circle' else path):
                    way_robot.append(r)
                    way_xyz.append((w[0], w[1], 0.0))
            for s in oracle.segments(drawn, shape, encoding, scale):
                for k, v in zip(('prob', 'px', 'mode', 'drop_last', 'value', 'start', 'stop', 'step'), (p, s[:4], s[4], s[5], s[6], s[7], s[8], s[9])):
                    seg[k].append(v)
            maps.append(want_map)
            local.append(np.ascontiguousarray(want_local, np.float32))

        for name, encoding, scale, thickness in CASES:
            m, robots, own = mapper(name, scale, thickness)
            t0 = time.perf_counter()
            want = m._create_global_intention_or_history_map(encoding)
            ref_seconds += time.perf_counter() - t0
            ref_maps += 1
            others = [r for k, r in enumerate(robots) if k != own]
            key = 'target' if encoding == 'circle' else 'history' if encoding == 'history' else 'intention'
            drawn = [r.paths[key] for r in others if not r.is_idle()]
            record(name, encoding, scale, thickness, drawn, sum(r.is_idle() for r in others), False, m, want, m._get_local_map(want))

        for name, scale, thickness in SPATIAL:
            m, robots, own = mapper(name, scale, thickness)
            seen = []
            m._get_local_map = lambda gm, m=m: (seen.append(np.array(gm, copy=True)), Mapper._get_local_map(m, gm))[1]
            channels = m._get_intention_channels()
            here = m.robot.get_position()
            order = [k for k in np.argsort([envs.distance(here, r.get_position()) for r in robots]) if k != own]      # envs.py:2350-2358
            assert len(channels) == len(seen) == len(order) == len(robots) - 1
            for k, gm, lm in zip(order, seen, channels):
                r = robots[k]
                record(name, 'circle', scale, thickness, [] if r.is_idle() else [r.paths['target']], int(r.is_idle()), True, m, gm, lm)

        arrays = {'maps': np.stack(maps), 'local': np.stack(local), 'robot_prob': np.asarray(robot_prob, np.int32),
                  'way_robot': np.asarray(way_robot, np.int32), 'way_xyz': np.asarray(way_xyz, np.float64).reshape(-1, 3)}
        for k, v in prob.items():
            arrays['prob_' + k] = np.asarray(v) if k == 'tag' else np.asarray(v, {'scale': np.float64, 'position': np.float64, 'heading': np.float64,
                                                                                   'spatial': np.bool_}.get(k, np.int32))
        for k, v in seg.items():
            arrays['seg_' + k] = np.asarray(v, {'value': np.float32, 'start': np.float64, 'stop': np.float64, 'step': np.float64}.get(k, np.int32))
        arrays['seg_px'] = arrays['seg_px'].reshape(-1, 4)
        path = os.path.join(args.out, fname)
        np.savez_compressed(path, **arrays)
        total += len(maps)
        print('%s: %d maps, %d segments, %d bytes' % (path, len(maps), len(seg['prob']), os.path.getsize(path)))
        assert os.path.getsize(path) < 1 << 20
    print('%d maps; reference Mapper on the host: %.3f ms per global map (scipy %s grey_dilation standing in for scikit-image, one CPU thread)'
          % (total, 1e3 * ref_seconds / ref_maps, __import__('scipy').__version__))


if __name__ == '__main__':
    main()
