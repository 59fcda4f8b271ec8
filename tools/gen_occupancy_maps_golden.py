"""Write tests/golden/occupancy_maps_*.npz: configuration spaces and closest free cells computed by the reference's own OccupancyMap.

    python tools/gen_occupancy_maps_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and scipy.  envs.py is imported as it is, with empty stand-in modules for what it imports but this code
never touches (pybullet, anki_vector, vector_utils, skimage.draw).  scikit-image, a third-party package the reference imports, is
replaced by stand-ins of the two names OccupancyMap uses: skimage.morphology.binary_dilation(image, selem) is
scipy.ndimage.binary_dilation(image, structure=selem) -- the call scikit-image's own function makes -- and
skimage.morphology.selem.disk is the x^2 + y^2 <= r^2 footprint.  shortest_paths.shortest_paths.GridGraph, which update() constructs
from the new configuration space, is a stand-in that takes the grid and keeps nothing.  Nothing of the reference is copied or kept.
The maps come from real OccupancyMap objects, one per robot class (its RADIUS) and room size, whose own update(points, seg,
obstacle_seg_value) is called with synthetic point clouds (this file's obstacle pixels turned into positions).  Every result is
asserted equal, element for element, to tests/occupancy_maps_oracle.py before anything is written.  Also prints the reference's host
time per update (one CPU thread).
"""
import argparse
import os
import sys
import time
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import occupancy_maps_oracle as oracle                              # noqa: E402

OBSTACLE_SEG, OTHER_SEG = 0.5, 0.25
ROBOT_CLASSES = ('PushingRobot', 'LiftingRobot', 'ThrowingRobot', 'RescueRobot')


def import_reference(ref):
    from scipy import ndimage

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def absent(*args, **kwargs):
        raise NotImplementedError('not part of the occupancy-map path')

    for name in ('anki_vector', 'pybullet', 'pybullet_utils', 'pybullet_utils.bullet_client', 'skimage', 'vector_utils', 'shortest_paths'):
        stub(name)
    stub('skimage.draw', line=absent)
    stub('skimage.morphology', binary_dilation=lambda image, selem: ndimage.binary_dilation(image, structure=selem), dilation=absent)
    stub('skimage.morphology.selem', disk=oracle.disk)
    stub('shortest_paths.shortest_paths', GridGraph=lambda grid: None)
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        import envs
    return envs


def cloud(shape, pixels, rng):
    """A camera frame (points [h, w, 3], seg [h, w]) whose obstacle points fall, one or more each, into `pixels` of a map of `shape`;
    a few non-obstacle points lie among them."""
    pixels = np.asarray(sorted(set(pixels)), np.int64).reshape(-1, 2)
    pixels = np.concatenate([pixels, pixels[:max(1, len(pixels) // 7)]])                       # some pixels hit twice
    frac = rng.uniform(0.1, 0.9, (len(pixels), 2))
    x = (pixels[:, 1] + frac[:, 1] - shape[1] / 2) / 96.0
    y = (shape[0] / 2 - pixels[:, 0] - frac[:, 0]) / 96.0
    seg = np.full(len(pixels), OBSTACLE_SEG)
    n_free = 40
    x = np.concatenate([x, rng.uniform(-0.2, 0.2, n_free)])
    y = np.concatenate([y, rng.uniform(-0.2, 0.2, n_free)])
    seg = np.concatenate([seg, np.full(n_free, OTHER_SEG)])
    pad = (-len(x)) % 8
    x, y, seg = (np.concatenate([a, np.full(pad, v)]) for a, v in ((x, 0.0), (y, 0.0), (seg, OTHER_SEG)))
    points = np.stack([x, y, np.full(len(x), 0.02)], axis=1).reshape(-1, 8, 3)
    return points, seg.reshape(-1, 8)


def box(i, j, h, w):
    return [(a, b) for a in range(i, i + h) for b in range(j, j + w)]


def scenarios(room_mask, radius, rng):
    """name -> list of obstacle-pixel lists, one per successive update() call."""
    R, C = room_mask.shape
    ii, jj = np.nonzero(room_mask)
    i0, i1, j0, j1 = ii.min(), ii.max() + 1, jj.min(), jj.max() + 1                            # the room: [i0, i1) x [j0, j1)
    walls = [(i, j) for i in range(i0 - 3, i1 + 3) for j in range(j0 - 3, j1 + 3) if not room_mask[i, j]]
    ci, cj = (i0 + i1) // 2, (j0 + j1) // 2

    def clutter(n):
        px = list(walls)
        for _ in range(n):
            px += box(int(rng.randint(i0, i1 - 4)), int(rng.randint(j0, j1 - 4)), int(rng.randint(1, 5)), int(rng.randint(1, 5)))
        return px

    out = {'walls_only': [walls]}
    for k in range(6):
        out['clutter_%d' % k] = [clutter(3 + 3 * k)]
    out['touching_wall'] = [walls + box(i0, cj - 6, 5, 9) + box(ci - 2, j1 - 4, 6, 4)]
    out['border_corner'] = [walls + [(0, 0), (0, 1), (1, 0), (R - 1, C - 1), (0, C // 2), (R - 1, 3), (R // 2, 0), (ci, C - 1)] +
                            box(ci + 3, cj - 10, 3, 3)]
    # an obstacle just outside the room mask (no walls seen yet): it narrows the configuration space, the thin space ignores it
    out['outside_room'] = [box(i0 - 2, cj, 2, 3) + box(ci, j0 - 1, 4, 1) + box(ci - 8, cj + 12, 2, 2)]
    # everything further than the radius from one cell: that cell is the whole configuration space
    I, J = np.mgrid[0:R, 0:C]
    far = (I - (ci + 5)) ** 2 + (J - (cj - 7)) ** 2 > radius * radius
    out['one_free'] = [list(zip(I[far].tolist(), J[far].tolist()))]
    out['successive'] = [walls[::2] + box(ci - 9, cj - 20, 4, 4), walls[1::2] + box(ci + 4, cj + 15, 3, 6) + box(ci - 9, cj - 18, 2, 8)]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    envs = import_reference(os.path.abspath(args.reference))
    ref_seconds, ref_updates, total = 0.0, 0, 0
    radii_seen = {}

    for fname, room_width, room_length in (('occupancy_maps_184x232.npz', 0.5, 1.0), ('occupancy_maps_232x232.npz', 1.0, 1.0)):
        rng = np.random.RandomState(7)
        rec = {k: [] for k in ('names', 'occupancy', 'room_mask', 'radius', 'thin_radius', 'configuration_space', 'cspace_thin', 'closest')}
        probe = envs.OccupancyMap(types.SimpleNamespace(RADIUS=getattr(envs, ROBOT_CLASSES[0]).RADIUS, id=0), room_length, room_width)
        names = list(scenarios(probe.room_mask, 5, rng))
        for k, name in enumerate(names):
            cls = ROBOT_CLASSES[k % len(ROBOT_CLASSES)]
            robot = types.SimpleNamespace(RADIUS=getattr(envs, cls).RADIUS, id=k)
            m = envs.OccupancyMap(robot, room_length, room_width)
            radius, thin_radius = m.selem.shape[0] // 2, m.selem_thin.shape[0] // 2
            assert np.array_equal(m.selem, oracle.disk(radius)) and np.array_equal(m.selem_thin, oracle.disk(thin_radius))
            radii_seen[cls] = radius
            for step, pixels in enumerate(scenarios(m.room_mask, radius, rng)[name]):
                points, seg = cloud(m.occupancy_map.shape, pixels, rng)
                t0 = time.perf_counter()
                m.update(points, seg, OBSTACLE_SEG)
                ref_seconds += time.perf_counter() - t0
                ref_updates += 1
                want = np.zeros(m.occupancy_map.shape, np.uint8)
                if step == 0:
                    seen = set()
                seen |= set(pixels)
                want[tuple(np.asarray(sorted(seen)).T)] = 1
                assert np.array_equal(m.occupancy_map, want), (fname, name, step)            # the cloud landed where it was aimed
                closest = m.closest_cspace_indices
                assert m.configuration_space.dtype == m.cspace_thin.dtype == np.uint8 and closest.dtype == np.int32
                assert m.configuration_space.any(), (fname, name)                              # (an empty one has no defined result)
                cs, thin, near = oracle.update(m.occupancy_map, m.room_mask, radius, thin_radius)
                assert np.array_equal(cs, m.configuration_space), (fname, name, step)
                assert np.array_equal(thin, m.cspace_thin), (fname, name, step)
                assert near.dtype == closest.dtype and np.array_equal(near, closest), (fname, name, step)
                if name == 'one_free':
                    assert int(cs.sum()) == 1
                for key, v in zip(rec, ('%s_%s%s' % (name, cls, '_step%d' % step if name == 'successive' else ''), m.occupancy_map.copy(),
                                        m.room_mask.copy(), radius, thin_radius, m.configuration_space.copy(), m.cspace_thin.copy(),
                                        closest.copy())):
                    rec[key].append(v)
        arrays = {k: np.asarray(v) if k == 'names' else np.stack(v).astype(np.int32 if k in ('radius', 'thin_radius', 'closest') else np.uint8)
                  for k, v in rec.items()}
        path = os.path.join(args.out, fname)
        np.savez_compressed(path, **arrays)
        total += len(rec['names'])
        print('%s: %d maps, %d bytes' % (path, len(rec['names']), os.path.getsize(path)))
        assert os.path.getsize(path) < 881687
    assert total >= 24 and len(set(radii_seen.values())) >= 2, radii_seen
    print('%d maps; radii %s; reference OccupancyMap.update on the host: %.3f ms per update (scipy %s, binary_dilation standing in for '
          'scikit-image, one CPU thread, %d updates)' % (total, radii_seen, 1e3 * ref_seconds / ref_updates, __import__('scipy').__version__,
                                                         ref_updates))


if __name__ == '__main__':
    main()
