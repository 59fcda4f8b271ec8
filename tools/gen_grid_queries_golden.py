"""Write tests/golden/grid_queries.npz: shortest-path distances computed by the reference's own OccupancyMap.shortest_path_distance.

    python tools/gen_grid_queries_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout, Cython and scipy.  shortest_paths.pyx is compiled into a temporary directory outside this tree, as
gen_grid_waypoints_golden.py does (nothing compiled is kept), and envs.py is imported as it is with the stand-in modules of
gen_occupancy_maps_golden.py; its GridGraph is then the compiled one.  Per map of tests/golden/occupancy_maps_*.npz (both room
shapes) a real OccupancyMap of the fixture's robot class is updated with a synthetic point cloud that lands on the fixture's occupied
pixels -- so update() itself derives the configuration space and the closest cells, which must equal the fixture's, and builds the
GridGraph -- and its own shortest_path_distance(source_position, target_position) is called for 2 sources x 20 targets: positions
drawn over the room and a margin around it (so some fall on blocked cells and are snapped, some outside the image and are clipped),
the source itself, and cells of components the source cannot reach where the map has any.  tests/grid_queries_oracle.py must equal
every result bit for bit before anything is written.  The file holds positions, pixels and float64 results only.
"""
import argparse
import os
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import grid_queries_oracle as oracle                                                # noqa: E402
import grid_paths_oracle                                                            # noqa: E402
from gen_grid_waypoints_golden import build_reference                               # noqa: E402
from gen_occupancy_maps_golden import OBSTACLE_SEG, ROBOT_CLASSES, cloud, import_reference   # noqa: E402

SOURCES, TARGETS = 2, 20
ROOMS = (('184x232', 0.5, 1.0), ('232x232', 1.0, 1.0))                              # fixture, room_width, room_length


def pixel_centre(i, j, shape):
    """A position inside pixel (i, j), a quarter pixel off its centre."""
    return ((j + 0.75) - shape[1] / 2) / 96.0, (shape[0] / 2 - (i + 0.25)) / 96.0


def draw_positions(cspace, closest, rng):
    """[SOURCES, 2] source positions and [SOURCES, TARGETS, 2] target positions for one map."""
    R, C = cspace.shape
    free = np.argwhere(cspace != 0)
    i0, j0, i1, j1 = free[:, 0].min(), free[:, 1].min(), free[:, 0].max(), free[:, 1].max()
    lo_x, hi_x = (j0 - 12 - C / 2) / 96.0, (j1 + 13 - C / 2) / 96.0
    lo_y, hi_y = (R / 2 - i1 - 13) / 96.0, (R / 2 - i0 + 12) / 96.0
    sources, targets = [], []
    for s in range(SOURCES):
        # the first source on a free cell (a receptacle in a corner of the room), the second anywhere over the room and its margin
        src = pixel_centre(*free[rng.randint(len(free))], (R, C)) if s == 0 else (rng.uniform(lo_x, hi_x), rng.uniform(lo_y, hi_y))
        pts = [(rng.uniform(lo_x, hi_x), rng.uniform(lo_y, hi_y)) for _ in range(TARGETS - 4)]
        pts.append(src)
        pts.append((-(C / 2 + 5) / 96.0, (R / 2 + 5) / 96.0))                       # outside the image: clipped to pixel (0, 0)
        pts.append(((C / 2 + 5) / 96.0, rng.uniform(lo_y, hi_y)))                   # clipped to the last column
        # a free cell the source cannot reach, when there is one; else one more free cell
        image = grid_paths_oracle.distance_image(cspace, oracle.snap(closest, oracle.position_to_pixel_indices(src[0], src[1], (R, C))))
        cut = np.argwhere((cspace != 0) & (image < 0))
        pool = cut if len(cut) else free
        pts.append(pixel_centre(*pool[rng.randint(len(pool))], (R, C)))
        sources.append(src)
        targets.append(pts)
    return np.asarray(sources, np.float64), np.asarray(targets, np.float64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    tmp = tempfile.mkdtemp(prefix='grid_queries_ref_')
    try:
        GridGraph, _ = build_reference(ref, tmp)
        envs = import_reference(ref)
        envs.GridGraph = GridGraph                                                  # what OccupancyMap.update constructs (envs.py:2459)
        arrays, unreachable, snapped, total = {}, 0, 0, 0
        for room, room_width, room_length in ROOMS:
            z = np.load(os.path.join(args.out, 'occupancy_maps_%s.npz' % room))
            rng = np.random.RandomState(29)
            rec = {k: [] for k in ('source_positions', 'target_positions', 'source_pixels', 'target_pixels', 'distances')}
            for k, name in enumerate(z['names']):
                cls = next(c for c in ROBOT_CLASSES if c in str(name))
                m = envs.OccupancyMap(types.SimpleNamespace(RADIUS=getattr(envs, cls).RADIUS, id=k), room_length, room_width)
                points, seg = cloud(m.occupancy_map.shape, [tuple(int(x) for x in px) for px in np.argwhere(z['occupancy'][k])], rng)
                m.update(points, seg, OBSTACLE_SEG)
                cspace, closest = m.configuration_space, m.closest_cspace_indices
                assert np.array_equal(cspace, z['configuration_space'][k]) and np.array_equal(closest, z['closest'][k]), (room, name)
                assert type(m.grid_graph) is GridGraph
                sources, targets = draw_positions(cspace, closest, rng)
                src_px = np.asarray([oracle.position_to_pixel_indices(x, y, cspace.shape) for x, y in sources], np.int16)
                tgt_px = np.asarray([[oracle.position_to_pixel_indices(x, y, cspace.shape) for x, y in ts] for ts in targets], np.int16)
                dist = np.zeros((SOURCES, TARGETS), np.float64)
                cache = {}
                for s in range(SOURCES):
                    for t in range(TARGETS):
                        got = m.shortest_path_distance(tuple(sources[s]), tuple(targets[s, t]))
                        assert isinstance(got, float)
                        want = oracle.shortest_path_distance(cspace, closest, sources[s], targets[s, t], cache)
                        assert np.float64(got).view(np.int64) == np.float64(want).view(np.int64), (room, name, s, t, got, want)
                        dist[s, t] = got
                        unreachable += got < 0
                        snapped += cspace[tuple(tgt_px[s, t])] == 0
                        total += 1
                for key, v in zip(rec, (sources, targets, src_px, tgt_px, dist)):
                    rec[key].append(v)
            for key, v in rec.items():
                arrays['%s_%s' % (key, room)] = np.stack(v)
        assert unreachable >= 8 and snapped >= total // 8, (unreachable, snapped, total)
        path = os.path.join(args.out, 'grid_queries.npz')
        np.savez_compressed(path, **arrays)
        print('%s: %d queries (%d unreachable, %d on blocked cells), %d bytes' % (path, total, unreachable, snapped, os.path.getsize(path)))
        assert os.path.getsize(path) < 27937                                        # under the smallest waypoint fixture
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
