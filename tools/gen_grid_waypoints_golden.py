"""Write tests/golden/grid_waypoints_*.npz: parents, dense paths and waypoints computed by the reference's own GridGraph.

    python tools/gen_grid_waypoints_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and Cython.  shortest_paths.pyx is compiled into a temporary directory outside this tree, as
gen_grid_paths_golden.py does; nothing compiled is kept.  Its two skimage imports are served by stand-ins: `line` is the closed form
tests/intention_maps_oracle.py pins to the published algorithm; `approximate_polygon` records its `coords` argument -- the dense
path built from the reference's own parents -- and applies one of two documented stand-in simplifiers, the identity or "keep the
first point, every third, the last" (tests/grid_waypoints_oracle.py).  Grids and sources are those of tests/golden/grid_paths_*.npz.
Per (grid, source) the file holds the reference's whole parent image as direction codes (one shortest_path call per free target,
cache hits after the first), some 40 dense paths and the reference's final shortest_path output under both simplifiers.  The numpy
oracle must equal all of it before anything is written.  Also prints the reference's time for the first call from each source
(GridGraph._spfa plus one walk).
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import grid_waypoints_oracle as oracle                                  # noqa: E402
from intention_maps_oracle import line_points                           # noqa: E402

TARGETS = 40
STUB = {
    'skimage/__init__.py': '',
    'skimage/draw.py': 'IMPL = [None]\ndef line(r0, c0, r1, c1):\n    return IMPL[0](int(r0), int(c0), int(r1), int(c1))\n',
    'skimage/measure.py': 'RECORD = []\nSIMPLIFY = [None]\ndef approximate_polygon(coords, tolerance):\n    RECORD.append(coords.copy())\n'
                          '    return SIMPLIFY[0](coords, tolerance)\n',
}


def build_reference(ref, tmp):
    shutil.copy(os.path.join(ref, 'shortest_paths', 'shortest_paths.pyx'), tmp)
    for name, text in STUB.items():
        os.makedirs(os.path.join(tmp, os.path.dirname(name)), exist_ok=True)
        with open(os.path.join(tmp, name), 'w') as f:
            f.write(text)
    subprocess.run([sys.executable, '-m', 'Cython.Build.Cythonize', '-3', '-i', 'shortest_paths.pyx'], cwd=tmp, check=True,
                   stdout=subprocess.DEVNULL)
    sys.path.insert(0, tmp)
    import shortest_paths
    import skimage.draw
    import skimage.measure
    skimage.draw.IMPL[0] = line_points
    return shortest_paths.GridGraph, skimage.measure


def direction_codes(parents):
    """uint8 [rows, cols]: the direction k of shortest_paths.pyx:30 with cell = parent + dirs[k], 255 where the cell has no parent."""
    rows, cols = parents.shape
    codes = np.full((rows, cols), 255, np.uint8)
    ii, jj = np.nonzero(parents >= 0)
    pi, pj = parents[ii, jj] // cols, parents[ii, jj] % cols
    for k, (di, dj) in enumerate(oracle.DIRS):
        sel = (ii - pi == di) & (jj - pj == dj)
        codes[ii[sel], jj[sel]] = k
    assert (codes[ii, jj] != 255).all()
    return codes


def pick_targets(grid, source, dist, rng):
    """Some 40 targets: reachable free cells, a few blocked or unreachable ones, the source itself."""
    reach = np.argwhere(dist > 0)
    other = np.argwhere(dist < 0)
    picks = [tuple(int(x) for x in source)]
    if reach.size:
        picks += [tuple(int(x) for x in reach[k]) for k in rng.choice(len(reach), min(TARGETS - 5, len(reach)), replace=False)]
    if other.size:
        picks += [tuple(int(x) for x in other[k]) for k in rng.choice(len(other), min(4, len(other)), replace=False)]
    return picks


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix='grid_waypoints_ref_')
    rng = np.random.RandomState(13)
    try:
        GridGraph, measure = build_reference(os.path.abspath(args.reference), tmp)
        for kind in ('rooms', 'clutter', 'edges'):
            z = np.load(os.path.join(args.out, 'grid_paths_%s.npz' % kind))
            arrays, names = {}, []
            for name in z['names']:
                name = str(name)
                grid = np.ascontiguousarray(z['grid_' + name], np.uint8)
                for si, source in enumerate(z['src_' + name]):
                    source = tuple(int(x) for x in source)
                    key = '%s_%d' % (name, si)
                    dist = z['dist_' + name][si]
                    gg = GridGraph(grid)
                    measure.SIMPLIFY[0] = oracle.identity
                    del measure.RECORD[:]
                    t0 = time.perf_counter()
                    gg.shortest_path(source, source)
                    dt = time.perf_counter() - t0
                    # the whole parent image: the second point of the dense path from every free target
                    parents = np.full(grid.shape, -1, np.int32)
                    for ti, tj in np.argwhere(grid != 0):
                        del measure.RECORD[:]
                        gg.shortest_path(source, (int(ti), int(tj)))
                        dense = measure.RECORD[0]
                        if len(dense) > 1:
                            parents[ti, tj] = dense[1][0] * grid.shape[1] + dense[1][1]
                    o_dist, o_parents, count = oracle.spfa(grid, source)
                    assert np.array_equal(o_parents, parents), key
                    assert np.array_equal(o_dist.view(np.int32), dist.view(np.int32)), key
                    targets = pick_targets(grid, source, dist, rng)
                    dense_all, way = [], {'identity': [], 'every_third': []}
                    for t in targets:
                        for label, fn in (('identity', oracle.identity), ('every_third', oracle.every_third)):
                            measure.SIMPLIFY[0] = fn
                            del measure.RECORD[:]
                            got = np.asarray(gg.shortest_path(source, t), np.int32).reshape(-1, 2)
                            dense = np.asarray(measure.RECORD[0], np.int32)
                            assert np.array_equal(dense, oracle.dense_path(o_parents, source, t)), (key, t)
                            assert np.array_equal(got, np.asarray(oracle.prune(grid, dense, fn), np.int32).reshape(-1, 2)), (key, t, label)
                            way[label].append(got)
                        dense_all.append(dense)
                    arrays['parents_' + key] = direction_codes(parents)
                    arrays['targets_' + key] = np.asarray(targets, np.int16)
                    arrays['dense_' + key] = np.concatenate(dense_all).astype(np.int16)
                    arrays['dense_len_' + key] = np.asarray([len(d) for d in dense_all], np.int32)
                    for label in way:
                        arrays['way_%s_%s' % (label, key)] = np.concatenate(way[label]).astype(np.int16)
                        arrays['way_%s_len_%s' % (label, key)] = np.asarray([len(w) for w in way[label]], np.int32)
                    names.append(key)
                    print('%-20s %4d x %-4d src %-12s %8.3f ms first call (reference SPFA + walk)  pops %d pushes %d swaps %d'
                          % (key, grid.shape[0], grid.shape[1], source, 1e3 * dt, count['pops'], count['pushes'], count['swaps']))
            arrays['names'] = np.asarray(names)
            path = os.path.join(args.out, 'grid_waypoints_%s.npz' % kind)
            np.savez_compressed(path, **arrays)
            print('%s: %d bytes' % (path, os.path.getsize(path)))
            assert os.path.getsize(path) < 150000
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
