"""Write tests/golden/grid_paths_*.npz: distance images computed by the reference's own GridGraph (shortest_paths.pyx).

    python tools/gen_grid_paths_golden.py --reference PATH/TO/spatial-intention-maps

Needs the reference checkout and Cython.  shortest_paths.pyx is compiled into a temporary directory outside this tree (its two
skimage imports serve only GridGraph.shortest_path, so a stub module stands in for them); nothing compiled is kept.  Every case is
a synthetic grid of this file plus sources; each output file stays well under 1 MB.  Also prints the reference's time per image.
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
PPM = 96                                   # Mapper.LOCAL_MAP_PIXELS_PER_METER (envs.py:2010-2012)
SKIMAGE_STUB = {
    'skimage/__init__.py': '',
    'skimage/draw.py': 'def line(*args):\n    raise NotImplementedError\n',
    'skimage/measure.py': 'def approximate_polygon(*args, **kwargs):\n    raise NotImplementedError\n',
}


def build_reference(ref, tmp):
    src = os.path.join(ref, 'shortest_paths', 'shortest_paths.pyx')
    shutil.copy(src, tmp)
    for name, text in SKIMAGE_STUB.items():
        os.makedirs(os.path.join(tmp, os.path.dirname(name)), exist_ok=True)
        with open(os.path.join(tmp, name), 'w') as f:
            f.write(text)
    subprocess.run([sys.executable, '-m', 'Cython.Build.Cythonize', '-3', '-i', 'shortest_paths.pyx'], cwd=tmp, check=True,
                   stdout=subprocess.DEVNULL)
    sys.path.insert(0, tmp)
    import shortest_paths
    return shortest_paths.GridGraph


# ---- synthetic grids (1 = free) ------------------------------------------------------------------------------------------------
def padded_room(rows, cols, room_rows, room_cols):
    """A Mapper-style configuration space: everything blocked but a centred room (OccupancyMap._create_room_mask)."""
    g = np.zeros((rows, cols), np.uint8)
    i0, j0 = rows // 2 - room_rows // 2, cols // 2 - room_cols // 2
    g[i0:i0 + room_rows, j0:j0 + room_cols] = 1
    return g


def dilate(mask, r):
    out = mask.copy()
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            if di * di + dj * dj <= r * r:
                out |= np.roll(np.roll(mask, di, 0), dj, 1)
    return out


def cluttered(rows, cols, room_rows, room_cols, boxes, seed):
    """A room with square boxes dilated by a robot radius of 5 pixels, as the configuration space of envs.py:2453-2455."""
    rng = np.random.RandomState(seed)
    g = padded_room(rows, cols, room_rows, room_cols)
    occ = np.zeros_like(g, bool)
    ii, jj = np.nonzero(g)
    for _ in range(boxes):
        k = rng.randint(ii.size)
        occ[ii[k]:ii[k] + 4, jj[k]:jj[k] + 4] = True
    g[dilate(occ, 5)] = 0
    return g


def serpentine(rows, cols, pitch, vertical=False):
    """Walls every `pitch` lines with the gap alternating ends: hop counts of rows * cols / pitch."""
    g = np.ones((cols, rows) if vertical else (rows, cols), np.uint8)
    for k, i in enumerate(range(pitch - 1, g.shape[0] - 1, pitch)):
        g[i, :] = 0
        g[i, -2:] = 1 if k % 2 == 0 else 0
        if k % 2:
            g[i, :2] = 1
    return np.ascontiguousarray(g.T) if vertical else g


def first_free(g, near):
    ii, jj = np.nonzero(g)
    k = np.argmin((ii - near[0]) ** 2 + (jj - near[1]) ** 2)
    return int(ii[k]), int(jj[k])


def cases():
    """name -> (grid, [sources]) grouped per output file."""
    rooms, clutter, edges = {}, {}, {}
    small = padded_room(184, 232, 44, 92)                       # 0.5 x 1 m room (envs.py:2383-2403, 2440)
    large = padded_room(232, 232, 92, 92)                       # 1 x 1 m room
    rooms['room_small'] = (small, [first_free(small, (92, 116)), first_free(small, (0, 0))])
    rooms['room_large'] = (large, [first_free(large, (116, 116)), first_free(large, (231, 231))])
    div = padded_room(232, 232, 92, 92)
    div[70:162, 115:117] = 0
    div[150:156, 115:117] = 1                                   # the gap
    rooms['divider'] = (div, [first_free(div, (80, 80)), first_free(div, (80, 150))])
    clutter['clutter_small'] = (cluttered(184, 232, 44, 92, 6, 1),)
    clutter['clutter_large'] = (cluttered(232, 232, 92, 92, 14, 2),)
    for k in list(clutter):
        g = clutter[k][0]
        clutter[k] = (g, [first_free(g, (g.shape[0] // 2, g.shape[1] // 2)), first_free(g, (0, g.shape[1] - 1))])
    open_big = np.ones((232, 232), np.uint8)
    clutter['open_232'] = (open_big, [(0, 0), (115, 200)])
    maze = serpentine(64, 96, 4)
    edges['maze_rows'] = (maze, [(0, 0)])
    mazev = serpentine(64, 96, 4, vertical=True)
    edges['maze_cols'] = (mazev, [(0, 0)])
    pocket = padded_room(96, 128, 60, 100)
    pocket[30:50, 40:70] = 0
    pocket[33:47, 43:67] = 1                                    # free cells sealed inside the wall ring
    edges['sealed_pocket'] = (pocket, [first_free(pocket, (20, 20)), (40, 55)])
    blk = padded_room(64, 80, 40, 50)
    edges['blocked_source'] = (blk, [(0, 0), (32, 40)])
    iso = padded_room(64, 80, 40, 50)
    iso[30:35, 30:35] = 0
    iso[32, 32] = 1
    edges['isolated_source'] = (iso, [(32, 32)])
    edges['one_free'] = (np.ones((1, 1), np.uint8), [(0, 0)])
    edges['one_blocked'] = (np.zeros((1, 1), np.uint8), [(0, 0)])
    edges['row_300'] = (np.ones((1, 300), np.uint8), [(0, 0), (0, 170)])
    edges['col_300'] = (np.ones((300, 1), np.uint8), [(299, 0)])
    rng = np.random.RandomState(7)
    vals = rng.choice(np.array([0, 7, 255], np.uint8), size=(70, 90), p=[0.3, 0.35, 0.35])
    edges['values_7_255'] = (vals, [first_free(vals, (35, 45))])
    wide = (rng.rand(40, 600) > 0.25).astype(np.uint8)         # wider than one 256-column block of the kernel
    edges['wide_600'] = (wide, [first_free(wide, (20, 10)), first_free(wide, (20, 590))])
    return {'grid_paths_rooms.npz': rooms, 'grid_paths_clutter.npz': clutter, 'grid_paths_edges.npz': edges}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of jimmyyhwu/spatial-intention-maps')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix='grid_paths_ref_')
    try:
        GridGraph = build_reference(os.path.abspath(args.reference), tmp)
        for fname, group in cases().items():
            arrays, names = {}, []
            for name, (grid, srcs) in group.items():
                grid = np.ascontiguousarray(grid, np.uint8)
                imgs = []
                for s in srcs:
                    gg = GridGraph(grid)
                    t0 = time.perf_counter()
                    img = np.array(gg.shortest_path_image(tuple(s)), np.float32)
                    dt = time.perf_counter() - t0
                    imgs.append(img)
                    print('%-16s %4d x %-4d src %-12s %8.3f ms  (reference GridGraph + SPFA, one CPU thread)'
                          % (name, grid.shape[0], grid.shape[1], tuple(s), 1e3 * dt))
                arrays['grid_' + name] = grid
                arrays['src_' + name] = np.asarray(srcs, np.int32).reshape(-1, 2)
                arrays['dist_' + name] = np.stack(imgs)
                names.append(name)
            arrays['names'] = np.asarray(names)
            path = os.path.join(args.out, fname)
            np.savez_compressed(path, **arrays)
            print('%s: %d bytes' % (path, os.path.getsize(path)))
            assert os.path.getsize(path) < 1 << 20
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
