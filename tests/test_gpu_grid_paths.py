"""GPU: simq_grid_distance_images / simq.GridGraph against the reference's own distances (tests/golden/grid_paths_*.npz) and the
numpy fixed-point oracle (tests/grid_paths_oracle.py), bit for bit (compared as int32 bit patterns)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from grid_paths_oracle import distance_image, mapper_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def fixture_cases(golden_dir):
    for path in sorted(glob.glob(os.path.join(golden_dir, 'grid_paths_*.npz'))):
        z = np.load(path)
        for name in z['names']:
            yield str(name), z['grid_' + name], z['src_' + name], z['dist_' + name]


def random_grid(rng, rows, cols, p_blocked):
    return (rng.rand(rows, cols) >= p_blocked).astype(np.uint8)


def test_every_fixture_bit_for_bit(simq_mod, golden_dir):
    n = 0
    for name, grid, srcs, dists in fixture_cases(golden_dir):
        got = simq_mod.grid_distance_images([grid], [tuple(s) for s in srcs], grid_index=[0] * len(srcs))
        assert tuple(got.shape) == dists.shape and got.dtype == torch.float32
        assert np.array_equal(bits(got), bits(dists)), name
        g = simq_mod.GridGraph(grid)
        for s, want in zip(srcs, dists):
            assert np.array_equal(bits(g.shortest_path_image(tuple(s))), bits(want)), (name, tuple(s))
        n += len(srcs)
    assert n >= 25


def test_random_grids_against_the_oracle(simq_mod):
    rng = np.random.RandomState(11)
    grids, srcs = [], []
    for k in range(40):
        rows, cols = int(rng.randint(1, 90)), int(rng.randint(1, 300))
        grids.append(random_grid(rng, rows, cols, rng.choice([0.0, 0.1, 0.25, 0.45])))
        srcs.append((int(rng.randint(rows)), int(rng.randint(cols))))          # blocked sources included
    got = simq_mod.grid_distance_images(grids, srcs)
    assert isinstance(got, list) and len(got) == 40
    for g, s, img in zip(grids, srcs, got):
        assert tuple(img.shape) == g.shape
        assert np.array_equal(bits(img), bits(distance_image(g, s))), (g.shape, s)


def test_mixed_shape_batch_equals_per_problem_calls(simq_mod):
    rng = np.random.RandomState(5)
    shapes = [(184, 232), (232, 232), (60, 90), (1, 300), (300, 1), (40, 600)]
    grids = [random_grid(rng, r, c, 0.2) for r, c in shapes]
    idx = [int(rng.randint(len(grids))) for _ in range(64)]
    srcs = [(int(rng.randint(grids[k].shape[0])), int(rng.randint(grids[k].shape[1]))) for k in idx]
    # device-resident grids are taken as they are; numpy ones are uploaded
    dev_grids = [torch.from_numpy(g).cuda() if k % 2 else g for k, g in enumerate(grids)]
    batch = simq_mod.grid_distance_images(dev_grids, srcs, grid_index=idx)
    assert len(batch) == 64
    for k, s, img in zip(idx, srcs, batch):
        one = simq_mod.grid_distance_images([grids[k]], [s])
        assert tuple(one.shape) == (1,) + grids[k].shape
        assert np.array_equal(bits(img), bits(one[0])), (grids[k].shape, s)
    for k, s, img in list(zip(idx, srcs, batch))[:6]:
        assert np.array_equal(bits(img), bits(distance_image(grids[k], s)))


def test_batch_of_1024_problems(simq_mod):
    rng = np.random.RandomState(3)
    grids = np.stack([random_grid(rng, 48, 64, p) for p in np.linspace(0.0, 0.4, 16)])
    idx = [k % 16 for k in range(1024)]
    srcs = [(int(rng.randint(48)), int(rng.randint(64))) for _ in range(1024)]
    out = torch.full((1024, 48, 64), 123.0, device='cuda')
    got = simq_mod.grid_distance_images(torch.from_numpy(grids).cuda(), srcs, grid_index=idx, out=out)
    assert got is out
    host = bits(out)
    for p in range(1024):
        assert np.array_equal(host[p], bits(distance_image(grids[idx[p]], srcs[p]))), p


def test_cache_snapshot_and_one_launch_for_uncached_sources(simq_mod, golden_dir):
    from simq import _lib
    z = np.load(os.path.join(golden_dir, 'grid_paths_rooms.npz'))
    grid, srcs, want = z['grid_room_small'].copy(), [tuple(s) for s in z['src_room_small']], z['dist_room_small']
    g = simq_mod.GridGraph(grid)
    grid[:] = 0                                        # the graph snapshotted the grid at construction
    _lib.lib.c.simq_launch_counts_reset()
    imgs = g.shortest_path_images(srcs + srcs[:1])
    assert _lib.lib.c.simq_launch_count(b'grid_distance') == 1
    for img, w in zip(imgs, list(want) + [want[0]]):
        assert np.array_equal(bits(img), bits(w))
    again = g.shortest_path_image(srcs[1])
    assert again is imgs[1] and _lib.lib.c.simq_launch_count(b'grid_distance') == 1        # cached: no launch
    # numpy integers as pixel indices hit the same cache entry
    assert g.shortest_path_image((np.int64(srcs[0][0]), np.int32(srcs[0][1]))) is imgs[0]
    assert _lib.lib.c.simq_launch_count(b'grid_distance') == 1


def test_shortest_path_distance_is_the_image_value(simq_mod, golden_dir):
    z = np.load(os.path.join(golden_dir, 'grid_paths_edges.npz'))
    grid, src, want = z['grid_sealed_pocket'], tuple(z['src_sealed_pocket'][0]), z['dist_sealed_pocket'][0]
    g = simq_mod.GridGraph(grid)
    rng = np.random.RandomState(0)
    for _ in range(50):
        t = (int(rng.randint(grid.shape[0])), int(rng.randint(grid.shape[1])))
        v = g.shortest_path_distance(src, t)
        assert type(v) is float and v == float(want[t])
    assert g.shortest_path_distance(src, (40, 55)) == -1.0                   # inside the sealed pocket
    assert g.shortest_path_distance(src, src) == 0.0


def test_mapper_epilogue_matches_numpy(simq_mod, golden_dir):
    """Mapper._create_global_shortest_path_map after OccupancyMap.shortest_path_image (envs.py:2294-2299, 2513-2516) on the fixtures:
    (d / 96.0), then < 0 -> max, then * 0.25; and the division alone."""
    for name, grid, srcs, dists in fixture_cases(golden_dir):
        s = [tuple(x) for x in srcs]
        got = simq_mod.grid_distance_images([grid], s, grid_index=[0] * len(s), pixels_per_meter=96.0, unreachable_to_max=True,
                                            scale=0.25)
        want = np.stack([mapper_image(d, 96.0, 0.25) for d in dists])
        assert np.array_equal(bits(got), bits(want)), name
        got = simq_mod.grid_distance_images([grid], s, grid_index=[0] * len(s), pixels_per_meter=96.0)
        assert np.array_equal(bits(got), bits(dists / np.float32(96.0))), name


def test_out_of_range_sources_raise_instead_of_faulting(simq_mod):
    from simq import _lib
    grid = np.ones((10, 12), np.uint8)
    for bad in ((10, 0), (0, 12), (-1, 3), (3, -1), (1 << 20, 0)):
        with pytest.raises(_lib.SimqError, match='outside'):
            simq_mod.grid_distance_images([grid], [bad])
        with pytest.raises(_lib.SimqError, match='outside'):
            simq_mod.GridGraph(grid).shortest_path_image(bad)
    with pytest.raises(_lib.SimqError, match='outside'):
        simq_mod.GridGraph(grid).shortest_path_distance((0, 0), (10, 0))
    with pytest.raises(_lib.SimqError, match='2\\^22'):
        simq_mod.grid_distance_images([torch.ones(2048, 2048, dtype=torch.uint8, device='cuda')], [(0, 0)])
    # the library is still usable afterwards
    assert float(simq_mod.grid_distance_images([grid], [(0, 0)])[0, 9, 11]) == float(distance_image(grid, (0, 0))[9, 11])
