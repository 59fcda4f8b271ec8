"""CPU: the grid-path oracle against the reference's own distances (tests/golden/grid_paths_*.npz, written by
tools/gen_grid_paths_golden.py from shortest_paths.pyx), the C-ABI entry point simq_grid_distance_images and its argument checks
(no kernel is launched here), and simq.GridGraph's input contract."""
import ctypes
import glob
import os

import numpy as np
import pytest

from grid_paths_oracle import distance_image, mapper_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_cases(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'grid_paths_*.npz')))
    assert len(files) == 3, files
    for path in files:
        z = np.load(path)
        for name in z['names']:
            yield str(name), z['grid_' + name], z['src_' + name], z['dist_' + name]


def test_fixtures_cover_the_issue_grid_kinds(golden_dir):
    cases = {name: (g, s, d) for name, g, s, d in fixture_cases(golden_dir)}
    assert {'room_small', 'room_large', 'divider', 'clutter_small', 'clutter_large', 'maze_rows', 'maze_cols', 'sealed_pocket',
            'blocked_source', 'isolated_source', 'one_free', 'one_blocked', 'row_300', 'col_300', 'values_7_255'} <= set(cases)
    for name, (g, s, d) in cases.items():
        assert g.dtype == np.uint8 and d.dtype == np.float32 and d.shape == (len(s),) + g.shape, name
        for (i, j), img in zip(s, d):
            assert img[i, j] == 0, name                                    # the source holds 0, blocked or not
    assert (cases['sealed_pocket'][2] == -1).any() and (cases['sealed_pocket'][2] > 0).any()
    assert (cases['blocked_source'][2][0] == -1).sum() == cases['blocked_source'][0].size - 1
    assert (cases['one_blocked'][2] == 0).all() and (cases['one_free'][2] == 0).all()
    assert set(np.unique(cases['values_7_255'][0])) == {0, 7, 255}


def test_oracle_equals_the_reference_bit_for_bit(golden_dir):
    n = 0
    for name, grid, srcs, dists in fixture_cases(golden_dir):
        for s, want in zip(srcs, dists):
            got = distance_image(grid, tuple(s))
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, tuple(s))
            n += 1
    assert n >= 25


def test_mapper_epilogue_of_the_oracle():
    d = np.array([[0, 1, -1], [np.float32(np.sqrt(2)), 2, -1]], np.float32)
    img = mapper_image(d, 96.0, 0.25)
    assert img.dtype == np.float32
    assert img[0, 2] == img[1, 2] == np.float32(np.float32(2) / np.float32(96)) * np.float32(0.25)


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_export_is_declared_bound_and_laid_out(L):
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    assert 'int simq_grid_distance_images(' in text and 'simq_grid_distance_images' in L.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), 'simq_grid_distance_images')
    from simq.grid_paths import GridProblem
    assert ctypes.sizeof(GridProblem) == 32
    assert [(f, getattr(GridProblem, f).offset) for f, _ in GridProblem._fields_] == [
        ('grid_offset', 0), ('out_offset', 8), ('rows', 16), ('cols', 20), ('src_i', 24), ('src_j', 28)]


def test_c_abi_rejects_bad_arguments_before_any_device_call(L):
    """Every check of simq_grid_distance_images runs on the host before the descriptor copy / launch (the fake device pointers below
    are never dereferenced)."""
    from simq.grid_paths import GridProblem
    c = L.lib.c
    fake = ctypes.c_void_p(4096)

    def call(probs, n=None, grids_bytes=1 << 20, out_floats=1 << 20, ppm=1.0, scale=1.0, null_out=False):
        arr = (GridProblem * len(probs))(*probs)
        return c.simq_grid_distance_images(fake, grids_bytes, arr, len(probs) if n is None else n, fake, None if null_out else fake,
                                           out_floats, ppm, 0, scale, fake, None)

    ok = GridProblem(0, 0, 10, 12, 3, 4)
    assert call([ok], null_out=True) == -1 and 'NULL' in L.last_error()
    assert call([ok], n=0) == -1 and 'n = 0' in L.last_error()
    assert call([GridProblem(0, 0, 10, 12, 10, 4)]) == -1 and 'source (10, 4) outside' in L.last_error()
    assert call([GridProblem(0, 0, 10, 12, 3, -1)]) == -1 and 'outside' in L.last_error()
    assert call([GridProblem(0, 0, 2048, 2048, 0, 0)]) == -1 and '2^22' in L.last_error()
    assert call([GridProblem(0, 0, 0, 5, 0, 0)]) == -1 and 'rows, cols >= 1' in L.last_error()
    assert call([ok], grids_bytes=119) == -1 and 'd_grids' in L.last_error()
    assert call([GridProblem(-1, 0, 10, 12, 3, 4)]) == -1 and 'd_grids' in L.last_error()
    assert call([ok], out_floats=100) == -1 and 'd_out' in L.last_error()
    assert call([ok, GridProblem(0, 119, 10, 12, 3, 4)]) == -1 and 'overlap' in L.last_error()
    assert call([ok], ppm=0.0) == -1 and 'pixels_per_meter' in L.last_error()
    assert call([ok], ppm=float('nan')) == -1 and 'pixels_per_meter' in L.last_error()
    assert call([ok], scale=float('inf')) == -1 and 'scale' in L.last_error()


def test_grid_graph_rejects_bad_grids_before_touching_a_device(L):
    import torch
    import simq
    good = np.ones((4, 5), np.uint8)
    for bad in (good.astype(np.float32), good.astype(np.int8), good.astype(bool), np.ones((4, 10), np.uint8)[:, ::2],
                np.asfortranarray(np.ones((4, 5), np.uint8)), np.ones((2, 4, 5), np.uint8), np.ones(5, np.uint8), good.tolist(),
                torch.ones(4, 5, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            simq.GridGraph(bad)
    g = simq.GridGraph(good)
    with pytest.raises(NotImplementedError, match='order'):
        g.shortest_path((0, 0), (3, 4))
    with pytest.raises(ValueError):
        simq.grid_distance_images([good.astype(np.int16)], [(0, 0)])
    with pytest.raises(ValueError):
        simq.grid_distance_images([good, good], [(0, 0)])


def test_without_a_gpu_the_distance_images_raise(L, monkeypatch):
    import torch
    import simq
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.GridGraph(np.ones((4, 5), np.uint8)).shortest_path_image((0, 0))
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.grid_distance_images([np.ones((4, 5), np.uint8)], [(0, 0)])
