"""CPU: the occupancy-map oracle (tests/occupancy_maps_oracle.py) against the reference OccupancyMap's own results
(tests/golden/occupancy_maps_*.npz, written by tools/gen_occupancy_maps_golden.py) element for element; its dilation against
scipy.ndimage.binary_dilation and its closest free cells against scipy.ndimage.distance_transform_edt(return_indices=True) on fresh
random grids; the C-ABI entry point simq_occupancy_maps, its descriptor layout and its argument checks (no kernel is launched here);
the Python input contract."""
import ctypes
import glob
import os

import numpy as np
import pytest

import occupancy_maps_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DIM, MAX_RADIUS = 256, 16


def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'occupancy_maps_*.npz')))
    assert len(files) == 2, files
    return [(os.path.basename(f), oracle.load_fixture(f)) for f in files]


def test_fixtures_cover_the_issue_cases(golden_dir):
    shapes, n, radii = set(), 0, set()
    for fname, cases in fixtures(golden_dir):
        assert os.path.getsize(os.path.join(golden_dir, fname)) < 881687
        find = lambda prefix: [c for c in cases if c['name'].startswith(prefix)]
        assert find('walls_only') and len(find('clutter')) >= 3 and find('touching_wall')
        for c in cases:
            occ, mask, cs, thin, near = c['occupancy'], c['room_mask'], c['configuration_space'], c['cspace_thin'], c['closest']
            shapes.add(occ.shape)
            radii.add(c['radius'])
            assert occ.dtype == mask.dtype == cs.dtype == thin.dtype == np.uint8 and near.dtype == np.int32
            assert mask.shape == cs.shape == thin.shape == occ.shape and near.shape == (2,) + occ.shape
            assert cs.any()                                                        # no empty configuration space: undefined in the reference
            assert set(np.unique(cs)) <= {0, 1} and set(np.unique(thin)) <= {0, 1} and not (cs & (1 - mask)).any()
            n += 1
        R, C = cases[0]['occupancy'].shape
        (border,) = find('border_corner')
        o = border['occupancy']
        assert o[0, 0] and o[R - 1, C - 1] and o[0, C // 2] and o[R // 2, 0]       # the dilation is clipped at the border and in the corners
        (outside,) = find('outside_room')
        o, m = outside['occupancy'], outside['room_mask']
        assert (o & (1 - m)).any() and (o & m).any()
        only_inside = oracle.configuration_space(o & m, m, outside['radius'])
        assert (only_inside != outside['configuration_space']).any()               # ... it counts for the configuration space
        assert np.array_equal(oracle.cspace_thin(o & m, m, outside['thin_radius']), outside['cspace_thin'])       # ... not for the thin one
        (one,) = find('one_free')
        assert int(one['configuration_space'].sum()) == 1
        i, j = [int(x[0]) for x in np.nonzero(one['configuration_space'])]
        assert (one['closest'][0] == i).all() and (one['closest'][1] == j).all()
        s0, s1 = find('successive')
        assert s0['name'].endswith('step0') and s1['name'].endswith('step1')
        assert (s1['occupancy'] >= s0['occupancy']).all() and (s1['occupancy'] != s0['occupancy']).any()           # the map accumulates
        touching = find('touching_wall')[0]
        ii, jj = np.nonzero(touching['room_mask'])
        assert touching['occupancy'][ii.min(), jj.min():jj.max()].any() and touching['occupancy'][ii.min() - 1, jj.min():jj.max()].all()
    assert shapes == {(184, 232), (232, 232)} and n >= 24 and len(radii) >= 2


def test_oracle_equals_the_reference_element_for_element(golden_dir):
    n = 0
    for fname, cases in fixtures(golden_dir):
        for c in cases:
            cs, thin, near = oracle.update(c['occupancy'], c['room_mask'], c['radius'], c['thin_radius'])
            assert cs.dtype == np.uint8 and np.array_equal(cs, c['configuration_space']), (fname, c['name'])
            assert thin.dtype == np.uint8 and np.array_equal(thin, c['cspace_thin']), (fname, c['name'])
            assert near.dtype == np.int32 and np.array_equal(near, c['closest']), (fname, c['name'])
            n += 1
    assert n >= 24


def test_dilation_equals_scipy_binary_dilation():
    from scipy import ndimage
    rng = np.random.RandomState(21)
    n = 0
    for k in range(340):
        radius = k % (MAX_RADIUS + 1)
        rows, cols = [(184, 232), (232, 232), (int(rng.randint(1, 40)), int(rng.randint(1, 300 if k % 3 else 40))), (MAX_DIM, MAX_DIM),
                      (1, int(rng.randint(1, MAX_DIM + 1))), (int(rng.randint(1, MAX_DIM + 1)), 1)][k % 6]
        cols = min(cols, MAX_DIM)
        density = [None, 0.001, 0.01, 0.1, 0.5, 0.9, 0.995][k % 7]
        if density is None:
            image = np.zeros((rows, cols), np.uint8)                                # a single occupied pixel, often on the border
            image[[0, rows - 1, int(rng.randint(rows))][k % 3], [int(rng.randint(cols)), 0, cols - 1][k // 3 % 3]] = 1
        else:
            image = (rng.rand(rows, cols) < density).astype(np.uint8) * rng.choice([1, 7, 255])
        want = ndimage.binary_dilation(image, structure=oracle.disk(radius))
        assert np.array_equal(oracle.dilate(image, radius), want), (k, rows, cols, radius, density)
        n += 1
    assert n >= 300


def random_free_grid(rng, k):
    """A grid with at least one free cell (1 = free): sizes from 1 x 1 to the cap, all free, one free cell, sparse, dense, and
    room-shaped ones whose padded band is full of ties."""
    kind = k % 8
    if kind == 7:                                                                   # a room with blocked boxes inside a blocked band
        rows, cols = [(184, 232), (232, 232), (MAX_DIM, MAX_DIM), (96, 130)][k // 8 % 4]
        g = np.zeros((rows, cols), np.uint8)
        h, w = rows // 4, cols // 5
        g[rows // 2 - h:rows // 2 + h, cols // 2 - w:cols // 2 + w] = 1
        for _ in range(k % 5):
            i, j = int(rng.randint(rows // 2 - h, rows // 2 + h)), int(rng.randint(cols // 2 - w, cols // 2 + w))
            g[i:i + int(rng.randint(1, 12)), j:j + int(rng.randint(1, 12))] = 0
        g[rows // 2 - h, cols // 2 - w] = 1
        return g
    if k % 50 == 0:
        rows, cols = 1, 1
    elif k % 11 == 0:
        rows, cols = MAX_DIM, int(rng.randint(1, MAX_DIM + 1))
    elif k % 13 == 0:
        rows, cols = int(rng.randint(1, MAX_DIM + 1)), MAX_DIM
    elif k % 17 == 0:
        rows, cols = [(1, int(rng.randint(1, MAX_DIM + 1))), (int(rng.randint(1, MAX_DIM + 1)), 1)][k % 2]
    else:
        rows, cols = int(rng.randint(1, 70)), int(rng.randint(1, 70))
    if kind == 0:
        return np.ones((rows, cols), np.uint8)
    if kind == 1:
        g = np.zeros((rows, cols), np.uint8)
        g[int(rng.randint(rows)), int(rng.randint(cols))] = 1
        return g
    g = (rng.rand(rows, cols) < [0.5, 0.1, 0.02, 0.9, 0.3][kind - 2]).astype(np.uint8)
    if kind == 6:                                                                   # small integer lattices: many equal distances
        g = np.zeros((rows, cols), np.uint8)
        g[::int(rng.randint(2, 7)), ::int(rng.randint(2, 7))] = 1
    if not g.any():
        g[int(rng.randint(rows)), int(rng.randint(cols))] = 1
    return g


def test_closest_free_cells_equal_scipy_feature_transform():
    from scipy import ndimage
    rng = np.random.RandomState(22)
    n, capped = 0, 0
    for k in range(1040):
        g = random_free_grid(rng, k)
        assert g.any()
        want = ndimage.distance_transform_edt(1 - g, return_distances=False, return_indices=True)
        got = oracle.closest_free(g)
        assert got.dtype == want.dtype == np.int32 and np.array_equal(got, want), (k, g.shape)
        capped += MAX_DIM in g.shape
        n += 1
    assert n >= 1000 and capped >= 50


def test_empty_configuration_space_gives_minus_one():
    got = oracle.closest_free(np.zeros((5, 7), np.uint8))
    assert got.shape == (2, 5, 7) and (got == -1).all()


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_export_is_declared_bound_and_laid_out(L):
    import re
    import subprocess
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    assert 'int simq_occupancy_maps(' in text and 'simq_occupancy_maps' in L.EXPORTS and hasattr(ctypes.CDLL(L.LIB_PATH), 'simq_occupancy_maps')
    assert 'global: simq_*; local: *;' in open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'libsimq.map')).read()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert ' T simq_occupancy_maps' in out
    assert 'occupancy_maps.hip' in open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'Makefile')).read()
    from simq import occupancy as om
    # the header's struct: three int64 and four int32, in this order
    body = re.search(r'typedef struct simq_occupancy_problem \{(.*?)\} simq_occupancy_problem;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r'(int64_t|int32_t)\s+([^;]+);', body):
        fields += [(name.strip(), 8 if ctype == 'int64_t' else 4) for name in names.split(',')]
    assert [f for f, _ in fields] == [f for f, _ in om.OccupancyProblem._fields_]
    assert [s for _, s in fields] == [ctypes.sizeof(t) for _, t in om.OccupancyProblem._fields_]
    assert ctypes.sizeof(om.OccupancyProblem) == sum(s for _, s in fields) == 40
    assert [(f, getattr(om.OccupancyProblem, f).offset) for f, _ in om.OccupancyProblem._fields_] == [
        ('occupancy_offset', 0), ('mask_offset', 8), ('out_offset', 16), ('rows', 24), ('cols', 28), ('radius', 32), ('thin_radius', 36)]
    assert '#define SIMQ_OCCUPANCY_MAX_DIM %d' % om.MAX_DIM in text and '#define SIMQ_OCCUPANCY_MAX_RADIUS %d' % om.MAX_RADIUS in text
    assert om.MAX_DIM >= 256 and om.MAX_RADIUS >= 16 and (om.MAX_DIM, om.MAX_RADIUS) == (MAX_DIM, MAX_RADIUS)
    import simq
    assert simq.occupancy_maps is om.occupancy_maps and simq.configuration_space is om.configuration_space
    assert simq.occupancy_maps is om.occupancy_maps                                # (importing the submodule shadows no exported function)


MAPS, PROBS, CSPACE, THIN, CLOSEST, STATUS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000


def c_call(L, probs=None, n=None, maps=MAPS, maps_bytes=1 << 20, d_probs=PROBS, cspace=CSPACE, thin=THIN, cspace_bytes=1 << 20, closest=CLOSEST,
           closest_ints=1 << 21, status=STATUS):
    """simq_occupancy_maps on fake device pointers: every check runs on the host before the descriptor copy / launch."""
    from simq.occupancy import OccupancyProblem
    probs = [OccupancyProblem(0, 184 * 232, 0, 184, 232, 6, 3)] if probs is None else probs
    arr = (OccupancyProblem * max(len(probs), 1))(*probs)
    vp = lambda a: None if a is None else ctypes.c_void_p(a)
    return L.lib.c.simq_occupancy_maps(vp(maps), maps_bytes, arr, len(probs) if n is None else n, vp(d_probs), vp(cspace), vp(thin), cspace_bytes,
                                       vp(closest), closest_ints, vp(status), None)


def test_c_abi_rejects_bad_descriptors_before_any_device_call(L):
    from simq.occupancy import OccupancyProblem as P

    def refused(word, **kw):
        assert c_call(L, **kw) == -1, kw
        assert word in L.last_error(), (word, L.last_error())

    cells = 184 * 232
    prob = lambda **kw: P(**dict(dict(occupancy_offset=0, mask_offset=cells, out_offset=0, rows=184, cols=232, radius=6, thin_radius=3), **kw))
    for name in ('maps', 'd_probs', 'cspace', 'thin', 'closest', 'status'):
        refused('NULL', **{name: None})
    refused('n = 0', n=0)
    refused('n = -1', n=-1)
    # sizes and radii
    for kw in (dict(rows=0), dict(cols=0), dict(rows=-4), dict(rows=257), dict(cols=257), dict(rows=1 << 20)):
        refused('rows, cols in 1 .. 256', probs=[prob(**kw)])
    refused('radius = -1', probs=[prob(radius=-1)])
    refused('radius = 17', probs=[prob(radius=17)])
    refused('thin_radius = -1', probs=[prob(thin_radius=-1)])
    refused('thin_radius = 17', probs=[prob(thin_radius=17)])
    # inputs inside d_maps
    refused('occupancy bytes', probs=[prob(occupancy_offset=-1)])
    refused('occupancy bytes', maps_bytes=2 * cells, probs=[prob(occupancy_offset=cells + 1)])
    refused('room mask bytes', probs=[prob(mask_offset=-8)])
    refused('room mask bytes', maps_bytes=2 * cells - 1)
    refused('of d_maps', maps_bytes=cells - 1)
    # outputs inside their buffers
    refused('output bytes', probs=[prob(out_offset=-1)])
    refused('output bytes', cspace_bytes=cells - 1)
    refused('output bytes', cspace_bytes=2 * cells - 1, probs=[prob(), prob(out_offset=cells)])
    refused('closest ints', closest_ints=2 * cells - 1)
    refused('closest ints', cspace_bytes=2 * cells, closest_ints=4 * cells - 1, probs=[prob(), prob(out_offset=cells)])
    refused('problem 1', closest_ints=4 * cells - 1, probs=[prob(), prob(out_offset=cells)])
    # no two problems' outputs overlap (sharing inputs is fine)
    refused('outputs overlap', probs=[prob(), prob()])
    refused('outputs overlap', probs=[prob(), prob(out_offset=cells - 1)])
    refused('outputs overlap', probs=[prob(out_offset=cells), prob(rows=10, cols=10, out_offset=2 * cells), prob(rows=10, cols=10, out_offset=2 * cells - 50)])
    # outputs disjoint from the inputs, from d_problems and from each other
    refused('d_cspace overlaps d_maps', cspace=MAPS + 64)
    refused('d_thin overlaps d_maps', thin=MAPS + (1 << 20) - 1)
    refused('d_closest overlaps d_maps', closest=MAPS - 4 * (1 << 21) + 4)
    refused('d_cspace overlaps d_problems', cspace=PROBS + 8)
    refused('d_thin overlaps d_problems', thin=PROBS - (1 << 20) + 8)
    refused('d_closest overlaps d_problems', closest=PROBS + 36)
    refused('d_cspace overlaps d_thin', thin=CSPACE)
    refused('d_cspace overlaps d_closest', closest=CSPACE + (1 << 20) - 4)
    refused('d_thin overlaps d_closest', closest=THIN + 4)
    refused('overlaps', status=CSPACE + 16)
    refused('overlaps', status=MAPS + 16)
    refused('aligned', d_probs=PROBS + 4)
    refused('aligned', closest=CLOSEST + 2)
    refused('aligned', status=STATUS + 1)


def test_the_case_that_just_fits_is_not_refused(L):
    """Maps at the cap with the largest radii, two problems sharing one mask, buffers of exactly the needed size laid end to end:
    every check but the one corrupted last passes (the call is refused only by it, so nothing touches the fake pointers)."""
    from simq.occupancy import OccupancyProblem as P
    c = MAX_DIM * MAX_DIM
    probs = [P(0, 2 * c, c, MAX_DIM, MAX_DIM, MAX_RADIUS, MAX_RADIUS), P(c, 2 * c, 0, MAX_DIM, MAX_DIM, 0, 0), P(3 * c - 1, 3 * c - 1, 2 * c, 1, 1, 0, 16)]
    kw = dict(maps_bytes=3 * c, cspace_bytes=2 * c + 1, closest_ints=4 * c + 2, cspace=CSPACE, thin=CSPACE + 2 * c + 1, closest=CSPACE + 4 * c + 4,
              d_probs=PROBS, status=PROBS + 4 * 40)
    assert c_call(L, **dict(kw, probs=probs + [P(0, 0, 2 * c + 1, 1, 1, 0, 0)])) == -1
    assert 'problem 3: output bytes [%d, %d) outside the %d' % (2 * c + 1, 2 * c + 2, 2 * c + 1) in L.last_error()
    assert c_call(L, **dict(kw, probs=probs[:2] + [P(3 * c - 1, 3 * c, 2 * c, 1, 1, 0, 16)])) == -1
    assert 'problem 2: room mask bytes' in L.last_error()
    assert c_call(L, **dict(kw, probs=probs, status=PROBS + 3 * 40 - 4)) == -1 and 'd_status overlaps d_problems' in L.last_error()


def test_python_rejects_bad_input_before_touching_a_device(L, monkeypatch):
    import torch
    import simq
    from simq import occupancy as om
    occ, mask = np.zeros((6, 9), np.uint8), np.ones((6, 9), np.uint8)
    # without a device nothing runs (and nothing falls back to the host)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.occupancy_maps([occ], [mask], 6, 3)
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.configuration_space(occ, mask, 6, 3)
    # the argument checks come first: they raise ValueError without a device too
    bad_maps = (occ.astype(np.float32), occ.astype(np.int8), occ.astype(bool), np.zeros((6, 18), np.uint8)[:, ::2],
                np.asfortranarray(np.zeros((6, 9), np.uint8)), np.zeros(9, np.uint8), occ.tolist(), torch.zeros(6, 9, dtype=torch.int32),
                torch.zeros(6, 18, dtype=torch.uint8)[:, ::2])
    for bad in bad_maps:
        with pytest.raises(ValueError, match=r'occupancy\[0\] must be a 2-D'):
            simq.occupancy_maps([bad], [mask], 6, 3)
        with pytest.raises(ValueError, match=r'room_masks\[0\] must be a 2-D'):
            simq.occupancy_maps([occ], [bad], 6, 3)
    for kw in (dict(occupancy=[]), dict(room_masks=[]), dict(occupancy=np.zeros((2, 2, 6, 9), np.uint8)), dict(occupancy=occ), dict(occupancy=None),
               dict(room_masks=[mask, mask]), dict(room_masks=[np.ones((6, 8), np.uint8)]), dict(room_index=[1]), dict(room_index=[-1]),
               dict(room_index=[0, 0]), dict(radius=-1), dict(radius=17), dict(radius=2.5), dict(radius=[1, 2]), dict(radius=None), dict(radius=True),
               dict(thin_radius=-1), dict(thin_radius=17), dict(thin_radius='3'), dict(thin_radius=[3, 3])):
        args = dict(dict(occupancy=[occ], room_masks=[mask], radius=6, thin_radius=3), **kw)
        with pytest.raises(ValueError):
            simq.occupancy_maps(**args)
    monkeypatch.setattr(om._batch, 'device', lambda what: torch.device('cpu'))
    good = [torch.zeros(1, 6, 9, dtype=torch.uint8), torch.zeros(1, 6, 9, dtype=torch.uint8), torch.zeros(1, 2, 6, 9, dtype=torch.int32)]
    for k, bad in ((0, torch.zeros(1, 6, 8, dtype=torch.uint8)), (1, torch.zeros(1, 6, 9, dtype=torch.float32)), (2, torch.zeros(1, 6, 9, dtype=torch.int32)),
                   (2, torch.zeros(1, 2, 6, 9, dtype=torch.int64)), (0, torch.zeros(1, 6, 18, dtype=torch.uint8)[:, :, ::2]), (1, np.zeros((1, 6, 9), np.uint8))):
        out = list(good)
        out[k] = bad
        with pytest.raises(ValueError, match='out: ' + om.OccupancyMaps._fields[k]):
            simq.occupancy_maps([occ], [mask], 6, 3, out=out)
    with pytest.raises(ValueError, match='three tensors'):
        simq.occupancy_maps([occ], [mask], 6, 3, out=good[:2])
    # mixed shapes: packed buffers of at least the needed size
    with pytest.raises(ValueError, match='at least 84 elements'):
        simq.occupancy_maps([occ, np.zeros((5, 6), np.uint8)], [mask, np.ones((5, 6), np.uint8)], 6, 3,
                            out=[torch.zeros(84, dtype=torch.uint8), torch.zeros(83, dtype=torch.uint8), torch.zeros(168, dtype=torch.int32)])
