"""GPU: simq_occupancy_maps / simq.occupancy_maps against the reference OccupancyMap's own results
(tests/golden/occupancy_maps_*.npz) and the numpy oracle (tests/occupancy_maps_oracle.py), element for element, and chained into
simq.grid_distance_images."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import occupancy_maps_oracle as oracle
from grid_paths_oracle import distance_image, mapper_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


def host(t):
    return t.detach().cpu().numpy()


def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'occupancy_maps_*.npz')))
    assert len(files) == 2, files
    return [(os.path.basename(f), oracle.load_fixture(f)) for f in files]


def c_abi(problems, maps, garbage=0):
    """simq_occupancy_maps called directly.  problems: (occupancy index, mask index, rows, cols, radius, thin_radius) over the list of
    2-D uint8 arrays `maps`; outputs packed in problem order.  Returns (cspace, thin, closest, status) as flat numpy arrays and the
    output byte offset of every problem."""
    from simq import _lib
    from simq.occupancy import OccupancyProblem
    offs = np.concatenate([[0], np.cumsum([m.size for m in maps])]).astype(np.int64)
    packed = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
    outs, total = [], 0
    for _, _, r, c, _, _ in problems:
        outs.append(total)
        total += r * c
    probs = (OccupancyProblem * len(problems))(*[OccupancyProblem(int(offs[o]), int(offs[m]), outs[p], r, c, rad, thin)
                                                 for p, (o, m, r, c, rad, thin) in enumerate(problems)])
    d_probs = torch.empty(ctypes.sizeof(probs), dtype=torch.uint8, device='cuda')
    cs = torch.full((total,), garbage, dtype=torch.uint8, device='cuda')
    th = torch.full((total,), garbage, dtype=torch.uint8, device='cuda')
    near = torch.full((2 * total,), -12345, dtype=torch.int32, device='cuda')
    status = torch.full((len(problems),), 77, dtype=torch.int32, device='cuda')
    _lib.lib.call('simq_occupancy_maps', _lib.ptr(packed), ctypes.c_int64(packed.numel()), probs, len(problems), _lib.ptr(d_probs), _lib.ptr(cs),
                  _lib.ptr(th), ctypes.c_int64(total), _lib.ptr(near), ctypes.c_int64(2 * total), _lib.ptr(status), _lib.stream_ptr())
    torch.cuda.synchronize()
    return host(cs), host(th), host(near), host(status), outs


def test_every_fixture_through_python_and_the_c_abi(simq_mod, golden_dir):
    n = 0
    for fname, cases in fixtures(golden_dir):
        occ = np.stack([c['occupancy'] for c in cases])
        masks = np.stack([c['room_mask'] for c in cases])
        got = simq_mod.occupancy_maps(occ, masks, [c['radius'] for c in cases], [c['thin_radius'] for c in cases])
        R, C = occ.shape[1:]
        assert got.configuration_space.dtype == got.cspace_thin.dtype == torch.uint8 and got.closest_cspace_indices.dtype == torch.int32
        assert tuple(got.configuration_space.shape) == tuple(got.cspace_thin.shape) == (len(cases), R, C)
        assert tuple(got.closest_cspace_indices.shape) == (len(cases), 2, R, C)
        # the C-ABI directly, every problem sharing the file's one room mask
        assert all(np.array_equal(m, masks[0]) for m in masks)
        maps = list(occ) + [masks[0]]
        cs, th, near, status, outs = c_abi([(k, len(cases), R, C, c['radius'], c['thin_radius']) for k, c in enumerate(cases)], maps, garbage=9)
        assert not status.any()
        for k, c in enumerate(cases):
            tag = (fname, c['name'])
            assert np.array_equal(host(got.configuration_space[k]), c['configuration_space']), tag
            assert np.array_equal(host(got.cspace_thin[k]), c['cspace_thin']), tag
            assert np.array_equal(host(got.closest_cspace_indices[k]), c['closest']), tag
            o = outs[k]
            assert np.array_equal(cs[o:o + R * C].reshape(R, C), c['configuration_space']), tag
            assert np.array_equal(th[o:o + R * C].reshape(R, C), c['cspace_thin']), tag
            assert np.array_equal(near[2 * o:2 * o + 2 * R * C].reshape(2, R, C), c['closest']), tag
            one = simq_mod.configuration_space(c['occupancy'], c['room_mask'], c['radius'], c['thin_radius'])
            assert all(isinstance(a, np.ndarray) for a in one) and one.closest_cspace_indices.dtype == np.int32
            assert np.array_equal(one.configuration_space, c['configuration_space']) and np.array_equal(one.cspace_thin, c['cspace_thin'])
            assert np.array_equal(one.closest_cspace_indices, c['closest']), tag
            n += 1
    assert n >= 24


def random_problem(rng, rows, cols):
    occ = (rng.rand(rows, cols) < rng.choice([0.0, 0.002, 0.02, 0.15, 0.6])).astype(np.uint8) * rng.choice([1, 3, 255])
    kind = rng.randint(3)
    if kind == 0:
        mask = np.ones((rows, cols), np.uint8)
    elif kind == 1:
        mask = np.zeros((rows, cols), np.uint8)
        mask[rows // 5:rows - rows // 5, cols // 6:cols - cols // 6] = 200
    else:
        mask = (rng.rand(rows, cols) < 0.8).astype(np.uint8)
    mask[rows // 2, cols // 2] = 1
    return occ.astype(np.uint8), mask


def test_one_launch_of_mixed_shapes_and_radii_equals_the_oracle(simq_mod):
    rng = np.random.RandomState(31)
    shapes = [(1, 1), (1, 200), (200, 1), (1, 256), (256, 1), (256, 256), (184, 232), (232, 232), (7, 13), (63, 65), (33, 129), (255, 3)]
    shapes += [(int(rng.randint(1, 100)), int(rng.randint(1, 257))) for _ in range(40)]
    masks = [random_problem(rng, r, c)[1] for r, c in shapes]              # one shared mask per shape, used by several problems
    P = 208
    occupancy, room_index, radii, thin = [], [], [], []
    for p in range(P):
        k = p % len(shapes)
        rows, cols = shapes[k]
        occ, _ = random_problem(rng, rows, cols)
        radius = int(rng.randint(0, 17)) if p % 4 else [0, 16, 6, 5][p // 4 % 4]
        # (the reference's result is undefined without a free cell: nothing occupied within the radius of the mask's centre cell)
        occ[max(rows // 2 - radius, 0):rows // 2 + radius + 1, max(cols // 2 - radius, 0):cols // 2 + radius + 1] = 0
        occupancy.append(torch.from_numpy(occ).cuda() if p % 3 == 0 else occ)           # device maps are read with a device copy
        room_index.append(k)
        radii.append(radius)
        thin.append(int(rng.randint(0, 17)) if p % 5 else 3)
    dev_masks = [torch.from_numpy(m).cuda() if k % 2 else m for k, m in enumerate(masks)]
    got = simq_mod.occupancy_maps(occupancy, dev_masks, radii, thin, room_index=room_index)
    assert all(isinstance(x, list) and len(x) == P for x in got)
    for p in range(P):
        tag = (p, shapes[room_index[p]], radii[p], thin[p])
        occ = host(occupancy[p]) if isinstance(occupancy[p], torch.Tensor) else occupancy[p]
        want = oracle.update(occ, masks[room_index[p]], radii[p], thin[p])
        assert want[0].any()
        assert tuple(got.closest_cspace_indices[p].shape) == (2,) + shapes[room_index[p]]
        assert np.array_equal(host(got.configuration_space[p]), want[0]), tag
        assert np.array_equal(host(got.cspace_thin[p]), want[1]), tag
        assert np.array_equal(host(got.closest_cspace_indices[p]), want[2]), tag


def test_batch_of_1024_uniform_problems(simq_mod):
    rng = np.random.RandomState(32)
    rows, cols = 48, 80
    mask = np.zeros((rows, cols), np.uint8)
    mask[6:42, 8:72] = 1
    occ = np.zeros((1024, rows, cols), np.uint8)
    for p in range(1024):
        for _ in range(1 + p % 6):
            i, j = int(rng.randint(rows)), int(rng.randint(cols))
            occ[p, i:i + int(rng.randint(1, 5)), j:j + int(rng.randint(1, 5))] = 1
    radii = [p % 8 for p in range(1024)]
    got = simq_mod.occupancy_maps(torch.from_numpy(occ).cuda(), [mask], radii, 3, room_index=[0] * 1024)
    cs, th, near = (host(t) for t in got)
    assert cs.shape == th.shape == (1024, rows, cols) and near.shape == (1024, 2, rows, cols)
    for p in range(1024):
        want = oracle.update(occ[p], mask, radii[p], 3)
        assert want[0].any()
        assert np.array_equal(cs[p], want[0]) and np.array_equal(th[p], want[1]) and np.array_equal(near[p], want[2]), p


def test_out_tensors_full_of_garbage_are_overwritten(simq_mod, golden_dir):
    cases = fixtures(golden_dir)[0][1][:5]
    R, C = cases[0]['occupancy'].shape
    out = [torch.full((5, R, C), 0xAB, dtype=torch.uint8, device='cuda'), torch.full((5, R, C), 0xCD, dtype=torch.uint8, device='cuda'),
           torch.full((5, 2, R, C), -987654, dtype=torch.int32, device='cuda')]
    got = simq_mod.occupancy_maps([c['occupancy'] for c in cases], [c['room_mask'] for c in cases], [c['radius'] for c in cases], 3, out=out)
    assert got.configuration_space is out[0] and got.cspace_thin is out[1] and got.closest_cspace_indices is out[2]
    for k, c in enumerate(cases):
        assert np.array_equal(host(out[0][k]), c['configuration_space']) and np.array_equal(host(out[1][k]), c['cspace_thin'])
        assert np.array_equal(host(out[2][k]), c['closest'])
    # mixed shapes into packed buffers larger than needed: the problems' elements are written, the tail is left alone
    small = np.zeros((9, 11), np.uint8)
    small[4, 5] = 1
    n = R * C + 99
    out = [torch.full((n + 5,), 0xAB, dtype=torch.uint8, device='cuda'), torch.full((n + 5,), 0xCD, dtype=torch.uint8, device='cuda'),
           torch.full((2 * n + 5,), -987654, dtype=torch.int32, device='cuda')]
    got = simq_mod.occupancy_maps([cases[0]['occupancy'], small], [cases[0]['room_mask'], np.ones((9, 11), np.uint8)], [cases[0]['radius'], 2], 3, out=out)
    want = oracle.update(small, np.ones((9, 11), np.uint8), 2, 3)
    assert np.array_equal(host(got.configuration_space[0]), cases[0]['configuration_space']) and np.array_equal(host(got.closest_cspace_indices[0]), cases[0]['closest'])
    for a, b in zip(got, want):
        assert np.array_equal(host(a[1]), b)
    assert got.configuration_space[1].data_ptr() == out[0].data_ptr() + R * C and got.closest_cspace_indices[1].data_ptr() == out[2].data_ptr() + 8 * R * C
    assert (host(out[0][n:]) == 0xAB).all() and (host(out[1][n:]) == 0xCD).all() and (host(out[2][2 * n:]) == -987654).all()


def test_a_blocked_problem_reports_status_1_and_leaves_its_neighbours_alone(simq_mod):
    from simq import _lib
    rng = np.random.RandomState(33)
    rows, cols = 40, 56
    mask = np.ones((rows, cols), np.uint8)
    occ = [(rng.rand(rows, cols) < 0.01).astype(np.uint8) for _ in range(5)]
    occ[2][::3, ::3] = 1                                       # radius 4 around a 3 x 3 lattice: nothing stays free
    occ[4][:] = 0
    no_room = np.zeros((rows, cols), np.uint8)                 # problem 4: an empty room mask, nothing occupied
    with pytest.raises(_lib.SimqError, match=r'no free cell.*problems \[2, 4\]'):
        simq_mod.occupancy_maps(occ, [mask, no_room], 4, 3, room_index=[0, 0, 0, 0, 1])
    cs, th, near, status, outs = c_abi([(k, 5 if k < 4 else 6, rows, cols, 4, 3) for k in range(5)], occ + [mask, no_room], garbage=5)
    assert status.tolist() == [0, 0, 1, 0, 1]
    n = rows * cols
    for k in range(5):
        want = oracle.update(occ[k], mask if k < 4 else no_room, 4, 3)
        o = outs[k]
        assert np.array_equal(cs[o:o + n].reshape(rows, cols), want[0]) and np.array_equal(th[o:o + n].reshape(rows, cols), want[1]), k
        assert np.array_equal(near[2 * o:2 * o + 2 * n].reshape(2, rows, cols), want[2]), k              # -1 everywhere for problems 2 and 4
    assert (near[2 * outs[2]:2 * outs[2] + 2 * n] == -1).all() and not cs[outs[2]:outs[2] + n].any() and th[outs[4]:outs[4] + n].all()
    # what the library refuses launches nothing and names the problem
    with pytest.raises(_lib.SimqError, match=r'problem 1 is 257 x 4'):
        simq_mod.occupancy_maps([occ[0], np.zeros((257, 4), np.uint8)], [mask, np.ones((257, 4), np.uint8)], 4, 3)
    assert np.array_equal(simq_mod.configuration_space(occ[0], mask, 4, 3).configuration_space, oracle.configuration_space(occ[0], mask, 4))


def test_chain_into_grid_distance_images(simq_mod, golden_dir):
    """occupancy_maps -> the sources looked up in the closest cells on the device (one small readback) -> grid_distance_images on the
    device configuration space with the Mapper epilogue, against the oracle on the reference's own configuration space and closest
    cells."""
    c = next(c for c in fixtures(golden_dir)[0][1] if c['name'].startswith('clutter_2'))
    R, C = c['occupancy'].shape
    got = simq_mod.occupancy_maps([c['occupancy']], [c['room_mask']], c['radius'], c['thin_radius'])
    ii, jj = np.nonzero(c['occupancy'] & c['room_mask'])
    # a robot pixel in free space, a receptacle pixel in the corner of the room (inside the wall's dilation), an occupied pixel, one in the padding
    mi, mj = np.nonzero(c['room_mask'])
    fi, fj = np.nonzero(c['configuration_space'])
    pixels = [(int(fi[len(fi) // 2]), int(fj[len(fi) // 2])), (int(mi.min()), int(mj.max())), (int(ii[0]), int(jj[0])), (3, C - 2)]
    assert not c['configuration_space'][pixels[1]] and not c['configuration_space'][pixels[2]]
    px = torch.tensor(pixels, device='cuda')
    sources = got.closest_cspace_indices[0][:, px[:, 0], px[:, 1]].t().cpu().numpy()           # the 2 * P source pixels: the only readback
    want_sources = [tuple(int(v) for v in c['closest'][:, i, j]) for i, j in pixels]
    assert [tuple(int(v) for v in s) for s in sources] == want_sources
    imgs = simq_mod.grid_distance_images([got.configuration_space[0]], [tuple(int(v) for v in s) for s in sources], grid_index=[0] * len(pixels),
                                         pixels_per_meter=96.0, unreachable_to_max=True, scale=0.25)
    for img, s in zip(imgs, want_sources):
        want = mapper_image(distance_image(c['configuration_space'], s), 96.0, 0.25)
        assert np.array_equal(host(img).view(np.int32), want.view(np.int32)), s
