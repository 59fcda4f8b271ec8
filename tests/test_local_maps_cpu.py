"""CPU: the local-map oracle (tests/local_maps_oracle.py) against the reference Mapper's own images (tests/golden/local_maps_*.npz,
written by tools/gen_local_maps_golden.py) and against scipy.ndimage.rotate on fresh random poses, bit for bit; the C-ABI entry point
simq_local_state_images, its descriptor layout and its argument checks (no kernel is launched here); the Python input contract."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest

import local_maps_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'local_maps_*.npz')))
    assert len(files) == 2, files
    return [(os.path.basename(f), oracle.load_fixture(f)) for f in files]


def test_fixtures_cover_the_issue_cases(golden_dir):
    shapes, headings, images = set(), [], 0
    for name, fx in fixtures(golden_dir):
        rows, cols = fx['maps'].shape[1:]
        shapes.add((rows, cols))
        assert fx['maps'].dtype == fx['want'].dtype == fx['masks'].dtype == np.float32
        assert fx['want'].shape == (len(fx['states']), 96, 96, len(fx['channels']))
        images += fx['want'].shape[0] * fx['want'].shape[3]
        assert {c if isinstance(c, str) else c[0] for c in fx['channels']} == set(oracle.KIND_NAMES)
        assert fx['maps'][0].min() < 0 and fx['maps'][0].max() > 1                       # a map with negative and > 1 values
        pix = np.array([s['pixel'] for s in fx['states']])
        assert 68 in pix[:, 0] and rows - 68 in pix[:, 0] and 68 in pix[:, 1] and cols - 68 in pix[:, 1]      # the legal extremes
        headings += [s['heading'] for s in fx['states']]
        for env in fx['robots'].values():
            assert 1 <= len(env) <= 4
        # a lifting robot drawn with the with-cube mask in the robot map and its own in the overhead map; two robots overlapping
        assert any(r[2] != r[5] for env in fx['robots'].values() for r in env)
        a = fx['robots'][0]
        assert max(abs(a[0][0][0] - a[1][0][0]), abs(a[0][0][1] - a[1][0][1])) < 8
    assert shapes == {(184, 232), (232, 232)} and images >= 40
    for h in (0.0, math.pi / 2, -math.pi / 2, math.pi, math.pi / 4, -math.pi / 4, math.pi / 6):
        assert any(x == h for x in headings), h


def test_oracle_equals_the_reference_bit_for_bit(golden_dir):
    """With the doubles the fixtures store: no scipy involved."""
    n = 0
    for name, fx in fixtures(golden_dir):
        for p, s in enumerate(fx['states']):
            got = oracle.state(fx['maps'], fx['channels'], s['pixel'], s['rot'], fx['robots'][s['env']], fx['masks'])
            assert got.dtype == np.float32
            for c in range(got.shape[2]):
                assert np.array_equal(bits(got[:, :, c]), bits(fx['want'][p, :, :, c])), (name, p, fx['channels'][c])
                n += 1
    assert n >= 40


def test_stored_doubles_are_what_this_machine_computes(golden_dir):
    """The rotation triples of the fixtures against oracle.rotation / simq's own helper here: pixels and shapes equal; R and the
    offsets equal to the last bits that cosdg / sindg and the 2 x 2 product may differ in between machines (2 ulp of the offset's scale)."""
    pytest.importorskip('scipy.special')
    for name, fx in fixtures(golden_dir):
        rows, cols = fx['maps'].shape[1:]
        for s in fx['states']:
            assert oracle.position_to_pixel_indices(s['position'][0], s['position'][1], (rows, cols)) == s['pixel']
            R, off, shape = oracle.crop_rotation(s['heading'])
            assert np.array_equal(shape, s['rot'][2])
            assert np.allclose(R, s['rot'][0], rtol=0, atol=4e-16) and np.allclose(off, s['rot'][1], rtol=0, atol=1e-13)


def scipy_local_map(gm, pixel, heading):
    """The reference's sequence (envs.py:2199-2210) through scipy itself."""
    from scipy.ndimage import rotate
    pi, pj = pixel
    crop = gm[pi - 68:pi + 68, pj - 68:pj + 68]
    r = rotate(crop, 90 - math.degrees(heading), order=0)
    return r[r.shape[0] // 2 - 48:r.shape[0] // 2 + 48, r.shape[1] // 2 - 48:r.shape[1] // 2 + 48]


def scipy_robot_map(shape, robots, masks, seg):
    """envs.py:2250-2275 through scipy itself; robots: (pixel, heading, mask, seg value, map value, seg mask)."""
    from scipy.ndimage import rotate
    out = np.zeros(shape, np.float32)
    for pixel, heading, mask, seg_value, map_value, seg_mask in robots:
        vis = masks[seg_mask if seg else mask].copy()
        vis *= seg_value if seg else map_value
        rot = rotate(vis, math.degrees(heading) - 90, order=0)
        si, sj = pixel[0] - rot.shape[0] // 2, pixel[1] - rot.shape[1] // 2
        out[si:si + rot.shape[0], sj:sj + rot.shape[1]] = np.maximum(out[si:si + rot.shape[0], sj:sj + rot.shape[1]], rot)
    return out


SPECIAL_HEADINGS = [0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, math.pi / 4, -math.pi / 4, 3 * math.pi / 4, -3 * math.pi / 4, math.pi / 6,
                    math.pi / 3, -math.pi / 6]


def test_oracle_equals_scipy_on_fresh_random_poses(golden_dir):
    pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(2024)
    masks = oracle.load_fixture(os.path.join(golden_dir, 'local_maps_184x232.npz'))['masks']
    n = 0
    for k in range(520):
        rows, cols = (184, 232) if k % 2 else (232, 232)
        gm = rng.rand(rows, cols).astype(np.float32) * 4 - 1
        pixel = (int(rng.randint(68, rows - 68 + 1)), int(rng.randint(68, cols - 68 + 1)))
        heading = SPECIAL_HEADINGS[k % len(SPECIAL_HEADINGS)] if k % 5 == 0 else rng.uniform(-math.pi, math.pi)
        rot = oracle.crop_rotation(heading)
        want = scipy_local_map(gm, pixel, heading)
        assert want.shape == (96, 96)
        assert np.array_equal(bits(oracle.local_map(gm, pixel, rot)), bits(want)), (k, pixel, heading)
        dist = want.copy()
        dist -= dist.min()
        assert np.array_equal(bits(oracle.local_distance_map(gm, pixel, rot)), bits(dist)), (k, pixel, heading)
        n += 1
        if k % 8 == 0:                                     # robot and overhead maps of 1-4 robots near this one
            robots, stamps = [], []
            for r in range(1 + k // 8 % 4):
                rp = (int(np.clip(pixel[0] + rng.randint(-30, 31), 68, rows - 68)), int(np.clip(pixel[1] + rng.randint(-30, 31), 68, cols - 68)))
                rh = SPECIAL_HEADINGS[(k + r) % len(SPECIAL_HEADINGS)] if r == 0 else rng.uniform(-math.pi, math.pi)
                mask, seg_mask = int(rng.randint(len(masks))), int(rng.randint(len(masks)))
                seg_value, map_value = float(rng.randint(5, 9)) / 8, float(rng.choice([0.5, 1.0]))
                robots.append((rp, rh, mask, seg_value, map_value, seg_mask))
                stamps.append((rp, oracle.mask_rotation(rh), mask, seg_value, map_value, seg_mask))
            base = (rng.rand(rows, cols) * 0.5).astype(np.float32)
            want_r = scipy_local_map(scipy_robot_map((rows, cols), robots, masks, False), pixel, heading)
            seg = scipy_robot_map((rows, cols), robots, masks, True)
            over = base.copy()
            over[seg > 0] = seg[seg > 0]
            want_o = scipy_local_map(over, pixel, heading)
            got = oracle.state([base], ['robots', ('overhead', 0)], pixel, rot, stamps, masks)
            assert np.array_equal(bits(got[:, :, 0]), bits(want_r)) and np.array_equal(bits(got[:, :, 1]), bits(want_o)), (k, robots)
            assert want_r.max() > 0
    assert n >= 500


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_export_is_declared_bound_and_laid_out(L):
    import subprocess
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    for name in ('simq_local_state_images', 'simq_local_state_desc_bytes'):
        assert name + '(' in text and name in L.EXPORTS and hasattr(ctypes.CDLL(L.LIB_PATH), name)
    # the version script exports the simq_ prefix and nothing else; the new names are among the dynamic symbols
    assert 'global: simq_*; local: *;' in open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'libsimq.map')).read()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert ' T simq_local_state_images' in out and ' T simq_local_state_desc_bytes' in out
    from simq import local_maps as lm
    layout = lambda cls: [(f, getattr(cls, f).offset) for f, _ in cls._fields_]
    assert ctypes.sizeof(lm.Rotation) == 56 and layout(lm.Rotation) == [('r', 0), ('offset', 32), ('shape', 48)]
    assert ctypes.sizeof(lm.LocalMap) == 16 and layout(lm.LocalMap) == [('d_data', 0), ('rows', 8), ('cols', 12)]
    assert ctypes.sizeof(lm.LocalRobot) == 80 and layout(lm.LocalRobot) == [
        ('rot', 0), ('pixel_i', 56), ('pixel_j', 60), ('mask', 64), ('seg_value', 68), ('map_value', 72), ('seg_mask', 76)]
    assert ctypes.sizeof(lm.LocalProblem) == 80 and layout(lm.LocalProblem) == [
        ('rot', 0), ('pixel_i', 56), ('pixel_j', 60), ('rows', 64), ('cols', 68), ('robot_begin', 72), ('robot_count', 76)]
    assert ctypes.sizeof(lm.LocalChannel) == 16 and layout(lm.LocalChannel) == [('kind', 0), ('map', 4), ('value', 8), ('reserved_', 12)]
    assert L.lib.c.simq_local_state_desc_bytes(3, 5, 7, 4) == 3 * 16 + 5 * 80 + 7 * 80 + 7 * 4 * 16
    assert L.lib.c.simq_local_state_desc_bytes(-1, 0, 1, 1) == -1
    for name, code in lm.KINDS.items():
        assert '#define SIMQ_LOCAL_%s %d' % (name.upper(), code) in text
    import simq
    assert simq.local_state_images is lm.local_state_images and simq.local_map is lm.local_map and simq.local_distance_map is lm.local_distance_map


def test_c_abi_rejects_bad_descriptors_before_any_device_call(L):
    """Every check of simq_local_state_images runs on the host before the descriptor copy / launch: the device pointers below are fake
    and never dereferenced."""
    from simq import local_maps as lm
    c = L.lib.c
    MAPS, MASKS, DESC, OUT = 0x10000000, 0x20000000, 0x30000000, 0x40000000

    def rot(n, shape=None, bad=None):
        r = lm.Rotation((ctypes.c_double * 4)(1, 0, -0.0, 1), (ctypes.c_double * 2)(0, 0), (ctypes.c_int32 * 2)(*(shape or (n, n))))
        if bad is not None:
            r.r[1] = bad
        return r

    def call(problem=None, chans=None, maps=None, robots=(), n_masks=2, out=OUT, out_floats=1 << 24, desc=DESC, desc_bytes=1 << 20, n=None,
             masks=MASKS):
        problem = problem or lm.LocalProblem(rot(136), 92, 116, 184, 232, 0, len(robots))
        chans = chans or [lm.LocalChannel(0, 0, 0.0, 0)]
        maps = [lm.LocalMap(MAPS, 184, 232)] if maps is None else maps
        a_maps = (lm.LocalMap * max(len(maps), 1))(*maps)
        a_rob = (lm.LocalRobot * max(len(robots), 1))(*robots)
        a_ch = (lm.LocalChannel * len(chans))(*chans)
        return c.simq_local_state_images(a_maps, len(maps), ctypes.c_void_p(masks), n_masks, a_rob if robots else None, len(robots),
                                         ctypes.byref(problem), 1 if n is None else n, a_ch, len(chans), ctypes.c_void_p(desc), desc_bytes,
                                         ctypes.c_void_p(out), out_floats, None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in L.last_error(), (word, L.last_error())

    robot = lambda **kw: lm.LocalRobot(**dict(dict(rot=rot(96), pixel_i=92, pixel_j=116, mask=0, seg_value=0.625, map_value=1.0, seg_mask=1), **kw))
    refused('NULL', out=None)
    refused('NULL', desc=None)
    refused('n = 0', n=0)
    refused('n_channels', chans=[lm.LocalChannel(4, 0, 0.0, 0)] * 65)
    # the crop inside its map
    for pi, pj in ((67, 116), (117, 116), (92, 67), (92, 165), (-5, 116)):
        refused('crop around pixel', problem=lm.LocalProblem(rot(136), pi, pj, 184, 232, 0, 0))
    for pi, pj in ((68, 68), (116, 164)):                                             # the legal extremes pass this check (and fail a later one)
        refused('kind 5', problem=lm.LocalProblem(rot(136), pi, pj, 184, 232, 0, 0), chans=[lm.LocalChannel(5, 0, 0.0, 0)])
    # rotated shapes, finite doubles
    refused('rotated crop shape', problem=lm.LocalProblem(rot(136, (135, 136)), 92, 116, 184, 232, 0, 0))
    refused('rotated crop shape', problem=lm.LocalProblem(rot(136, (136, 194)), 92, 116, 184, 232, 0, 0))
    refused('not finite', problem=lm.LocalProblem(rot(136, bad=float('nan')), 92, 116, 184, 232, 0, 0))
    refused('not finite', problem=lm.LocalProblem(rot(136, bad=float('inf')), 92, 116, 184, 232, 0, 0))
    refused('rotated mask shape', robots=[robot(rot=rot(96, (96, 137)))])
    refused('rotated mask shape', robots=[robot(rot=rot(96, (95, 96)))])
    refused('not finite', robots=[robot(rot=rot(96, bad=float('nan')))])
    # indices
    refused('map 1 outside', chans=[lm.LocalChannel(1, 1, 0.0, 0)])
    refused('map -1 outside', chans=[lm.LocalChannel(3, -1, 0.0, 0)])
    refused('kind 5', chans=[lm.LocalChannel(5, 0, 0.0, 0)])
    refused('kind -1', chans=[lm.LocalChannel(-1, 0, 0.0, 0)])
    refused('outside the bank', robots=[robot(mask=2)])
    refused('outside the bank', robots=[robot(seg_mask=-1)])
    refused('outside the 1 given', robots=[robot()], problem=lm.LocalProblem(rot(136), 92, 116, 184, 232, 0, 2))
    refused('outside the 1 given', robots=[robot()], problem=lm.LocalProblem(rot(136), 92, 116, 184, 232, -1, 1))
    refused('mask bank', robots=[robot()], n_masks=0)
    # a map of another shape than the problem's; a map too small for any crop
    refused('the problem\'s maps are', maps=[lm.LocalMap(MAPS, 232, 232)])
    refused('rows, cols >= 136', maps=[lm.LocalMap(MAPS, 100, 232)])
    refused('NULL or misaligned', maps=[lm.LocalMap(0, 184, 232)])
    refused('NULL or misaligned', maps=[lm.LocalMap(MAPS + 2, 184, 232)])
    # every stamp inside the map
    for pi, pj in ((47, 116), (137, 116), (92, 47), (92, 185)):
        refused('leaves the 184 x 232 map', robots=[robot(pixel_i=pi, pixel_j=pj)])
    # buffers
    refused('d_out holds', out_floats=9215)
    refused('d_desc holds', desc_bytes=16 + 80 + 16 - 1)
    refused('aligned', desc=DESC + 4)
    refused('aligned', out=OUT + 2)
    refused('overlaps map 0', out=MAPS + 184 * 232 * 4 - 4)
    refused('overlaps map 0', out=MAPS - 9216 * 4 + 4)
    refused('overlaps the mask bank', out=MASKS + 4, robots=[robot()])
    refused('overlaps d_desc', out=DESC + 8)


def test_the_stamp_that_just_fits_is_not_refused_for_its_place(L):
    """Pixel 116 with a 136-row rotated mask covers rows [48, 184) of a 184-row map and passes the stamp check: the call is refused
    only by the channel check that follows it."""
    from simq import local_maps as lm
    r = lm.Rotation((ctypes.c_double * 4)(1, 0, 0, 1), (ctypes.c_double * 2)(0, 0), (ctypes.c_int32 * 2)(136, 136))
    rob = (lm.LocalRobot * 1)(lm.LocalRobot(r, 116, 116, 0, 0.625, 1.0, 0))
    r2 = lm.Rotation((ctypes.c_double * 4)(1, 0, 0, 1), (ctypes.c_double * 2)(0, 0), (ctypes.c_int32 * 2)(136, 136))
    prob = lm.LocalProblem(r2, 92, 116, 184, 232, 0, 1)
    ch = (lm.LocalChannel * 1)(lm.LocalChannel(7, 0, 0.0, 0))
    rc = L.lib.c.simq_local_state_images(None, 0, ctypes.c_void_p(0x20000000), 1, rob, 1, ctypes.byref(prob), 1, ch, 1,
                                         ctypes.c_void_p(0x30000000), 1 << 20, ctypes.c_void_p(0x40000000), 1 << 20, None)
    assert rc == -1 and 'kind 7' in L.last_error()


def test_python_rejects_bad_input_before_touching_a_device(L, monkeypatch):
    import torch
    import simq
    from simq import local_maps as lm
    good = np.zeros((184, 232), np.float32)
    pose = ((0.0, 0.0), 0.0)
    # without a device nothing runs (and nothing falls back to the host)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.local_state_images([good], [('map', 0)], [pose])
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.local_map(good, (0.0, 0.0), 0.0)
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.local_distance_map(good, (0.0, 0.0), 0.0)
    # the input contract (checked with a stand-in device so that the checks are reached)
    monkeypatch.setattr(lm._batch, 'device', lambda what: torch.device('cpu'))
    for bad in (good.astype(np.float64), good.astype(np.uint8), np.zeros(5, np.float32), good.tolist(), torch.zeros(184, 232, dtype=torch.float64)):
        with pytest.raises(ValueError):
            simq.local_state_images([bad], [('map', 0)], [pose])
    for chans in ([('map', 1)], [('map',)], [('nonsense', 0)], [('robots', 1)], [('constant',)], [('map', 0, 0)], [[('map', 0)], [('map', 0)]],
                  [[('map', 0)], [('map', 0), ('map', 0)]]):
        with pytest.raises(ValueError):
            simq.local_state_images([good], chans, [pose] * (2 if len(chans) == 2 and isinstance(chans[1], list) and len(chans[1]) == 2 else 1))
    with pytest.raises(ValueError, match='map_shape'):
        simq.local_state_images([], [('constant', 1.0)], [pose])
    with pytest.raises(ValueError, match='map_shape'):
        simq.local_state_images([good], [('map', 0)], [pose], map_shape=(232, 232))
    with pytest.raises(ValueError, match='pose'):
        simq.local_state_images([good], [('map', 0)], [0.5])
    with pytest.raises(ValueError, match='masks'):
        simq.local_state_images([good], ['robots', ('map', 0)], [pose], robots=[[lm.RobotStamp((0, 0), 0.0, 0, 0.625)]])
    with pytest.raises(ValueError, match='masks'):
        simq.local_state_images([good], ['robots', ('map', 0)], [pose], robots=[[lm.RobotStamp((0, 0), 0.0, 0, 0.625)]], masks=np.zeros((1, 96, 95), np.float32))
    with pytest.raises(ValueError, match='out'):
        simq.local_state_images([good], [('map', 0)], [pose], out=torch.zeros(1, 96, 96, 2))
    # the reference's pixel rule and scipy's rotation, as this package restates them
    assert lm.position_to_pixel_indices(0.0, 0.0, (184, 232)) == (92, 116)
    assert lm.position_to_pixel_indices(-5.0, 5.0, (184, 232)) == (0, 0) and lm.position_to_pixel_indices(5.0, -5.0, (184, 232)) == (183, 231)
    pytest.importorskip('scipy.special')
    for angle, n in ((0.0, 136), (90.0, 136), (45.0, 96), (-33.3, 136)):
        a, b = lm.rotation(angle, n), oracle.rotation(angle, n)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert tuple(lm.rotation(90.0, 136)[2]) == (136, 136) and tuple(lm.rotation(45.0, 136)[2]) == (192, 192)


def test_the_coordinate_path_is_compiled_without_contraction(tmp_path):
    """The rotated-image coordinate must be offset + (oi * R0 + oj * R1) with every product and sum rounded on its own: a fused
    multiply-add moves near-tie pixels (20 of a 45-degree fixture image with hipcc's default contraction, whose HIP __dmul_rn / __dadd_rn are
    plain operators).  The kernel's ISA for gfx950 holds float64 multiplies and adds and no fused form."""
    import re
    import shutil
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        hipcc = shutil.which('hipcc')
    if not hipcc:
        pytest.skip('hipcc not found: the ISA cannot be produced')
    src = os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'local_maps.hip')
    out = str(tmp_path / 'local_maps.s')
    flags = re.search(r'^CXXFLAGS\s*:=\s*(.*)$', open(os.path.join(os.path.dirname(src), 'Makefile')).read(), flags=re.M).group(1)
    flags = flags.replace('$(ARCH)', 'gfx950').split()
    subprocess.run([hipcc] + flags + ['--cuda-device-only', '-S', '-o', out, src], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    ops = set(re.findall(r'\bv_[a-z0-9_]*f64[a-z0-9_]*', open(out).read()))
    assert any(o.startswith('v_mul_f64') for o in ops) and any(o.startswith('v_add_f64') for o in ops), ops
    fused = [o for o in ops if re.match(r'v_(fma|fmac|mad|mac|pk_fma)', o)]
    assert not fused, fused
