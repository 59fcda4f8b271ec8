"""CPU: the numpy oracle of the observation maps (tests/observation_maps_oracle.py) against the fixtures the reference's own Mapper
and OccupancyMap wrote (tools/gen_observation_maps_golden.py), against a direct restatement of the arithmetic, and the ISA of the
kernel's projection."""
import os
import re

import numpy as np
import pytest

import observation_maps_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ('observation_maps_184x232.npz', 'observation_maps_232x232.npz')
F = np.float32


@pytest.mark.parametrize('fname', FILES)
def test_oracle_equals_the_reference_fixtures_under_the_tie_condition(golden_dir, fname):
    """A pixel is ambiguous when its highest points carry more than one seg value.  Off those pixels the oracle's overhead map equals
    the reference's bit for bit; on them the reference holds one of the tied values.  Ambiguous pixels occur only in tie_* cases and
    are at most 1 % of the file's written pixels.  The occupancy maps are equal everywhere."""
    top, cases = oracle.load_fixture(os.path.join(golden_dir, fname))
    names = [n for n, _ in cases]
    for want in ('flat_floor', 'boxes_cubes', 'obstacle_edge', 'near_wall_corner', 'unknown_ids', 'no_receptacle', 'successive_step2',
                 'tie_receptacle_a', 'tie_receptacle_b', 'forward_far', 'forward_wall'):
        assert want in names
    n_written = n_ambiguous = 0
    shapes = set()
    for name, rec in cases:
        over, occ = rec['overhead_before'].copy(), rec['occupancy_before'].copy()
        assert oracle.update(over, occ, rec['depth'], rec['ids'], rec['geometry'], rec['ranges']) == 0
        written, ambiguous, tied = oracle.tied_pixels(over.shape, rec['depth'], rec['ids'], rec['geometry'], rec['ranges'])
        ref = rec['overhead_after']
        assert np.array_equal(over[~ambiguous].view(np.int32), ref[~ambiguous].view(np.int32)), name
        assert np.array_equal(ref[~written].view(np.int32), rec['overhead_before'][~written].view(np.int32)), name
        for (i, j), values in tied.items():
            assert len(values) > 1 and float(ref[i, j]) in values and float(over[i, j]) in values, (name, i, j)
        assert len(tied) == int(ambiguous.sum())
        assert np.array_equal(occ, rec['occupancy_after']), name
        assert name.startswith('tie_') == bool(ambiguous.any()), (name, int(ambiguous.sum()))
        n_written += int(written.sum())
        n_ambiguous += int(ambiguous.sum())
        shapes.add(rec['depth'].shape)
        # the stored vectors are what the camera parameters give
        c = rec['camera_constants']
        g = oracle.camera_geometry(rec['camera'][0], rec['camera'][1], rec['camera'][2], c[0], c[1], c[2], int(c[3]), c[4])
        for a, b in zip(g, rec['geometry']):
            assert np.array_equal(np.asarray(a, F).view(np.int32), np.asarray(b, F).view(np.int32)), name
    assert 0 < n_ambiguous <= 0.01 * n_written
    assert shapes == {(156, 156), (156, 277)}
    assert top['room_mask'].shape == cases[0][1]['overhead_after'].shape == tuple(int(x) for x in fname[17:24].split('x'))
    # successive updates start where the previous one ended
    rec = dict(cases)
    for a, b in (('successive_step0', 'successive_step1'), ('successive_step1', 'successive_step2')):
        assert np.array_equal(rec[a]['overhead_after'], rec[b]['overhead_before']) and np.array_equal(rec[a]['occupancy_after'], rec[b]['occupancy_before'])


def test_oracle_arithmetic_equals_a_direct_numpy_restatement():
    """Depth, points and pixel indices of the oracle (one explicit float32 operation at a time) against the array expressions numpy
    evaluates when Python scalars meet float32 arrays, on 3 000 fresh random poses and buffers of both cameras."""
    rng = np.random.RandomState(5)
    for k in range(3000):
        forward = k % 2 == 1
        near, far, aspect = (0.001, 1, 16.0 / 9) if forward else (0.1, 10, 1)
        heading = rng.uniform(-np.pi, np.pi)
        x, y = rng.uniform(-1.2, 1.2, 2)
        if forward:
            position = (x, y, 0.08)
            target = (x + 0.14 * np.cos(heading), y + 0.14 * np.sin(heading), 0)
            up = (0.5 * np.cos(heading), 0.5 * np.sin(heading), 0.87)
        else:
            position, target, up = (x, y, 1), (x, y, 0), (np.cos(heading), np.sin(heading), 0)
        H = 9
        g = oracle.camera_geometry(position, target, up, near, far, aspect, H)
        W = g.pixel_x.size
        assert W == int(aspect * H) and all(np.asarray(a).dtype == F for a in g)
        buffer = rng.uniform(0, 1, (H, W)).astype(F)
        if k % 7 == 0:
            buffer[rng.randint(H), rng.randint(W)] = 1.0
        depth = far * near / (far - (far - near) * buffer)
        assert depth.dtype == F and np.array_equal(depth.view(np.int32), oracle.depth_of(buffer, g).view(np.int32))
        xv, yv = np.meshgrid(g.pixel_x, g.pixel_y)
        points = g.position + depth[:, :, np.newaxis] * (g.principal + xv[:, :, np.newaxis] * g.right + yv[:, :, np.newaxis] * g.up)
        got = oracle.points_of(buffer, g)
        assert points.dtype == F and np.array_equal(points.view(np.int32), got.view(np.int32))
        shape = ((184, 232), (232, 232))[k % 3 == 0]
        i = np.clip(np.floor(shape[0] / 2 - points[:, :, 1] * 96.0).astype(np.int32), 0, shape[0] - 1)
        j = np.clip(np.floor(shape[1] / 2 + points[:, :, 0] * 96.0).astype(np.int32), 0, shape[1] - 1)
        gi, gj = oracle.pixel_indices(points[:, :, 0], points[:, :, 1], shape)
        assert np.array_equal(i, gi) and np.array_equal(j, gj)


def test_oracle_order_rule_and_non_finite_frames():
    """Equal heights: the largest frame index stays (-0 equals +0).  A frame with a point that is not finite changes nothing."""
    g = oracle.Geometry(*[np.asarray(v, F) for v in ((0, 0, 1), (0, 0, -1), (0, -1, 0), (1, 0, 0), (0.0, 0.001, 0.002, 0.003), (0.0,))], F(1), F(10), F(8))
    r = oracle.IdRanges(3, 9, 10, 11, 20)
    buffer = np.full((1, 4), 1.125, F)                              # depth 1 / (10 - 8 * 1.125) = 1: z = 1 - 1 = 0 for every point
    assert np.all(oracle.points_of(buffer, g)[:, :, 2] == 0)
    over, occ = np.full((8, 8), -7, F), np.zeros((8, 8), np.uint8)
    assert oracle.update(over, occ, buffer, np.asarray([[0, 10, 3, 12]], np.int32), g, r) == 0
    assert over[4, 4] == F(0.5) and (over != -7).sum() == 1 and occ[4, 4] == 1 and occ.sum() == 1
    assert oracle.update(over, occ, buffer, np.asarray([[12, 3, 10, 0]], np.int32), g, r) == 0 and over[4, 4] == F(0.125)
    bad = buffer.copy()
    bad[0, 2] = 1.25                                                # 10 - 8 * 1.25 = 0: an infinite depth
    before = over.copy()
    assert oracle.update(over, occ, bad, np.asarray([[12, 12, 12, 12]], np.int32), g, r) == 1 and np.array_equal(over, before)


def test_the_projection_is_compiled_without_contraction(tmp_path):
    """cam + depth * ((principal + px * right) + py * up) and rows / 2 - y * 96 need every product and sum rounded on its own.  The
    kernel's ISA for gfx950 holds no fused multiply-add but the five of each correctly rounded division (the v_div_scale / v_rcp /
    v_div_fmas / v_div_fixup sequence: two refinements of the reciprocal, the quotient's residual twice and its correction), and
    holds the separate multiplies and adds: per projected point 13 products (one in the depth, six with px / py, three with the
    depth, two pixel scales, one of the division itself) and 12 sums."""
    import shutil
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        hipcc = shutil.which('hipcc')
    assert hipcc, 'hipcc not found (set HIPCC): the ISA check is part of what pins the arithmetic and is not skipped'
    src = os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'observation_maps.hip')
    assert '#pragma clang fp contract(off)' in open(src).read()
    out = str(tmp_path / 'observation_maps.s')
    flags = re.search(r'^CXXFLAGS\s*:=\s*(.*)$', open(os.path.join(os.path.dirname(src), 'Makefile')).read(), flags=re.M).group(1)
    flags = flags.replace('$(ARCH)', 'gfx950').split()
    subprocess.run([hipcc] + flags + ['--cuda-device-only', '-S', '-o', out, src], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    ops = re.findall(r'^\s+(v_[a-z0-9_]+)', open(out).read(), flags=re.M)
    count = lambda *prefixes: sum(o.startswith(prefixes) for o in ops)
    divisions = count('v_div_fixup_f32')
    assert divisions >= 1 and divisions == count('v_div_fmas_f32')
    assert not [o for o in ops if re.match(r'v_(mad|mac|pk_fma|dot)', o) and 'f32' in o], sorted(set(ops))
    assert not [o for o in ops if re.match(r'v_(fma|fmac|mad|mac)[a-z0-9_]*(f16|f64|bf16)', o)], sorted(set(ops))
    assert count('v_fma_f32', 'v_fmac_f32', 'v_fmaak_f32', 'v_fmamk_f32') == 5 * divisions, sorted(set(ops))
    assert count('v_mul_f32') + 2 * count('v_pk_mul_f32') >= 13 * divisions
    assert count('v_add_f32', 'v_sub_f32', 'v_subrev_f32') + 2 * count('v_pk_add_f32') >= 12 * divisions


def test_python_interface_checks_arguments_before_touching_a_device():
    import __graft_entry__ as ge
    ge.build()
    import simq
    from simq import observation as ob
    c = 1.63 * 96
    g = simq.camera_geometry((0.1, 0.2, 1), (0.1, 0.2, 0), (1, 0, 0), 0.1, 10, 1, int(c))
    want = oracle.camera_geometry((0.1, 0.2, 1), (0.1, 0.2, 0), (1, 0, 0), 0.1, 10, 1, int(c))
    for a, b in zip(g, want):
        assert np.asarray(a).dtype == F and np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))
    assert g.pixel_x.shape == (156,) and simq.camera_geometry((0, 0, 0.1), (1, 0, 0), (0, 0, 1), 0.001, 1, 16.0 / 9, 156).pixel_x.shape == (277,)
    import ctypes
    assert ctypes.sizeof(ob.ObservationProblem) == 152
    r = ob.IdRanges(3, 9, None, 11, 20)
    depth, ids = np.zeros((156, 156), F), np.zeros((156, 156), np.int32)
    with pytest.raises(ValueError):
        simq.observation_update([depth.astype(np.float64)], [ids], g, r, [], [])
    with pytest.raises(ValueError):
        simq.observation_update([depth], [ids.astype(np.int64)], g, r, [], [])
    with pytest.raises(ValueError):
        simq.observation_update([depth], [ids, ids], g, r, [], [])
    with pytest.raises(ValueError):
        simq.observation_update([depth], [ids], [g, g], r, [], [])


def test_library_validates_descriptors_before_any_device_call():
    """simq_observation_update refuses, with a message and before any copy or launch (there is no device here), what its header says."""
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib as L
    from simq.observation import ObservationProblem
    H = W = 4
    rows = cols = 8

    def problem(**kw):
        p = ObservationProblem()
        p.depth_offset, p.ids_offset, p.px_offset, p.py_offset = 0, 16, 32, 36
        p.far_near, p.far, p.far_minus_near = 1, 10, 9.9
        p.height, p.width, p.rows, p.cols = H, W, rows, cols
        p.occupancy_offset = p.overhead_offset = 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    # fake, well-separated, aligned device addresses: validation fails before anything dereferences them
    frames, probs_dev, over, occ, status = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def call(ps, frames=frames, words=40, over=over, floats=2 * rows * cols, occ=occ, nbytes=2 * rows * cols, status=status, probs_dev=probs_dev):
        arr = (ObservationProblem * len(ps))(*ps)
        rc = L.lib.c.simq_observation_update(ctypes.c_void_p(frames), words, arr, len(ps), ctypes.c_void_p(probs_dev), ctypes.c_void_p(over), floats,
                                             ctypes.c_void_p(occ), nbytes, ctypes.c_void_p(status), None)
        return rc, L.last_error()

    for ps, kw, word in (
            ([problem(height=0)], {}, 'frame'), ([problem(rows=0)], {}, 'maps of'), ([problem(rows=1 << 24, cols=1)], {}, 'maps of'),
            ([problem(rows=1, cols=1 << 24)], {}, 'maps of'), ([problem(depth_offset=25)], {}, 'depth words'),
            ([problem(ids_offset=-1)], {}, 'id words'), ([problem(px_offset=37)], {}, 'px words'), ([problem(overhead_offset=65)], {}, 'overhead floats'),
            ([problem(occupancy_offset=65)], {}, 'occupancy bytes'), ([problem(far=float('nan'))], {}, 'not finite'),
            ([problem(has_receptacle=2)], {}, 'has_receptacle'),
            ([problem(), problem()], {}, 'share memory'),                                                     # two problems, one pair of maps
            ([problem(), problem(overhead_offset=64)], {}, 'share memory'),                                   # ... one occupancy map
            ([problem(), problem(overhead_offset=32, occupancy_offset=64)], {}, 'share memory'),              # overlapping overhead maps
            ([problem()], {'occ': over + 16}, 'share memory'),                                                # occupancy inside the overhead map
            ([problem()], {'frames': over + 64}, 'overlaps d_frames'), ([problem()], {'status': occ + 8}, 'overlaps d_status'),
            ([problem()], {'probs_dev': over}, 'overlaps d_problems'), ([problem()], {'over': over + 2}, 'aligned'),
            ([problem()], {'frames': 0}, 'NULL')):
        rc, msg = call(ps, **kw)
        assert rc != 0 and word in msg, (word, msg)
    assert L.lib.c.simq_observation_update(None, 0, None, 0, None, None, 0, None, 0, None, None) != 0 and 'NULL' in L.last_error()
