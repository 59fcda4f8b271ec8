"""CPU: the intention-map oracle (tests/intention_maps_oracle.py) against the reference Mapper's own maps
(tests/golden/intention_maps_*.npz, written by tools/gen_intention_maps_golden.py) bit for bit; its line model, ramp values and
dilation against the sequential line algorithm, np.linspace and scipy.ndimage.grey_dilation on fresh random cases; the C-ABI entry
point simq_intention_maps, its descriptor layout and its argument checks (no kernel is launched here); the Python input contract."""
import ctypes
import glob
import os

import numpy as np
import pytest

import intention_maps_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'intention_maps_*.npz')))
    assert len(files) == 2, files
    return [(os.path.basename(f), oracle.load_fixture(f)) for f in files]


def octant(seg):
    """(sign of dr, sign of dc, kind) of a segment: kind 0 axis-aligned, 1 exact 45 degrees, 2 steep, 3 shallow."""
    dr, dc = seg[2] - seg[0], seg[3] - seg[1]
    kind = 0 if dr == 0 or dc == 0 else 1 if abs(dr) == abs(dc) else 2 if abs(dr) > abs(dc) else 3
    return int(np.sign(dr)), int(np.sign(dc)), kind


def test_fixtures_cover_the_issue_cases(golden_dir):
    shapes = set()
    for name, fx in fixtures(golden_dir):
        rows, cols = fx['shape']
        shapes.add((rows, cols))
        probs = fx['problems']
        assert fx['maps'].dtype == fx['local'].dtype == np.float32
        assert fx['maps'].shape == (len(probs), rows, cols) and fx['local'].shape == (len(probs), 96, 96)
        assert {p['encoding'] for p in probs} == set(oracle.ENCODINGS)                              # all five encodings
        assert {p['thickness'] for p in probs} >= {1, 2, 3}
        assert any(p['scale'] != 1 and p['encoding'] == 'ramp' for p in probs) and any(p['scale'] != 1 and p['encoding'] == 'binary' for p in probs)
        segs = [s for p in probs for s in p['segments']]
        ramps = [s for s in segs if s[4] == oracle.RAMP]
        assert any(s[7] > 0 and s[8] < 0 for s in ramps) and any(s[7] < 0 for s in ramps)         # the path length passes 1: the clip reaches 0
        single = [s for p in probs if p['encoding'] != 'circle' for s in p['segments'] if s[0] == s[2] and s[1] == s[3]]
        assert any(s[5] == 1 for s in single) and any(s[5] == 0 for s in single)                    # len(rr) == 1 mid-path and as the last segment
        assert any(s[5] == 0 and s[4] == oracle.RAMP for s in single)
        kinds = {octant(s) for s in segs}
        for sr in (-1, 1):
            for sc in (-1, 1):
                assert {(sr, sc, 1), (sr, sc, 2), (sr, sc, 3)} <= kinds, (sr, sc)                   # 45 degrees, steep, shallow in every quadrant
        assert {(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)} <= kinds                              # the four axis directions
        # crossing paths of two robots: two robots of one problem whose pixels intersect
        crossed = False
        for p in probs:
            if p['encoding'] == 'binary' and len(p['robots']) >= 2:
                sets = [set(zip(*[x.tolist() for x in np.nonzero(oracle.global_map([r], (rows, cols), 'binary', 1.0, 1))])) for r in p['robots']]
                crossed |= any(sets[a] & sets[b] for a in range(len(sets)) for b in range(a + 1, len(sets)))
        assert crossed
        assert any(p['idle'] > 0 and p['robots'] for p in probs)                                    # an idle robot beside drawn ones
        empty = [k for k, p in enumerate(probs) if not p['robots'] and not p['spatial']]
        assert empty and all(p['idle'] >= 2 for p in (probs[k] for k in empty)) and not fx['maps'][empty].any()       # idle robots only
        # a segment ending on the map border under a dilation
        assert any(p['thickness'] > 1 and any(s[2] in (0, rows - 1) or s[3] in (0, cols - 1) for s in p['segments']) for p in probs)
        assert any(s[2] in (0, rows - 1) and s[3] in (0, cols - 1) for s in segs)                  # ... and one in a corner
        spatial = [p for p in probs if p['spatial']]
        assert len(spatial) >= 3 and all(p['encoding'] == 'circle' and len(p['robots']) <= 1 for p in spatial)
        assert any(not p['robots'] for p in spatial) and any(p['thickness'] == 1 for p in spatial)
        # the local images see the maps
        assert sum(bool(fx['local'][k].any()) for k in range(len(probs))) >= len(probs) // 2
    assert shapes == {(184, 232), (232, 232)}


def test_oracle_equals_the_reference_bit_for_bit(golden_dir):
    """From the paths (the doubles computed here) and from the stored descriptors (no float64 arithmetic on this machine's part but
    the ramp itself)."""
    n = 0
    for name, fx in fixtures(golden_dir):
        for k, p in enumerate(fx['problems']):
            got = oracle.global_map(p['robots'], fx['shape'], p['encoding'], p['scale'], p['thickness'])
            assert got.dtype == np.float32 and np.array_equal(bits(got), bits(fx['maps'][k])), (name, k, p['tag'], p['encoding'])
            got = oracle.draw(p['segments'], fx['shape'], p['thickness'] - 1)
            assert np.array_equal(bits(got), bits(fx['maps'][k])), (name, k, p['tag'], p['encoding'])
            n += 1
    assert n >= 40


def test_stored_doubles_are_what_this_machine_computes(golden_dir):
    """Pixels, modes, flags and the float64 start / stop / step of every segment: sqrt, the products and the sums are IEEE operations,
    so they are equal to the last bit."""
    n = 0
    for name, fx in fixtures(golden_dir):
        for k, p in enumerate(fx['problems']):
            here = oracle.segments(p['robots'], fx['shape'], p['encoding'], p['scale'])
            assert len(here) == len(p['segments'])
            for a, b in zip(here, p['segments']):
                assert tuple(a[:6]) == tuple(b[:6]) and np.float32(a[6]) == np.float32(b[6]), (name, k, a, b)
                assert np.array_equal(np.array(a[7:], np.float64).view(np.int64), np.array(b[7:], np.float64).view(np.int64)), (name, k, a, b)
                n += 1
    assert n >= 200


def random_line(rng, rows, cols, k):
    """Random end points; every fourth line has an end on the border, every 16th is a single pixel or axis-aligned or diagonal."""
    r0, r1 = rng.randint(0, rows, 2)
    c0, c1 = rng.randint(0, cols, 2)
    if k % 4 == 0:
        r1, c1 = [(0, c1), (rows - 1, c1), (r1, 0), (r1, cols - 1), (0, 0), (rows - 1, cols - 1)][k // 4 % 6]
    if k % 16 == 1:
        r1, c1 = r0, c0
    if k % 16 == 2:
        r1 = r0
    if k % 16 == 3:
        c1 = c0
    if k % 16 == 5:
        d = min(abs(r1 - r0), abs(c1 - c0))
        r1, c1 = r0 + d * (1 if r1 >= r0 else -1), c0 + d * (1 if c1 >= c0 else -1)
    return int(r0), int(c0), int(r1), int(c1)


def test_line_model_equals_the_sequential_algorithm():
    rng = np.random.RandomState(11)
    n = 0
    for k in range(2000):
        rows, cols = (184, 232) if k % 2 else (232, 232)
        r0, c0, r1, c1 = random_line(rng, rows, cols, k)
        rr, cc = oracle.sequential_line(r0, c0, r1, c1)
        qr, qc = oracle.line_points(r0, c0, r1, c1)
        assert np.array_equal(rr, qr) and np.array_equal(cc, qc), (r0, c0, r1, c1)
        assert len(rr) == max(abs(r1 - r0), abs(c1 - c0)) + 1 and len(set(zip(rr.tolist(), cc.tolist()))) == len(rr)      # no pixel twice
        assert (rr[0], cc[0]) == (r0, c0) and (rr[-1], cc[-1]) == (r1, c1)
        n += 1
    assert n >= 500


def test_ramp_values_equal_linspace():
    rng = np.random.RandomState(12)
    n = 0
    for k in range(3000):
        num = 1 if k % 50 == 0 else int(rng.randint(1, 300))
        path_length = 0 if k % 7 == 0 else rng.uniform(0, 1.6)
        segment_length = 0.0 if k % 33 == 0 else rng.choice([0.25, 0.5, 1.0, 2.0]) * rng.uniform(0, 1.2)
        start, stop = 1 - path_length, 1 - (path_length + segment_length)
        step = (stop - start) / (num - 1) if num > 1 else 0.0
        want = np.clip(np.linspace(start, stop, num), 0, 1)
        got = oracle.ramp_values(start, stop, step, num)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want.astype(np.float32))), (start, stop, num)
        # assigning the float64 maximum with an fp32 map back into the map is the fp32 maximum with the rounded value
        m = rng.rand(num).astype(np.float32)
        back = m.copy()
        back[:] = np.maximum(m, want)
        assert np.array_equal(bits(back), bits(np.maximum(m, got)))
        n += 1
    assert n >= 500


def test_dilation_equals_scipy_grey_dilation():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(13)
    n = 0
    for k in range(300):
        rows, cols = [(184, 232), (232, 232), (9, 7), (40, 300)][k % 4]
        radius = k % 6
        image = np.zeros((rows, cols), np.float32)
        for _ in range(1 + k % 5):
            r0, c0, r1, c1 = random_line(rng, rows, cols, k + _ * 4)
            rr, cc = oracle.line_points(r0, c0, r1, c1)
            image[rr, cc] = np.maximum(image[rr, cc], rng.rand(len(rr)).astype(np.float32))
        image[0, 0] = image[rows - 1, cols - 1] = image[0, cols // 2] = 0.75          # lit pixels on the border and in the corners
        want = ndimage.grey_dilation(image, footprint=oracle.disk(radius))
        assert np.array_equal(bits(oracle.dilate(image, radius)), bits(want)), (k, radius)
        n += 1
    assert n >= 300


def test_whole_maps_on_fresh_random_paths_equal_the_sequential_pipeline():
    """The reference's sequence of operations (sequential lines, np.linspace, np.maximum assigned back, grey_dilation) restated on
    random paths, lines to the border included, against the oracle's closed forms."""
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(14)
    n = 0
    for k in range(400):
        rows, cols = (184, 232) if k % 2 else (232, 232)
        encoding = oracle.ENCODINGS[1 + k % 4]
        scale, thickness = [1.0, 0.5, 2.0][k % 3], 1 + k % 4
        robots = []
        for _ in range(1 + k % 3):
            pts = [(rng.uniform(-1.6, 1.6), rng.uniform(-1.6, 1.6), 0.0) for _ in range(2 + rng.randint(5))]      # beyond the map: clipped to the border
            if k % 5 == 0:
                pts.insert(1, pts[1])
            robots.append(pts)
        image = np.zeros((rows, cols), np.float32)
        for pts in robots:
            pts = [pts[0], pts[-1]] if encoding == 'line' else pts[::-1] if encoding == 'history' else pts
            path_length = 0
            for i in range(1, len(pts)):
                a, b = pts[i - 1], pts[i]
                seg_len = scale * np.sqrt((b[0] - a[0])**2 + (b[1] - a[1])**2)
                rr, cc = oracle.sequential_line(*oracle.position_to_pixel_indices(a[0], a[1], image.shape),
                                                *oracle.position_to_pixel_indices(b[0], b[1], image.shape))
                values = np.clip(np.linspace(1 - path_length, 1 - (path_length + seg_len), len(rr)), 0, 1)
                if encoding in ('binary', 'line'):
                    values = np.full(len(rr), scale)
                if i < len(pts) - 1:
                    rr, cc, values = rr[:-1], cc[:-1], values[:-1]
                image[rr, cc] = np.maximum(image[rr, cc], values)
                path_length += seg_len
        if thickness > 1:
            image = ndimage.grey_dilation(image, footprint=oracle.disk(thickness - 1))
        got = oracle.global_map(robots, (rows, cols), encoding, scale, thickness)
        assert np.array_equal(bits(got), bits(image)), (k, encoding, scale, thickness)
        n += 1
    assert n >= 300


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_export_is_declared_bound_and_laid_out(L):
    import subprocess
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    for name in ('simq_intention_maps', 'simq_intention_desc_bytes'):
        assert name + '(' in text and name in L.EXPORTS and hasattr(ctypes.CDLL(L.LIB_PATH), name)
    assert 'global: simq_*; local: *;' in open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'libsimq.map')).read()
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert ' T simq_intention_maps' in out and ' T simq_intention_desc_bytes' in out
    assert 'intention_maps.hip' in open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'Makefile')).read()
    from simq import intention_drawing as im
    layout = lambda cls: [(f, getattr(cls, f).offset) for f, _ in cls._fields_]
    assert ctypes.sizeof(im.Segment) == 56 and layout(im.Segment) == [
        ('start', 0), ('stop', 8), ('step', 16), ('r0', 24), ('c0', 28), ('r1', 32), ('c1', 36), ('mode', 40), ('drop_last', 44), ('value', 48),
        ('reserved_', 52)]
    assert ctypes.sizeof(im.Problem) == 8 and layout(im.Problem) == [('seg_begin', 0), ('seg_count', 4)]
    assert L.lib.c.simq_intention_desc_bytes(5, 7) == 5 * 56 + 7 * 8
    assert L.lib.c.simq_intention_desc_bytes(0, 1) == 8 and L.lib.c.simq_intention_desc_bytes(-1, 1) == -1
    assert '#define SIMQ_INTENTION_STORE %d' % im.STORE in text and '#define SIMQ_INTENTION_RAMP %d' % im.RAMP in text
    assert '#define SIMQ_INTENTION_MAX_RADIUS %d' % im.MAX_RADIUS in text
    import simq
    assert simq.intention_maps is im.intention_maps and simq.intention_map is im.intention_map


MAPS_OUT, DESC = 0x40000000, 0x30000000


def c_call(L, segs=None, probs=None, rows=184, cols=232, radius=1, out=MAPS_OUT, out_floats=None, desc=DESC, desc_bytes=1 << 20, n=None,
           n_segs=None):
    """simq_intention_maps on fake device pointers: every check runs on the host before the descriptor copy / launch."""
    from simq import intention_drawing as im
    segs = [im.Segment(1.0, 0.5, -0.05, 10, 10, 20, 15, im.RAMP, 0, 0.0, 0)] if segs is None else segs
    probs = [im.Problem(0, len(segs))] if probs is None else probs
    a_segs = (im.Segment * max(len(segs), 1))(*segs)
    a_probs = (im.Problem * max(len(probs), 1))(*probs)
    n = len(probs) if n is None else n
    return L.lib.c.simq_intention_maps(a_segs if segs else None, len(segs) if n_segs is None else n_segs, a_probs, n, rows, cols, radius,
                                       ctypes.c_void_p(desc), desc_bytes, ctypes.c_void_p(out), n * rows * cols if out_floats is None else out_floats,
                                       None)


def test_c_abi_rejects_bad_descriptors_before_any_device_call(L):
    from simq import intention_drawing as im

    def refused(word, **kw):
        assert c_call(L, **kw) == -1, kw
        assert word in L.last_error(), (word, L.last_error())

    seg = lambda **kw: im.Segment(**dict(dict(start=1.0, stop=0.5, step=-0.05, r0=10, c0=10, r1=20, c1=15, mode=im.RAMP, drop_last=0, value=0.0,
                                              reserved_=0), **kw))
    refused('NULL', out=None)
    refused('NULL', desc=None)
    refused('n = 0', n=0, out_floats=1 << 20)
    refused('n_segments = -1', n_segs=-1)
    refused('segments NULL', segs=[], n_segs=1, probs=[im.Problem(0, 0)])
    # end pixels inside the map
    for kw in (dict(r0=-1), dict(r0=184), dict(r1=184), dict(c0=-1), dict(c0=232), dict(c1=232), dict(r1=-7)):
        refused('leaves the 184 x 232 map', segs=[seg(**kw)])
    refused('leaves the 100 x 232 map', segs=[seg(r1=100)], rows=100)
    # modes and flags
    refused('mode 2', segs=[seg(mode=2)])
    refused('mode -1', segs=[seg(mode=-1)])
    refused('drop_last = 2', segs=[seg(drop_last=2)])
    # doubles of a ramp, value of a store
    for field in ('start', 'stop', 'step'):
        for bad in (float('nan'), float('inf'), float('-inf')):
            refused('not finite', segs=[seg(**{field: bad})])
    for bad in (-0.5, -0.0, float('nan'), float('inf')):
        refused('stored value', segs=[seg(mode=im.STORE, value=bad)])
    # ranges
    refused('outside the 1 given', probs=[im.Problem(0, 2)])
    refused('outside the 1 given', probs=[im.Problem(1, 1)])
    refused('outside the 1 given', probs=[im.Problem(-1, 1)])
    refused('outside the 1 given', probs=[im.Problem(0, -1)])
    refused('problem 1', probs=[im.Problem(0, 1), im.Problem(0, 2)])
    # radius, shape
    refused('radius = -1', radius=-1)
    refused('radius = 9', radius=9)
    refused('rows * cols < 2^28', rows=0, out_floats=1 << 20)
    refused('rows * cols < 2^28', cols=-3, out_floats=1 << 20)
    refused('rows * cols < 2^28', rows=1 << 14, cols=1 << 14, segs=[], probs=[im.Problem(0, 0)])
    # buffers
    refused('d_out holds', out_floats=184 * 232 - 1)
    refused('d_out holds', probs=[im.Problem(0, 1)] * 3, out_floats=3 * 184 * 232 - 1)
    refused('d_desc holds', desc_bytes=56 + 8 - 1)
    refused('aligned', desc=DESC + 4)
    refused('aligned', out=MAPS_OUT + 2)
    refused('overlaps d_desc', out=DESC + 8)
    refused('overlaps d_desc', out=DESC - 184 * 232 * 4 + 8)


def test_the_case_that_just_fits_is_not_refused(L):
    """Segments from corner to corner, the largest radius, a stored value of +0, buffers of exactly the needed size: every check but
    the one corrupted last passes (the call is refused only by it, so nothing touches the fake pointers)."""
    from simq import intention_drawing as im
    segs = [im.Segment(1.0, -3.0, -0.01, 0, 0, 183, 231, im.RAMP, 1, 0.0, 0), im.Segment(0.0, 0.0, 0.0, 183, 231, 0, 0, im.STORE, 0, 0.0, 0),
            im.Segment(-5.0, -6.0, 0.0, 183, 0, 183, 0, im.RAMP, 0, 0.0, 0)]
    probs = [im.Problem(0, 3), im.Problem(3, 0), im.Problem(1, 2)]
    kw = dict(segs=segs, probs=probs, radius=8, desc_bytes=3 * 56 + 3 * 8, out_floats=3 * 184 * 232)
    assert c_call(L, **dict(kw, probs=probs + [im.Problem(2, 2)], desc_bytes=3 * 56 + 4 * 8, out_floats=4 * 184 * 232)) == -1
    assert 'problem 3: segments [2, 2 + 2) outside the 3 given' in L.last_error()
    assert c_call(L, **dict(kw, out=DESC + 3 * 56 + 3 * 8 - 4)) == -1 and 'overlaps d_desc' in L.last_error()
    # ... and d_out right behind the descriptors is no overlap: only the problem range is refused
    assert c_call(L, **dict(kw, probs=probs[:2] + [im.Problem(1, 3)], out=DESC + 3 * 56 + 3 * 8)) == -1
    assert 'problem 2' in L.last_error()


def test_python_rejects_bad_input_before_touching_a_device(L, monkeypatch):
    import torch
    import simq
    from simq import intention_drawing as im
    path = [(0.0, 0.0, 0.0), (0.2, 0.1, 0.0)]
    # without a device nothing runs (and nothing falls back to the host)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.intention_maps([[path]], (184, 232), 'ramp')
    with pytest.raises(L.SimqError, match='MI355X'):
        simq.intention_map([path], (184, 232), 'ramp')
    # the argument checks come first: they raise without a device too
    for kw in (dict(paths=[]), dict(map_shape=(184,)), dict(map_shape=(184, 232, 3)), dict(map_shape=(0, 232)), dict(map_shape=None),
               dict(encoding='spiral'), dict(encoding=['ramp', 'ramp']), dict(encoding=None), dict(line_thickness=0),
               dict(line_thickness=10), dict(line_thickness=1.5), dict(scale=-1.0), dict(scale=float('nan')), dict(scale=-0.0),
               dict(paths=[[0.5]]), dict(paths=[[[]]]), dict(paths=[[path]], encoding='circle'), dict(paths=[[(0.1, 0.2, 0.0)]], encoding='binary')):
        args = dict(dict(paths=[[path]], map_shape=(184, 232), encoding='ramp'), **kw)
        with pytest.raises((ValueError, TypeError)):
            simq.intention_maps(**args)
    monkeypatch.setattr(im._batch, 'device', lambda what: torch.device('cpu'))
    with pytest.raises(ValueError, match='out'):
        simq.intention_maps([[path]], (184, 232), 'ramp', out=torch.zeros(1, 184, 231))
    with pytest.raises(ValueError, match='out'):
        simq.intention_maps([[path]], (184, 232), 'ramp', out=torch.zeros(1, 184, 232, dtype=torch.float64))
    # the descriptors this package computes are the oracle's
    for enc in oracle.ENCODINGS:
        robots = [(0.3, -0.2, 0.0)] if enc == 'circle' else [path + [(0.2, 0.1, 0.0), (-0.7, 0.6, 0.0)], path]
        assert im.segments(robots, (184, 232), enc, 0.5) == oracle.segments(robots, (184, 232), enc, 0.5)


def test_the_value_path_is_compiled_without_contraction(tmp_path):
    """A ramp value must be i * step + start with the product and the sum rounded on their own, as np.linspace rounds them: the
    kernel's ISA for gfx950 holds a float64 multiply and a float64 add and no fused form."""
    import re
    import shutil
    import subprocess
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        hipcc = shutil.which('hipcc')
    if not hipcc:
        pytest.skip('hipcc not found: the ISA cannot be produced')
    src = os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'intention_maps.hip')
    out = str(tmp_path / 'intention_maps.s')
    flags = re.search(r'^CXXFLAGS\s*:=\s*(.*)$', open(os.path.join(os.path.dirname(src), 'Makefile')).read(), flags=re.M).group(1)
    flags = flags.replace('$(ARCH)', 'gfx950').split()
    subprocess.run([hipcc] + flags + ['--cuda-device-only', '-S', '-o', out, src], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    text = open(out).read()
    ops = set(re.findall(r'\bv_[a-z0-9_]*f64[a-z0-9_]*', text))
    assert any(o.startswith('v_mul_f64') for o in ops) and any(o.startswith('v_add_f64') for o in ops), ops
    fused = [o for o in ops if re.match(r'v_(fma|fmac|mad|mac|pk_fma)', o)]
    assert not fused, fused
    assert 'ds_max_u32' in text                                                   # the maximum is taken on bit patterns, in LDS
