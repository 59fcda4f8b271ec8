"""GPU: simq_intention_maps_shapes / simq.intention_maps with lists of shapes and thicknesses against the
reference Mapper's own maps (tests/golden/intention_maps_*.npz) and the numpy oracle (tests/intention_maps_oracle.py), bit for bit
(compared as int32 bit patterns): problems of both room shapes and of every stored thickness in one launch, the tile and halo edges at
the smallest shapes that have them, maps placed in any order with gaps, the grid of a large map beside a small one, the chain into
simq.local_state_images, and every refusal on real device buffers."""
import copy
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import intention_maps_oracle as oracle

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF                                                   # a NaN with a payload: any float left unwritten shows
STORE, RAMP = oracle.STORE, oracle.RAMP


@pytest.fixture(scope='module')
def S():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope='module')
def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'intention_maps_*.npz')))
    assert len(files) == 2, files
    fxs = [oracle.load_fixture(f) for f in files]
    assert [fx['shape'] for fx in fxs] == [(184, 232), (232, 232)]
    return fxs


def interleaved(fixtures):
    """(fixture, problem index) of every problem of both files, alternating between the files while both last."""
    a, b = [[(fx, k) for k in range(len(fx['problems']))] for fx in fixtures]
    both = [x for pair in zip(a, b) for x in pair]
    return both + a[len(b):] + b[len(a):]


def tiles(shape):
    return -(-shape[0] // 32) * -(-shape[1] // 256)


def launch(problems, offsets=None, total=None):
    """One simq_intention_maps_shapes call.  problems: dicts with 'shape', 'radius' and either 'segments' (tuples as the oracle takes
    them) or 'share' (the index of an earlier problem whose segment range it names).  offsets: where each map begins in d_out (packed
    in order without it); total: the floats of d_out.  d_out is filled with SENT first.  Returns (d_out's bit patterns, the offsets,
    the launch log, the tile prefix as the library left it in d_desc)."""
    from simq import _lib, intention_drawing as im
    segs, ranges = [], []
    for p in problems:
        if 'share' in p:
            ranges.append(ranges[p['share']])
            continue
        ranges.append((len(segs), len(p['segments'])))
        segs += [im.Segment(start, stop, step, r0, c0, r1, c1, mode, drop_last, value, 0)
                 for r0, c0, r1, c1, mode, drop_last, value, start, stop, step in p['segments']]
    cells = [p['shape'][0] * p['shape'][1] for p in problems]
    if offsets is None:
        offsets = (np.cumsum(cells) - cells).tolist()
    total = max(o + c for o, c in zip(offsets, cells)) if total is None else total
    c_segs = (im.Segment * max(len(segs), 1))(*segs)
    c_probs = (im.ShapedProblem * len(problems))(*[im.ShapedProblem(o, p['shape'][0], p['shape'][1], b, c, p['radius'], 0)
                                                   for o, p, (b, c) in zip(offsets, problems, ranges)])
    n = len(problems)
    need = _lib.lib.c.simq_intention_shapes_desc_bytes(len(segs), n)
    desc = torch.zeros(need, dtype=torch.uint8, device='cuda')
    out = torch.empty(total, dtype=torch.int32, device='cuda').fill_(SENT)
    _lib.lib.c.simq_launch_counts_reset()
    _lib.lib.call('simq_intention_maps_shapes', c_segs if segs else None, len(segs), c_probs, n, _lib.ptr(desc), ctypes.c_int64(need), _lib.ptr(out),
                  ctypes.c_int64(total), _lib.stream_ptr())
    log = _lib.launch_counts()
    prefix = desc.cpu().numpy()[56 * len(segs) + 32 * n:][:4 * (n + 1)].view(np.int32)
    return out.cpu().numpy(), offsets, log, prefix


def check(problems, want, got, offsets, what):
    """Every map equals `want`, nothing of the fill is left inside a map, and every float outside the maps keeps the fill."""
    outside = np.ones(got.size, bool)
    for p, (prob, o) in enumerate(zip(problems, offsets)):
        rows, cols = prob['shape']
        mine = got[o:o + rows * cols].reshape(rows, cols)
        assert not (mine == SENT).any(), '%s: problem %d: %d pixels were not written' % (what, p, int((mine == SENT).sum()))
        bad = int((mine != bits(want[p])).sum())
        assert bad == 0, '%s: problem %d (%d x %d, radius %d): %d pixels differ' % (what, p, rows, cols, prob['radius'], bad)
        assert outside[o:o + rows * cols].all()
        outside[o:o + rows * cols] = False
    assert (got[outside] == SENT).all(), '%s: %d floats outside the maps were written' % (what, int((got[outside] != SENT).sum()))


def test_every_fixture_problem_of_both_shapes_and_all_thicknesses_in_one_launch(S, fixtures):
    both = interleaved(fixtures)
    assert len(both) >= 40 and {fx['shape'] for fx, _ in both[:2]} == {(184, 232), (232, 232)}
    assert {fx['problems'][k]['thickness'] for fx, k in both} == {1, 2, 3}
    problems = [{'shape': fx['shape'], 'radius': fx['problems'][k]['thickness'] - 1, 'segments': fx['problems'][k]['segments']} for fx, k in both]
    got, offsets, log, prefix = launch(problems)
    assert log == {'intention_maps_shapes': 1}
    check(problems, [fx['maps'][k] for fx, k in both], got, offsets, 'fixtures')
    assert prefix.tolist() == np.concatenate([[0], np.cumsum([tiles(p['shape']) for p in problems])]).tolist()


def test_lists_of_shapes_and_thicknesses_through_the_python_interface(S, fixtures):
    """One call per scale (the one argument the problems of a call still share) with lists for map_shape and line_thickness: each view
    equals the tensor of today's call of that problem alone, with its shape and its thickness."""
    from simq import _lib
    both = interleaved(fixtures)
    n = 0
    for scale in sorted({fx['problems'][k]['scale'] for fx, k in both}):
        mine = [(fx, k) for fx, k in both if fx['problems'][k]['scale'] == scale]
        probs = [fx['problems'][k] for fx, k in mine]
        shapes = [fx['shape'] for fx, _ in mine]
        _lib.lib.c.simq_launch_counts_reset()
        views = S.intention_maps([p['robots'] for p in probs], shapes, [p['encoding'] for p in probs], scale, [p['thickness'] for p in probs])
        assert _lib.launch_counts() == ({'intention_maps_shapes': 1})
        assert isinstance(views, list) and len(views) == len(mine)
        base = views[0].data_ptr()
        for view, shape, p, (fx, k) in zip(views, shapes, probs, mine):
            assert view.is_cuda and view.dtype == torch.float32 and tuple(view.shape) == shape and view.is_contiguous()
            assert view.data_ptr() == base                                          # packed in problem order
            base += 4 * shape[0] * shape[1]
            alone = S.intention_maps([p['robots']], shape, p['encoding'], scale, p['thickness'])
            assert np.array_equal(bits(view), bits(alone[0])) and np.array_equal(bits(view), bits(fx['maps'][k])), (scale, p['tag'])
            n += 1
        # out=: a flat tensor with room to spare; the views lie in it and the rest keeps its fill
        total = sum(r * c for r, c in shapes)
        flat = torch.empty(total + 5, dtype=torch.int32, device='cuda').fill_(SENT).view(torch.float32)
        again = S.intention_maps([p['robots'] for p in probs], shapes, [p['encoding'] for p in probs], scale, [p['thickness'] for p in probs], out=flat)
        assert again[0].data_ptr() == flat.data_ptr() and (flat.view(torch.int32)[total:] == SENT).all()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again, views))
    assert n == len(both)
    # one shape, a list of thicknesses: the [P, rows, cols] tensor
    fx = fixtures[0]
    ks = [k for k, p in enumerate(fx['problems']) if p['scale'] == fx['problems'][0]['scale']]
    assert len({fx['problems'][k]['thickness'] for k in ks}) > 1
    _lib.lib.c.simq_launch_counts_reset()
    stacked = S.intention_maps([fx['problems'][k]['robots'] for k in ks], fx['shape'], [fx['problems'][k]['encoding'] for k in ks],
                               fx['problems'][0]['scale'], [fx['problems'][k]['thickness'] for k in ks])
    assert _lib.launch_counts() == {'intention_maps_shapes': 1}
    assert isinstance(stacked, torch.Tensor) and tuple(stacked.shape) == (len(ks),) + fx['shape']
    assert np.array_equal(bits(stacked), bits(fx['maps'][ks]))
    bank = torch.full((len(ks) + 1,) + fx['shape'], 7.0, device='cuda')
    into = S.intention_maps([fx['problems'][k]['robots'] for k in ks], fx['shape'], [fx['problems'][k]['encoding'] for k in ks],
                            fx['problems'][0]['scale'], [fx['problems'][k]['thickness'] for k in ks], out=bank[1:])
    assert into.data_ptr() == bank[1].data_ptr() and np.array_equal(bits(bank[1:]), bits(fx['maps'][ks])) and bool((bank[0] == 7.0).all())
    # a single pair and a single thickness make the call they made
    _lib.lib.c.simq_launch_counts_reset()
    S.intention_maps([fx['problems'][0]['robots']], fx['shape'], fx['problems'][0]['encoding'])
    assert _lib.launch_counts() == {'intention_maps': 1}


def store(r0, c0, r1, c1, value=1.0, drop_last=0):
    return (r0, c0, r1, c1, STORE, drop_last, value, 0.0, 0.0, 0.0)


def ramp(r0, c0, r1, c1, start, stop, drop_last=0):
    n = max(abs(r1 - r0), abs(c1 - c0))
    return (r0, c0, r1, c1, RAMP, drop_last, 0.0, start, stop, (stop - start) / n if n else 0.0)


def edge_problems():
    """The tile (32 x 256) and halo edges at the smallest shapes that have them."""
    return [
        {'shape': (1, 1), 'radius': 0, 'segments': [store(0, 0, 0, 0)]},
        {'shape': (1, 1), 'radius': 8, 'segments': [store(0, 0, 0, 0, 0.75)]},
        # the second column tile holds one column; the dilation crosses columns 255 | 256
        {'shape': (1, 257), 'radius': 0, 'segments': [store(0, 0, 0, 256)]},
        {'shape': (8, 9), 'radius': 2, 'segments': []},                                # no segments, between two that have some
        {'shape': (1, 257), 'radius': 3, 'segments': [store(0, 0, 0, 256, 0.5), store(0, 255, 0, 255, 1.0)]},
        # the second row tile holds one row; the halo crosses rows 31 | 32
        {'shape': (33, 5), 'radius': 8, 'segments': [store(0, 2, 32, 2, 0.25), store(31, 0, 31, 0, 1.0)]},
        # 3 x 3 tiles: a ramp over the diagonal without its last point, a stored line across it
        {'shape': (65, 513), 'radius': 2, 'segments': [ramp(0, 0, 64, 512, 1.0, 0.125, drop_last=1), store(64, 0, 0, 512, 0.5)]},
        # one segment range drawn by two problems of one shape with two radii
        {'shape': (40, 33), 'radius': 0, 'segments': [ramp(39, 1, 2, 32, 0.9, -0.2), store(20, 0, 20, 32, 0.125)]},
        {'shape': (40, 33), 'radius': 2, 'share': 7},
    ]


def draw(segs, shape, radius):
    """oracle.draw for maps with a side shorter than the radius too (oracle.dilate slices by the radius and needs both sides to be at
    least as long): the undilated map inside a frame of `radius` zeros, dilated there, the frame cut off again.  Pixels outside the map
    take no part in the reference's dilation; on a non-negative map zeros take no part in a maximum either."""
    plain = oracle.draw(segs, shape, 0)
    if radius == 0:
        return plain
    framed = np.zeros((shape[0] + 2 * radius, shape[1] + 2 * radius), np.float32)
    framed[radius:-radius, radius:-radius] = plain
    out = np.ascontiguousarray(oracle.dilate(framed, radius)[radius:-radius, radius:-radius])
    if min(shape) >= radius:
        assert np.array_equal(bits(out), bits(oracle.draw(segs, shape, radius)))
    return out


def wanted(problems):
    return [draw(problems[p.get('share', k)]['segments'], p['shape'], p['radius']) for k, p in enumerate(problems)]


def test_tile_and_halo_edges_in_one_launch():
    problems = edge_problems()
    want = wanted(problems)
    got, offsets, log, prefix = launch(problems)
    assert log == {'intention_maps_shapes': 1}
    check(problems, want, got, offsets, 'edges')
    assert prefix.tolist() == [0, 1, 2, 4, 5, 7, 9, 18, 20, 22]
    # what the cases are there for did happen
    assert bits(want[1]).tolist() == [[np.float32(0.75).view(np.int32)]] and not want[3].any()
    assert want[4][0, 252:].tolist() == [1.0] * 5 and want[4][0, 251] == 0.5        # the point at column 255 reaches 252 .. 256 (and beyond the map)
    assert (want[5][23:33, 0] == 1.0).all() and (want[5][:23, 0] == 0.25).all()      # the point of row 31 reaches rows 23 .. 32, across 31 | 32
    assert oracle.draw(problems[6]['segments'], (65, 513), 0)[64, 512] == 0        # drop_last: the diagonal's end is not drawn
    assert 0 < want[6][64, 512] < 0.5                                               # ... and is reached by the dilation of its neighbours
    assert (want[8] != 0).sum() > (want[7] != 0).sum() > 0


def test_maps_land_where_their_offsets_say_and_nowhere_else():
    """The offsets are a permutation of the problem order (problem 0 writes the last range), with gaps of 1 and of 7 floats between
    ranges and a tail: every gap and the tail keep the fill, every map is written fully."""
    problems = edge_problems()
    want = wanted(problems)
    cells = [p['shape'][0] * p['shape'][1] for p in problems]
    order = [4, 8, 2, 6, 1, 7, 3, 5, 0]                                               # the problems in the order of their places
    offsets, at = [None] * len(problems), 3
    for slot, p in enumerate(order):
        offsets[p] = at
        at += cells[p] + (1, 7, 0)[slot % 3]
    assert offsets[0] == max(offsets) and sorted(offsets) != offsets
    got, offsets, log, _ = launch(problems, offsets, at + 11)
    assert log == {'intention_maps_shapes': 1}
    check(problems, want, got, offsets, 'placement')
    assert (got[:3] == SENT).all() and (got[offsets[0] + cells[0]:] == SENT).all() and got.size == offsets[0] + cells[0] + 11
    gaps = sorted(b - (a + cells[p]) for (a, p), (b, _) in zip(sorted(zip(offsets, range(9))), sorted(zip(offsets, range(9)))[1:]))
    assert gaps == [0, 0, 1, 1, 1, 7, 7, 7]


def test_a_large_map_beside_a_small_one_launches_the_sum_of_their_tiles():
    problems = [{'shape': (300, 700), 'radius': 8, 'segments': [ramp(299, 0, 0, 699, 1.0, 0.0), store(150, 0, 150, 699, 0.25), store(0, 0, 0, 0, 1.0)]},
                {'shape': (2, 2), 'radius': 8, 'segments': [store(1, 1, 1, 1, 0.5)]}]
    got, offsets, log, prefix = launch(problems)
    assert log == {'intention_maps_shapes': 1}
    check(problems, wanted(problems), got, offsets, 'large and small')
    # the grid is the last entry of the prefix the launch was made from: 10 x 3 tiles and 1, not 2 x 30
    assert tiles((300, 700)) == 30 and tiles((2, 2)) == 1 and prefix.tolist() == [0, 30, 31]


def test_views_of_a_mixed_call_chain_into_local_state_images(S, fixtures):
    """The views handed over as they are: the 96 x 96 local images of both fixtures from one state launch equal the reference's."""
    from simq import _lib
    both = interleaved(fixtures)
    maps, poses, want = [], [], []
    for scale in sorted({fx['problems'][k]['scale'] for fx, k in both}):
        mine = [(fx, k) for fx, k in both if fx['problems'][k]['scale'] == scale]
        probs = [fx['problems'][k] for fx, k in mine]
        maps += S.intention_maps([p['robots'] for p in probs], [fx['shape'] for fx, _ in mine], [p['encoding'] for p in probs], scale,
                                 [p['thickness'] for p in probs])
        poses += [(p['position'], p['heading']) for p in probs]
        want += [fx['local'][k] for fx, k in mine]
    _lib.lib.c.simq_launch_counts_reset()
    states = S.local_state_images(maps, [[('map', i)] for i in range(len(maps))], poses)
    assert _lib.launch_counts() == {'local_state': 1} and tuple(states.shape) == (len(both), 96, 96, 1)
    for i in range(len(both)):
        assert np.array_equal(bits(states[i, :, :, 0]), bits(want[i])), i
    assert any(w.any() for w in want)


def test_each_validation_rule_raises_and_launches_nothing(S, fixtures):
    """On real device buffers, one field corrupted at a time: SimqError, the launch log stays empty, d_out keeps its fill."""
    from simq import _lib, intention_drawing as im
    SimqError = _lib.SimqError
    problems = edge_problems()[:8]
    segs, ranges = [], []
    for p in problems:
        ranges.append((len(segs), len(p['segments'])))
        segs += [im.Segment(start, stop, step, r0, c0, r1, c1, mode, drop_last, value, 0)
                 for r0, c0, r1, c1, mode, drop_last, value, start, stop, step in p['segments']]
    cells = [p['shape'][0] * p['shape'][1] for p in problems]
    offsets = (np.cumsum(cells) - cells).tolist()
    total, n = sum(cells), len(problems)
    c_segs = (im.Segment * len(segs))(*segs)
    c_probs = (im.ShapedProblem * n)(*[im.ShapedProblem(o, p['shape'][0], p['shape'][1], b, c, p['radius'], 0)
                                       for o, p, (b, c) in zip(offsets, problems, ranges)])
    need = _lib.lib.c.simq_intention_shapes_desc_bytes(len(segs), n)
    desc = torch.zeros(need, dtype=torch.uint8, device='cuda')
    out = torch.empty(total + need // 4, dtype=torch.int32, device='cuda').fill_(SENT)
    args = (c_segs, len(segs), c_probs, n, _lib.ptr(desc), ctypes.c_int64(need), _lib.ptr(out), ctypes.c_int64(total), _lib.stream_ptr())
    SEGS, N_SEGS, PROBS, N, DESC, DESC_BYTES, OUT, OUT_FLOATS = range(8)

    def refused(match, edit):
        a = list(args)
        for k in (SEGS, PROBS):
            a[k] = copy.deepcopy(a[k])
        edit(a)
        _lib.lib.c.simq_launch_counts_reset()
        with pytest.raises(SimqError, match=match):
            _lib.lib.call('simq_intention_maps_shapes', *a)
        torch.cuda.synchronize()
        assert _lib.launch_counts() == {} and bool((out == SENT).all())

    def field(index, item, name, value):
        def edit(a):
            setattr(a[index][item], name, value)
        return edit

    def arg(index, value):
        def edit(a):
            a[index] = value
        return edit

    is_ramp = next(i for i, s in enumerate(segs) if s.mode == RAMP)
    is_store = next(i for i, s in enumerate(segs) if s.mode == STORE)
    refused('n = 0', arg(N, 0))
    refused(r'n = 1048577 \(1 \.\. 2\^20 problems\)', arg(N, (1 << 20) + 1))
    refused('n_segments = -1', arg(N_SEGS, -1))
    refused('problem 3: a map of 0 x 9', field(PROBS, 3, 'rows', 0))
    refused(r'problem 3: a map of 16384 x 16384 \(rows, cols >= 1, rows \* cols < 2\^28\)',
            lambda a: (setattr(a[PROBS][3], 'rows', 1 << 14), setattr(a[PROBS][3], 'cols', 1 << 14)))
    refused('problem 1: radius = -1', field(PROBS, 1, 'radius', -1))
    refused('problem 6: radius = 9', field(PROBS, 6, 'radius', 9))
    refused(r'problem 5: segment %d: \(0, 2\) -> \(33, 2\) leaves the 33 x 5 map' % ranges[5][0], field(SEGS, ranges[5][0], 'r1', 33))
    refused(r'problem 2: segment %d: \(0, 0\) -> \(0, 257\) leaves the 1 x 257 map' % ranges[2][0], field(SEGS, ranges[2][0], 'c1', 257))
    # a range shared by the 65 x 513 and the 8 x 9 problem: its segments fit the first only, the second is named
    refused('problem 3: segment %d: .* leaves the 8 x 9 map' % ranges[6][0],
            lambda a: (setattr(a[PROBS][3], 'seg_begin', ranges[6][0]), setattr(a[PROBS][3], 'seg_count', 1)))
    refused('problem 7: segments .* outside the %d given' % len(segs), field(PROBS, 7, 'seg_count', ranges[7][1] + 1))
    refused('problem 0: segments .* outside the %d given' % len(segs), field(PROBS, 0, 'seg_begin', -1))
    refused(r'problem 0: floats \[-1, -1 \+ 1\)', field(PROBS, 0, 'out_offset', -1))
    refused(r'problem 7: floats .* lie outside the %d of d_out' % (total - 1), arg(OUT_FLOATS, ctypes.c_int64(total - 1)))
    refused('the maps of problems 0 and 1 overlap in d_out', field(PROBS, 1, 'out_offset', 0))
    refused('the maps of problems 6 and 7 overlap in d_out', field(PROBS, 7, 'out_offset', offsets[7] - 1))
    refused('problem 7: its map at float %d of d_out overlaps d_desc' % offsets[7],
            arg(OUT, ctypes.c_void_p(desc.data_ptr() - 4 * total + 4)))                              # its last float d_desc's first 4 bytes
    refused('overlaps d_desc', arg(OUT, ctypes.c_void_p(desc.data_ptr() + need - 4)))
    refused('aligned', arg(DESC, ctypes.c_void_p(desc.data_ptr() + 4)))
    refused('aligned', arg(OUT, ctypes.c_void_p(out.data_ptr() + 2)))
    refused('d_desc holds %d bytes' % (need - 1), arg(DESC_BYTES, ctypes.c_int64(need - 1)))
    refused('NULL', arg(OUT, None))
    refused('NULL', arg(DESC, None))
    refused('segment %d: mode 7' % is_store, field(SEGS, is_store, 'mode', 7))
    refused('drop_last = -1', field(SEGS, 1, 'drop_last', -1))
    refused('segment %d: start / stop / step is not finite' % is_ramp, field(SEGS, is_ramp, 'step', float('nan')))
    refused('segment %d: stored value -0' % is_store, field(SEGS, is_store, 'value', -0.0))
    # through the Python interface: a thickness beyond the cap and a wrong out tensor never reach the library
    _lib.lib.c.simq_launch_counts_reset()
    with pytest.raises(ValueError, match='line_thickness = 10'):
        S.intention_maps([[], []], [(8, 9), (4, 4)], 'ramp', line_thickness=[1, 10])
    with pytest.raises(ValueError, match='flat float32 tensor'):
        S.intention_maps([[], []], [(8, 9), (4, 4)], 'ramp', out=torch.empty((2, 8, 9), device='cuda'))
    with pytest.raises(ValueError, match='out must be a contiguous float32 tensor of at least 88 elements on cuda'):
        S.intention_maps([[], []], [(8, 9), (4, 4)], 'ramp', out=torch.empty(88))
    assert _lib.launch_counts() == {}
    # untouched, the same arguments run
    _lib.lib.call('simq_intention_maps_shapes', *args)
    check(problems, wanted(problems), out.cpu().numpy(), offsets, 'after the refusals')
