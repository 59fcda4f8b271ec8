"""GPU: simq_intention_maps / simq.intention_maps against the reference Mapper's own maps (tests/golden/intention_maps_*.npz) and the
numpy oracle (tests/intention_maps_oracle.py), bit for bit (compared as int32 bit patterns), alone and chained into
simq.local_state_images."""
import copy
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import intention_maps_oracle as oracle

pytestmark = pytest.mark.gpu

SENTINEL = 123.0


@pytest.fixture(scope='module')
def simq_mod():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    import simq
    return simq


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def fixtures(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'intention_maps_*.npz')))
    assert len(files) == 2, files
    return [(os.path.basename(f), oracle.load_fixture(f)) for f in files]


def assert_maps_equal(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for p in range(got.shape[0]):
        bad = int((got[p] != want[p]).sum())
        assert bad == 0, '%s: problem %d: %d of %d pixels differ' % (what, p, bad, got[p].size)


def by_settings(problems):
    """Fixture problems grouped by (scale, line thickness), the two arguments one call shares: {settings: [problem index]}."""
    groups = {}
    for k, p in enumerate(problems):
        groups.setdefault((p['scale'], p['thickness']), []).append(k)
    return groups


def test_every_fixture_problem_through_the_python_interface(simq_mod, golden_dir):
    """Each problem in a launch of its own, and all problems of one (scale, thickness) in one launch of mixed encodings."""
    n = 0
    for name, fx in fixtures(golden_dir):
        for k, p in enumerate(fx['problems']):
            got = simq_mod.intention_maps([p['robots']], fx['shape'], p['encoding'], p['scale'], p['thickness'])
            assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + fx['shape'] and got.is_cuda
            assert_maps_equal(got, fx['maps'][k:k + 1], '%s problem %d (%s %s)' % (name, k, p['tag'], p['encoding']))
            one = simq_mod.intention_map(p['robots'], fx['shape'], p['encoding'], p['scale'], p['thickness'])
            assert isinstance(one, np.ndarray) and one.dtype == np.float32 and np.array_equal(bits(one), bits(fx['maps'][k]))
            n += 1
        for (scale, thickness), ks in by_settings(fx['problems']).items():
            got = simq_mod.intention_maps([fx['problems'][k]['robots'] for k in ks], fx['shape'], [fx['problems'][k]['encoding'] for k in ks],
                                          scale, thickness)
            assert_maps_equal(got, fx['maps'][ks], '%s scale %g thickness %d' % (name, scale, thickness))
    assert n >= 40


def c_arrays(im, problems):
    segs, ranges = [], []
    for p in problems:
        ranges.append((len(segs), len(p['segments'])))
        for r0, c0, r1, c1, mode, drop_last, value, start, stop, step in p['segments']:
            segs.append(im.Segment(start, stop, step, r0, c0, r1, c1, mode, drop_last, value, 0))
    return (im.Segment * max(len(segs), 1))(*segs), len(segs), (im.Problem * len(ranges))(*[im.Problem(b, c) for b, c in ranges])


def test_every_fixture_through_the_c_abi_with_the_stored_doubles(simq_mod, golden_dir):
    """The descriptors the fixtures store (pixels, float64 start / stop / step): nothing is computed from positions here.  One launch
    per line thickness; encodings and scales mix in it."""
    from simq import _lib, intention_drawing as im
    for name, fx in fixtures(golden_dir):
        rows, cols = fx['shape']
        for thickness in (1, 2, 3):
            ks = [k for k, p in enumerate(fx['problems']) if p['thickness'] == thickness]
            c_segs, n_segs, c_probs = c_arrays(im, [fx['problems'][k] for k in ks])
            need = _lib.lib.c.simq_intention_desc_bytes(n_segs, len(ks))
            desc = torch.empty(need, dtype=torch.uint8, device='cuda')
            out = torch.full((len(ks), rows, cols), SENTINEL, device='cuda')
            _lib.lib.c.simq_launch_counts_reset()
            _lib.lib.call('simq_intention_maps', c_segs, n_segs, c_probs, len(ks), rows, cols, thickness - 1, _lib.ptr(desc), ctypes.c_int64(need),
                          _lib.ptr(out), ctypes.c_int64(out.numel()), _lib.stream_ptr())
            assert _lib.lib.c.simq_launch_count(b'intention_maps') == 1                  # one launch for all problems
            assert_maps_equal(out, fx['maps'][ks], '%s thickness %d' % (name, thickness))


def random_problems(rng, shape, P):
    """P problems of 0-3 robots with 2-6 waypoints, some beyond the map (clipped to its border), some repeated; mixed encodings."""
    paths, encodings = [], []
    for p in range(P):
        enc = oracle.ENCODINGS[p % 5]
        robots = []
        for _ in range(p % 4):
            if enc == 'circle':
                robots.append((rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 0.0))
                continue
            pts = [(rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 0.0) for _ in range(2 + rng.randint(5))]
            if p % 3 == 0:
                pts.insert(1 + rng.randint(len(pts)), pts[-1] if p % 2 else pts[0])
            robots.append(pts)
        paths.append(robots)
        encodings.append(enc)
    return paths, encodings


def test_mixed_batches_in_one_launch_against_the_oracle(simq_mod):
    """>= 64 problems of mixed encodings per launch, for both room shapes, other shapes that are no multiple of the kernel's tile and
    every line thickness up to the cap."""
    from simq import _lib
    rng = np.random.RandomState(5)
    for shape, P, scale, thickness in (((184, 232), 96, 1.0, 2), ((232, 232), 64, 0.5, 3), ((184, 232), 64, 2.0, 1), ((232, 232), 64, 1.0, 9),
                                       ((33, 300), 64, 0.25, 4), ((70, 513), 64, 1.0, 6), ((1, 1), 5, 1.0, 2), ((257, 31), 64, 1.5, 5)):
        paths, encodings = random_problems(rng, shape, P)
        _lib.lib.c.simq_launch_counts_reset()
        got = simq_mod.intention_maps(paths, shape, encodings, scale, thickness)
        assert _lib.lib.c.simq_launch_count(b'intention_maps') == 1
        want = np.stack([oracle.global_map(r, shape, e, scale, thickness) for r, e in zip(paths, encodings)])
        assert_maps_equal(got, want, 'random %s thickness %d' % (shape, thickness))
        assert want.max() > 0 or shape == (1, 1)


def chain(simq_mod, fx, ks, out=None, maps_out=None):
    """intention_maps -> local_state_images(('map', k)) for the fixture problems ks of one (scale, thickness)."""
    probs = [fx['problems'][k] for k in ks]
    maps = simq_mod.intention_maps([p['robots'] for p in probs], fx['shape'], [p['encoding'] for p in probs], probs[0]['scale'],
                                   probs[0]['thickness'], out=maps_out)
    poses = [(p['position'], p['heading']) for p in probs]
    return maps, simq_mod.local_state_images(maps, [[('map', i)] for i in range(len(ks))], poses, out=out)


def test_maps_chain_into_local_state_images_on_the_device(simq_mod, golden_dir):
    """The [P, rows, cols] tensor handed over as it is (no host copy between the two launches): the 96 x 96 local images equal the
    reference's _get_local_map of its own global maps, the spatial intention channels included."""
    n = 0
    for name, fx in fixtures(golden_dir):
        for (scale, thickness), ks in by_settings(fx['problems']).items():
            maps, states = chain(simq_mod, fx, ks)
            assert maps.is_cuda and tuple(states.shape) == (len(ks), 96, 96, 1)
            for i, k in enumerate(ks):
                assert np.array_equal(bits(states[i, :, :, 0]), bits(fx['local'][k])), (name, k, fx['problems'][k]['tag'])
                n += 1
        assert any(fx['local'][k].any() for k, p in enumerate(fx['problems']) if p['spatial'])
    assert n >= 40


def test_the_chain_writes_into_out_slices_and_overwrites_dirty_memory(simq_mod, golden_dir):
    """Maps into a slice of a larger bank, states into a slice of a ring: only the slices are written.  A second launch of other
    problems into the same, now dirty, slices leaves exactly those problems' maps: the kernel writes every pixel, zeros included."""
    fx = oracle.load_fixture(os.path.join(golden_dir, 'intention_maps_184x232.npz'))
    groups = by_settings(fx['problems'])
    ks = max(groups.values(), key=len)
    assert len(ks) >= 4
    n = len(ks)
    bank = torch.full((n + 3, 184, 232), SENTINEL, device='cuda')
    ring = torch.full((n + 4, 96, 96, 1), SENTINEL, device='cuda')
    maps, states = chain(simq_mod, fx, ks, out=ring[2:2 + n], maps_out=bank[1:1 + n])
    assert maps.data_ptr() == bank[1].data_ptr() and states.data_ptr() == ring[2].data_ptr()
    host_bank, host_ring = bank.cpu().numpy(), ring.cpu().numpy()
    assert np.array_equal(bits(host_bank[1:1 + n]), bits(fx['maps'][ks])) and np.array_equal(bits(host_ring[2:2 + n, :, :, 0]), bits(fx['local'][ks]))
    assert (host_bank[:1] == SENTINEL).all() and (host_bank[1 + n:] == SENTINEL).all()
    assert (host_ring[:2] == SENTINEL).all() and (host_ring[2 + n:] == SENTINEL).all()
    # the same slices again, the problems in reverse order: every pixel a map of the first launch lit and the second does not is 0 again
    back = ks[::-1]
    assert any(((fx['maps'][a] != 0) & (fx['maps'][b] == 0)).any() for a, b in zip(ks, back))
    chain(simq_mod, fx, back, out=ring[2:2 + n], maps_out=bank[1:1 + n])
    assert np.array_equal(bits(bank[1:1 + n]), bits(fx['maps'][back])) and np.array_equal(bits(ring[2:2 + n, :, :, 0]), bits(fx['local'][back]))
    # ... and an environment of idle robots only over a dirty map
    dirty = torch.full((1, 184, 232), SENTINEL, device='cuda')
    simq_mod.intention_maps([[]], (184, 232), 'ramp', out=dirty)
    assert not bool(dirty.any())


def test_each_validation_rule_raises_and_launches_nothing(simq_mod, golden_dir):
    """Through the Python interface what it can break, through the C-ABI on real device buffers the rest, one field corrupted at a
    time: SimqError / status -1, nothing launched, the output keeps its sentinel."""
    from simq import _lib, intention_drawing as im
    SimqError = _lib.SimqError
    fx = oracle.load_fixture(os.path.join(golden_dir, 'intention_maps_184x232.npz'))
    ks = [k for k, p in enumerate(fx['problems']) if p['thickness'] == 2 and p['scale'] == 1.0]
    probs = [fx['problems'][k] for k in ks]
    out = torch.full((len(ks), 184, 232), SENTINEL, device='cuda')
    args, _, keep = im._prepare([p['robots'] for p in probs], (184, 232), [p['encoding'] for p in probs], 1.0, 2, out)
    SEGS, PROBS, ROWS, COLS, RADIUS, DESC, DESC_BYTES, OUT, OUT_FLOATS = 0, 2, 4, 5, 6, 7, 8, 9, 10

    def untouched():
        torch.cuda.synchronize()
        assert _lib.lib.c.simq_launch_count(b'intention_maps') == 0 and bool((out == SENTINEL).all())

    def refused(match, edit):
        a = list(args)
        for k in (SEGS, PROBS):
            a[k] = copy.deepcopy(a[k])
        edit(a)
        _lib.lib.c.simq_launch_counts_reset()
        with pytest.raises(SimqError, match=match):
            _lib.lib.call('simq_intention_maps', *a)
        untouched()

    def field(index, item, name, value):
        def edit(a):
            setattr(a[index][item], name, value)
        return edit

    def arg(index, value):
        def edit(a):
            a[index] = value
        return edit

    ramp = next(i for i in range(args[1]) if args[SEGS][i].mode == im.RAMP)
    store = next(i for i in range(args[1]) if args[SEGS][i].mode == im.STORE)
    refused('leaves the 184 x 232 map', field(SEGS, 3, 'r1', 184))
    refused('leaves the 184 x 232 map', field(SEGS, 0, 'c0', -1))
    refused('leaves the 184 x 231 map', arg(COLS, 231))                                # (an end pixel of the fixtures lies on column 231)
    refused('mode 7', field(SEGS, 1, 'mode', 7))
    refused('drop_last = -1', field(SEGS, 1, 'drop_last', -1))
    refused('not finite', field(SEGS, ramp, 'start', float('nan')))
    refused('not finite', field(SEGS, ramp, 'stop', float('inf')))
    refused('not finite', field(SEGS, ramp, 'step', float('-inf')))
    refused('stored value', field(SEGS, store, 'value', -1.0))
    refused('stored value', field(SEGS, store, 'value', -0.0))
    refused('stored value', field(SEGS, store, 'value', float('nan')))
    refused('outside the %d given' % args[1], field(PROBS, 0, 'seg_count', args[1] + 1))
    refused('outside the %d given' % args[1], field(PROBS, 2, 'seg_begin', -1))
    refused('radius = 9', arg(RADIUS, 9))
    refused('radius = -1', arg(RADIUS, -1))
    refused('rows \\* cols < 2\\^28', arg(ROWS, 0))
    refused('d_out holds', arg(OUT_FLOATS, ctypes.c_int64(args[OUT_FLOATS].value - 1)))
    refused('d_desc holds', arg(DESC_BYTES, ctypes.c_int64(args[DESC_BYTES].value - 8)))
    refused('aligned', arg(DESC, ctypes.c_void_p(args[DESC].value + 4)))
    refused('aligned', arg(OUT, ctypes.c_void_p(args[OUT].value + 2)))
    refused('overlaps d_desc', arg(OUT, ctypes.c_void_p(args[DESC].value)))
    refused('NULL', arg(OUT, None))
    # through the Python interface: a thickness beyond the cap never reaches the library, a wrong out tensor neither
    _lib.lib.c.simq_launch_counts_reset()
    with pytest.raises(ValueError, match='line_thickness'):
        simq_mod.intention_maps([probs[0]['robots']], (184, 232), probs[0]['encoding'], line_thickness=10, out=out[:1])
    with pytest.raises(ValueError, match='out'):
        simq_mod.intention_maps([probs[0]['robots']], (184, 232), probs[0]['encoding'], out=out[:2])
    with pytest.raises(ValueError, match='out'):
        simq_mod.intention_maps([probs[0]['robots']], (184, 232), probs[0]['encoding'], out=out[:1].cpu())
    untouched()
    # untouched, the same arguments run
    _lib.lib.call('simq_intention_maps', *args)
    assert_maps_equal(out, fx['maps'][ks], 'after the refusals')
    del keep
