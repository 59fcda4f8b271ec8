"""CPU: simq_observation_update_sequences is named where an entry must be named; every refusal of its host validation, with fake
device pointers (nothing is dereferenced before the checks pass, and here nothing passes them); the bookkeeping of
BatchedMapper.defer / pending / reset and the refusal of reads while frames are pending, without a device; and the yardstick of the GPU
test -- the numpy oracle applied frame by frame -- on the reference's own three successive updates."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import mapper_oracle
import observation_maps_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ('observation_maps_184x232.npz', 'observation_maps_232x232.npz')
F = np.float32
ENTRY = 'simq_observation_update_sequences'


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_the_entry_is_named_in_the_header_the_export_list_and_the_ctypes_table(L):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'simq.h')).read(), flags=re.S)
    assert re.search(r'\bint %s\s*\(' % ENTRY, header) and re.search(r'#define SIMQ_OBSERVATION_MAX_SEQUENCE 1023\b', header)
    assert hasattr(ctypes.CDLL(L.LIB_PATH), ENTRY)                  # csrc/libsimq.map lets simq_* through
    assert ENTRY in L.EXPORTS and len(L._SIGS[ENTRY][1]) == 14
    declared = re.search(r'\bint %s\s*\((.*?)\)\s*;' % ENTRY, header, flags=re.S).group(1)
    assert len(declared.split(',')) == 14
    from simq import observation
    assert observation.MAX_SEQUENCE == 1023 and observation.MAX_POINTS == 1 << 22
    import simq
    assert simq.observation_update_sequences is observation.observation_update_sequences


def test_every_host_refusal_of_the_c_entry(L):
    import torch
    from simq.observation import ObservationProblem
    H = W = 4
    rows = cols = 8
    cells = rows * cols

    def frame(**kw):
        p = ObservationProblem()
        p.depth_offset, p.ids_offset, p.px_offset, p.py_offset = 0, 16, 32, 36
        p.far_near, p.far, p.far_minus_near = 1, 10, 9.9
        p.height, p.width, p.rows, p.cols = H, W, rows, cols
        p.occupancy_offset = p.overhead_offset = 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    second = dict(overhead_offset=cells, occupancy_offset=cells)   # a second pair of maps right behind the first
    # fake, well-separated, aligned device addresses
    base = dict(frames=0x10000, probs_dev=0x20000, begin_dev=0x28000, over=0x30000, occ=0x40000, status=0x50000, words=40, floats=4 * cells,
                nbytes=4 * cells)

    def call(ps, begin, **kw):
        a = dict(base, **kw)
        arr = (ObservationProblem * len(ps))(*ps)
        table = (ctypes.c_int32 * len(begin))(*begin)
        rc = L.lib.c.simq_observation_update_sequences(ctypes.c_void_p(a['frames']), a['words'], arr, a.get('n_frames', len(ps)), table,
                                                       a.get('n_sequences', len(begin) - 1), ctypes.c_void_p(a['probs_dev']), ctypes.c_void_p(a['begin_dev']),
                                                       ctypes.c_void_p(a['over']), a['floats'], ctypes.c_void_p(a['occ']), a['nbytes'],
                                                       ctypes.c_void_p(a['status']), None)
        return rc, L.last_error()

    def refused(word, ps, begin, **kw):
        rc, msg = call(ps, begin, **kw)
        assert rc == -1 and word in msg and msg.startswith('observation_update_sequences:'), (word, rc, msg)

    def accepted(ps, begin, **kw):
        """Every host check passes: the call then reaches the device (none here: it fails in the copy of the descriptors, not in a
        check).  With a device the fake addresses must not get that far, and the GPU test covers what is accepted."""
        if not torch.cuda.is_available():
            rc, msg = call(ps, begin, **kw)
            assert rc == -2 and 'upload_descriptors' in msg, (rc, msg)

    over, occ = base['over'], base['occ']
    three = [frame(), frame(), frame(**second)]
    # the table
    refused('begin rises from 0', three, [1, 2, 3])
    refused('begin rises from 0', three, [0, 2, 2], n_sequences=2, n_frames=3)
    refused('every sequence has a frame', three, [0, 2, 2, 3])                              # an empty sequence
    refused('every sequence has a frame', three, [0, 3, 2, 3])                              # begin falling
    refused('no sequence is empty', three, [0, 1, 2, 3, 3], n_sequences=4)
    refused('n_frames = 0', three, [0, 0], n_frames=0)
    refused('at most 1023 frames per sequence', [frame()] * 1024, [0, 1024])
    refused('at most 1023 frames per sequence', [frame()] * 1024 + [frame(**second)], [0, 1024, 1025])
    # what simq_observation_update checks per problem, per frame -- here in the second frame of a sequence
    for kw, word in ((dict(height=0), 'frame 1: a frame of'), (dict(rows=0), 'frame 1: maps of'), (dict(rows=1 << 24, cols=1), 'frame 1: maps of'),
                     (dict(depth_offset=25), 'frame 1: depth words'), (dict(ids_offset=-1), 'frame 1: id words'), (dict(px_offset=37), 'frame 1: px words'),
                     (dict(py_offset=37), 'frame 1: px words'), (dict(overhead_offset=4 * cells - 63), 'frame 1: overhead floats'),
                     (dict(occupancy_offset=4 * cells - 63), 'frame 1: occupancy bytes'), (dict(far=float('nan')), 'frame 1: a camera vector'),
                     (dict(has_receptacle=2), 'frame 1: has_receptacle')):
        refused(word, [frame(), frame(**kw)], [0, 2])
    # the frames of a sequence agree on the four map fields
    for kw, word in ((dict(overhead_offset=cells), 'names overhead_offset 64, frame 0 names 0'), (dict(occupancy_offset=cells), 'names occupancy_offset 64'),
                     (dict(rows=7), 'names rows 7, frame 0 names 8'), (dict(cols=7), 'names cols 7, frame 0 names 8')):
        refused('sequence 0: frame 2 ' + word, [frame(), frame(), frame(**kw)], [0, 3])
    refused('sequence 1: frame 2 names rows 7, frame 1 names 8', [frame(), frame(**second), frame(rows=7, **second)], [0, 1, 3])
    # frames of one sequence that differ in everything else are accepted: another camera, other id ranges
    accepted([frame(), frame(height=2, width=3, min_cube=5, receptacle=3, has_receptacle=1)], [0, 2])
    # two sequences one byte apart are accepted, sharing one byte they are refused -- of the occupancy maps, of the overhead maps
    accepted([frame(), frame(overhead_offset=cells, occupancy_offset=cells)], [0, 1, 2])
    refused('share memory', [frame(), frame(overhead_offset=cells, occupancy_offset=cells - 1)], [0, 1, 2])
    refused('share memory', [frame(), frame(overhead_offset=cells - 1, occupancy_offset=cells)], [0, 1, 2])
    refused('share memory', [frame(), frame()], [0, 1, 2])                                  # the frames of one map belong in one sequence
    accepted([frame(), frame()], [0, 2])
    refused('share memory', [frame()], [0, 1], occ=over + 16)                               # the occupancy map inside the overhead map
    # a map overlapping each of the other buffers, and those each other
    for kw, word in ((dict(frames=over + 4 * cells - 4), 'a map overlaps d_frames'), (dict(frames=occ - 4 * 40 + 4), 'a map overlaps d_frames'),
                     (dict(probs_dev=over + 8), 'a map overlaps d_problems'), (dict(probs_dev=occ + 8), 'a map overlaps d_problems'),
                     (dict(begin_dev=over + 4 * cells - 4), 'a map overlaps d_begin'), (dict(begin_dev=occ + cells - 4), 'a map overlaps d_begin'),
                     (dict(status=over + 4 * cells - 4), 'a map overlaps d_status'), (dict(status=occ + 8), 'a map overlaps d_status'),
                     (dict(status=base['begin_dev'] + 4), 'd_begin overlaps d_status'), (dict(begin_dev=base['probs_dev'] + 8), 'd_problems overlaps d_begin'),
                     (dict(status=base['frames'] + 8), 'd_frames overlaps d_status')):
        refused(word, [frame()], [0, 1], **kw)
    accepted([frame()], [0, 1], frames=over + 4 * cells, status=occ + cells)                # right behind a map is not inside it
    # alignment, NULL
    for kw in (dict(over=over + 2), dict(frames=base['frames'] + 1), dict(probs_dev=base['probs_dev'] + 4), dict(begin_dev=base['begin_dev'] + 2),
               dict(status=base['status'] + 2)):
        refused('aligned', [frame()], [0, 1], **kw)
    for name in ('frames', 'probs_dev', 'begin_dev', 'over', 'occ', 'status'):
        refused('NULL', [frame()], [0, 1], **{name: 0})
    assert L.lib.c.simq_observation_update_sequences(None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None, None) != 0 and 'NULL' in L.last_error()
    # the single-frame entry is what it was: two problems naming one map
    arr = (ObservationProblem * 2)(frame(), frame())
    assert L.lib.c.simq_observation_update(ctypes.c_void_p(base['frames']), 40, arr, 2, ctypes.c_void_p(base['probs_dev']), ctypes.c_void_p(over), 4 * cells,
                                           ctypes.c_void_p(occ), 4 * cells, ctypes.c_void_p(base['status']), None) == -1
    assert 'observation_update: two maps of one launch share memory' in L.last_error() and 'the order of two updates of one map matters' in L.last_error()


def test_the_wrapper_orders_frames_by_map_and_splits_at_the_cap(L):
    from simq import observation as ob
    launches = ob.sequence_launches([2, 0, 2, 1, 0, 2])
    assert len(launches) == 1 and launches[0][0].tolist() == [1, 4, 3, 0, 2, 5] and launches[0][1].tolist() == [0, 2, 3, 6] and launches[0][1].dtype == np.int32
    index = [0] * 1030 + [1] * 3
    index = index[:500] + [1] + index[500:]                         # map 1 once in between
    launches = ob.sequence_launches(index)
    assert [len(f) for f, _ in launches] == [1023 + 4, 7] and launches[0][1].tolist() == [0, 1023, 1027] and launches[1][1].tolist() == [0, 7]
    zeros = [k for k, m in enumerate(index) if m == 0]
    assert launches[0][0].tolist()[:1023] == zeros[:1023] and launches[1][0].tolist() == zeros[1023:]
    assert launches[0][0].tolist()[1023:] == [500, 1031, 1032, 1033]
    # the argument checks need no device
    g = ob.camera_geometry((0.1, 0.2, 1), (0.1, 0.2, 0), (1, 0, 0), 0.1, 10, 1, 4)
    r = ob.IdRanges(3, 9, None, 11, 20)
    depth, ids = np.zeros((4, 4), F), np.zeros((4, 4), np.int32)
    for args in (([depth.astype(np.float64)], [ids], g, r, [], [], [0]), ([depth], [ids, ids], g, r, [], [], [0]), ([depth], [ids], [g, g], r, [], [], [0]),
                 ([depth, depth], [ids, ids], g, r, [], [], [0]), ([depth], [ids], g, r, [], [], 0)):
        with pytest.raises(ValueError):
            ob.observation_update_sequences(*args)


def build(golden_dir, **kw):
    from simq import mapper
    fx = mapper_oracle.load_fixture(sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))[0])
    masks = {name: fx['masks'][k] for k, name in enumerate(fx['mask_names'])}
    return mapper.BatchedMapper([fx['room_width']] * 2, [fx['room_length']] * 2, [fx['types']] * 2, masks, [fx['groups']] * 2,
                                [fx['receptacle_position']] * 2, **kw), fx


def test_defer_pending_and_reset_bookkeeping_and_the_refusal_of_reads_without_a_device(golden_dir, L):
    import torch
    from simq import mapper, observation as ob
    from simq._lib import SimqError
    bm, fx = build(golden_dir, use_shortest_path_map=True)
    assert bm.num_mappers == 6 and bm.pending.tolist() == [0] * 6 and bm.pending.dtype == np.int64
    fr = fx['rounds'][0]['frames']
    depth, ids = [f['depth'].copy() for f in fr], [f['ids'].copy() for f in fr]
    geoms, ranges = [ob.CameraGeometry(*f['geometry']) for f in fr], [ob.IdRanges(*f['ranges']) for f in fr]
    # the checks of update's arguments
    with pytest.raises(ValueError, match='distinct mappers'):
        bm.defer(depth, ids, geoms, ranges, mappers=[1, 1, 2])
    with pytest.raises(ValueError, match='3 frames for 2 mappers'):
        bm.defer(depth, ids, geoms, ranges, mappers=[1, 2])
    with pytest.raises(ValueError, match='depth'):
        bm.defer([d.astype(np.float64) for d in depth], ids, geoms, ranges, mappers=[0, 1, 2])
    with pytest.raises(ValueError, match='ids'):
        bm.defer(depth, [i.astype(np.int64) for i in ids], geoms, ranges, mappers=[0, 1, 2])
    with pytest.raises(ValueError, match='as many id frames'):
        bm.defer(depth, ids[:2], geoms, ranges, mappers=[0, 1, 2])
    with pytest.raises(ValueError, match='geometry is for'):
        bm.defer([depth[0][:5]], [ids[0][:5]], geoms[0], ranges[0], mappers=[4])
    with pytest.raises(ValueError, match='geometries'):
        bm.defer(depth, ids, geoms[:2], ranges, mappers=[0, 1, 2])
    assert bm.pending.tolist() == [0] * 6 and bm._staging.used in ([], [0])
    # frames wait in capture order, in memory of the object
    bm.defer(depth, ids, geoms, ranges, mappers=[3, 4, 5])
    bm.defer(depth[:2], ids[:2], geoms[:2], ranges[:2], mappers=[4, 0])
    bm.defer([depth[2]], [ids[2]], geoms[2], ranges[2], mappers=[4])
    assert bm.pending.tolist() == [1, 0, 0, 1, 3, 1]
    want = [(f['depth'].copy(), f['ids'].copy()) for f in fr]
    for d, i in zip(depth, ids):                                    # the caller's arrays are the caller's again
        d.fill(np.nan)
        i.fill(-1)

    def held(m, k):
        f = bm._pending[m][k]
        q, room = f.problem, bm._staging.arrays[f.block][f.at:f.at + f.words]
        n = q.height * q.width
        assert (q.px_offset, q.py_offset, q.depth_offset, q.ids_offset, f.words) == (0, q.width, q.width + q.height, q.width + q.height + n, q.width + q.height + 2 * n)
        assert (q.rows, q.cols) == bm.shapes[m] and q.overhead_offset == q.occupancy_offset == m * bm.shapes[m][0] * bm.shapes[m][1]
        return room[q.depth_offset:q.depth_offset + n].view(F).reshape(q.height, q.width), room[q.ids_offset:q.ids_offset + n].reshape(q.height, q.width), \
            room[:q.width].view(F), room[q.width:q.width + q.height].view(F)

    for (m, k), src in {(3, 0): 0, (4, 0): 1, (5, 0): 2, (4, 1): 0, (0, 0): 1, (4, 2): 2}.items():
        d, i, px, py = held(m, k)
        assert np.array_equal(d.view(np.int32), want[src][0].view(np.int32)) and np.array_equal(i, want[src][1]), (m, k)
        assert np.array_equal(px, geoms[src].pixel_x) and np.array_equal(py, geoms[src].pixel_y)
    assert bm._staging.tensors[0].is_pinned() == torch.cuda.is_available()
    # reads of a mapper whose frames wait are refused, before anything else and without a device
    robots = [[mapper.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'], r['history_path'])
               for r in fx['rounds'][0]['robots']]] * 2
    for call, who in ((lambda: bm.update(depth, ids, geoms, ranges, mappers=[3, 4, 5]), r'update: mapper\(s\) 3 \(environment 1, robot 0\), 4 \(environment 1, robot 1\), 5'),
                      (lambda: bm.get_states(robots, mappers=[1, 0]), r'get_states: mapper\(s\) 0 \(environment 0, robot 0\) have deferred frames'),
                      (lambda: bm.get_states(mapper.RobotArrays.from_states(bm, robots)), r'get_states: mapper\(s\) 0 .*, 3 .*, 4 .*, 5 '),
                      (lambda: bm.shortest_paths([(0, 0)], [(0.1, 0.1)], mappers=[4]), r'shortest_paths: mapper\(s\) 4 \(environment 1, robot 1\) have deferred frames .*\(\[3\] pending\)'),
                      (lambda: bm.distances_to_receptacle([[(0, 0)]], mappers=[5]), r'distances_to_receptacle: mapper\(s\) 5 ')):
        with pytest.raises(SimqError, match=r'BatchedMapper\.' + who + r'.*flush\(\)'):
            call()
    # reset drops the frames of its environments, and what still waits moves to the front unchanged
    used = list(bm._staging.used)
    try:
        bm.reset([1])
    except SimqError as e:                                          # (without a device the maps cannot be zeroed; the frames are dropped all the same)
        assert not torch.cuda.is_available() and 'need an MI355X' in str(e)
    assert bm.pending.tolist() == [1, 0, 0, 0, 0, 0] and sum(bm._staging.used) == bm._pending[0][0].words < sum(used)
    assert (bm._pending[0][0].block, bm._pending[0][0].at) == (0, 0)
    d, i, _, _ = held(0, 0)
    assert np.array_equal(d.view(np.int32), want[1][0].view(np.int32)) and np.array_equal(i, want[1][1])
    try:
        bm.reset()
    except SimqError:
        assert not torch.cuda.is_available()
    assert bm.pending.tolist() == [0] * 6 and bm._staging.used == [0] * len(bm._staging.tensors)
    if not torch.cuda.is_available():
        bm.defer([want[0][0]], [want[0][1]], geoms[0], ranges[0], mappers=[2])
        with pytest.raises(SimqError, match='need an MI355X'):
            bm.flush()
        assert bm.pending.tolist() == [0, 0, 1, 0, 0, 0]
        bm.flush(mappers=[0, 1])                                    # no frames of theirs wait: nothing to do, no device needed


def test_staging_grows_in_blocks_and_compaction_never_overwrites_a_frame_that_waits():
    from simq.mapper import _Deferred, _Staging
    st = _Staging()
    st.BLOCK_WORDS = 100
    rng = np.random.RandomState(0)
    frames, content = [], {}
    for n in (60, 30, 30, 50, 250, 10, 90, 5):
        b, at = st.take(n)
        f = _Deferred(b, at, n, None)
        content[id(f)] = rng.randint(0, 1 << 30, n).astype(np.int32)
        st.arrays[b][at:at + n] = content[id(f)]
        frames.append(f)
    assert [a.size for a in st.arrays] == [100, 100, 250, 450] and [(f.block, f.at) for f in frames] == [(0, 0), (0, 60), (1, 0), (1, 30), (2, 0), (3, 0), (3, 10), (3, 100)]
    for keep in ([1, 2, 3, 4, 6, 7], [2, 4, 7], [7], []):
        waiting = [frames[k] for k in keep]
        st.compact(waiting)
        for f in waiting:
            assert np.array_equal(st.arrays[f.block][f.at:f.at + f.words], content[id(f)])
        spans = sorted((f.block, f.at, f.at + f.words) for f in waiting)
        assert all(a[0] != b[0] or a[2] <= b[1] for a, b in zip(spans, spans[1:])) and sum(st.used) == sum(f.words for f in waiting)
    assert st.used == [0, 0, 0, 0] and st.take(100) == (0, 0) and len(st.tensors) == 4


@pytest.mark.parametrize('fname', FILES)
def test_the_sequence_oracle_equals_the_references_three_successive_updates(golden_dir, fname):
    """The yardstick of tests/test_gpu_observation_sequences.py: the oracle applied frame by frame, a frame with a point that is not
    finite skipped, on the maps the reference's Mapper started from gives the maps it ended with."""
    top, cases = oracle.load_fixture(os.path.join(golden_dir, fname))
    rec = dict(cases)
    steps = [rec['successive_step%d' % k] for k in range(3)]
    over, occ = steps[0]['overhead_before'].copy(), steps[0]['occupancy_before'].copy()
    bad = steps[1]['depth'].copy()
    bad[3, 3] = np.nan
    status = []
    for k, s in enumerate(steps):
        if k == 1:                                                  # a skipped frame in between changes nothing
            before = over.copy(), occ.copy()
            status.append(oracle.update(over, occ, bad, s['ids'], s['geometry'], s['ranges']))
            assert np.array_equal(over.view(np.int32), before[0].view(np.int32)) and np.array_equal(occ, before[1])
        status.append(oracle.update(over, occ, s['depth'], s['ids'], s['geometry'], s['ranges']))
        _, ambiguous, _ = oracle.tied_pixels(over.shape, s['depth'], s['ids'], s['geometry'], s['ranges'])
        assert not ambiguous.any()
        assert np.array_equal(over.view(np.int32), s['overhead_after'].view(np.int32)) and np.array_equal(occ, s['occupancy_after'])
    assert status == [0, 1, 0, 0]
