"""CPU: what intention maps of several room shapes and thicknesses in one launch check before they need a
device -- the three places the two new entry points are named, the size of the descriptor scratch, every host refusal of
simq_intention_maps_shapes at its edge (fake device pointers, never dereferenced: one value inside, one outside), and the argument
checks of simq.intention_maps for lists of shapes and thicknesses.

d_out and d_desc are aligned to their elements, so they cannot share exactly one byte: the edges below are one ELEMENT shared
(refused) against none (accepted)."""
import ctypes
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('simq_intention_maps_shapes', 'simq_intention_shapes_desc_bytes')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def test_new_entry_points_are_named_in_the_header_the_map_file_and_the_ctypes_table(L):
    from simq import intention_drawing as im
    text = open(os.path.join(ROOT, 'include', 'simq.h')).read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    version_script = open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'libsimq.map')).read()
    exported = re.search(r'global:\s*([^;]+);', version_script).group(1).split()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        proto = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, header)
        assert proto, '%s is not declared in include/simq.h' % name
        assert any(fnmatch.fnmatchcase(name, pattern) for pattern in exported), (name, exported)
        assert hasattr(raw, name), 'libsimq.so does not export %s' % name
        assert name in L.EXPORTS and len(L._SIGS[name][1]) == proto.group(1).count(',') + 1, name
    assert len(L._SIGS['simq_intention_maps_shapes'][1]) == 9 and len(L._SIGS['simq_intention_shapes_desc_bytes'][1]) == 2
    assert '"intention_maps_shapes"' in text and 'typedef struct simq_intention_shaped_problem' in header
    # the structure as the header lays it out: a multiple of 8 bytes, like its neighbours
    layout = lambda cls: [(f, getattr(cls, f).offset) for f, _ in cls._fields_]
    assert im.ShapedProblem is L.IntentionShapedProblem and ctypes.sizeof(im.ShapedProblem) == 32 == im.SHAPED_PROBLEM.itemsize
    assert layout(im.ShapedProblem) == [('out_offset', 0), ('rows', 8), ('cols', 12), ('seg_begin', 16), ('seg_count', 20), ('radius', 24),
                                        ('reserved_', 28)]
    fields = re.search(r'typedef struct simq_intention_shaped_problem \{(.*?)\}', header, flags=re.S).group(1)
    assert re.findall(r'\b(out_offset|rows|cols|seg_begin|seg_count|radius|reserved_)\b', fields) == [f for f, _ in im.ShapedProblem._fields_]


def test_desc_bytes_grow_with_both_counts_and_hold_the_tile_prefix(L):
    c = L.lib.c
    size = c.simq_intention_shapes_desc_bytes
    # segments of 56 bytes, problems of 32, the prefix of tile counts: int32 [n + 1] padded to 8 bytes
    for n_segs, n in ((0, 1), (5, 7), (5, 8), (1, 1 << 20), (1 << 24, 3)):
        assert size(n_segs, n) == 56 * n_segs + 32 * n + (4 * (n + 1) + 7) // 8 * 8, (n_segs, n)
        assert size(n_segs, n) >= c.simq_intention_desc_bytes(n_segs, n) + 4 * (n + 1)          # the old size plus the prefix table
        assert size(n_segs, n) % 8 == 0
        assert size(n_segs + 1, n) > size(n_segs, n) and size(n_segs, n + 2) > size(n_segs, n + 1) >= size(n_segs, n)
    assert size(0, 0) == 8
    assert size(-1, 1) == -1 and size(1, -1) == -1 and size(-1, -1) == -1


OUT, DESC = 0x40000000, 0x30000000


def segment(im, **kw):
    return im.Segment(**dict(dict(start=1.0, stop=0.5, step=-0.05, r0=1, c0=2, r1=6, c1=7, mode=im.RAMP, drop_last=0, value=0.0, reserved_=0), **kw))


def problem(im, out_offset=0, rows=8, cols=9, seg_begin=0, seg_count=1, radius=1):
    return im.ShapedProblem(out_offset, rows, cols, seg_begin, seg_count, radius, 0)


def c_call(L, probs=None, segs=None, n=None, n_segs=None, out=OUT, out_floats=1 << 20, desc=DESC, desc_bytes=1 << 20):
    """simq_intention_maps_shapes on fake device pointers: every check runs on the host before the descriptor copy / launch."""
    from simq import intention_drawing as im
    segs = [segment(im)] if segs is None else segs
    probs = [problem(im)] if probs is None else probs
    a_segs = (im.Segment * max(len(segs), 1))(*segs)
    a_probs = (im.ShapedProblem * max(len(probs), 1))(*probs)
    return L.lib.c.simq_intention_maps_shapes(a_segs if segs else None, len(segs) if n_segs is None else n_segs, a_probs,
                                              len(probs) if n is None else n, None if desc is None else ctypes.c_void_p(desc), desc_bytes,
                                              None if out is None else ctypes.c_void_p(out), out_floats, None)


def test_shapes_entry_refuses_bad_tables_before_any_device_call(L):
    from simq import intention_drawing as im

    def refused(word, **kw):
        assert c_call(L, **kw) == -1, kw
        assert word in L.last_error(), (word, L.last_error())

    def accepted(**kw):
        """Every host check passed: without a device the call then fails in the copy of the descriptors, not in a check."""
        if not torch.cuda.is_available():
            assert c_call(L, **kw) == -2, (kw, L.last_error())

    P = lambda **kw: problem(im, **kw)
    accepted()
    refused('NULL', out=None)
    refused('NULL', desc=None)
    # n and n_segments
    refused('n = 0 (1 .. 2^20 problems)', n=0)
    many = np.zeros((1 << 20) + 1, im.SHAPED_PROBLEM)
    many['rows'], many['cols'], many['out_offset'] = 1, 1, np.arange(len(many))

    def call_many(n):
        return L.lib.c.simq_intention_maps_shapes(None, 0, many.ctypes.data_as(ctypes.c_void_p), n, ctypes.c_void_p(DESC), 1 << 30, ctypes.c_void_p(OUT),
                                                  1 << 21, None)
    assert call_many((1 << 20) + 1) == -1 and 'n = 1048577 (1 .. 2^20 problems)' in L.last_error()
    if not torch.cuda.is_available():
        assert call_many(1 << 20) == -2, L.last_error()
    refused('n_segments = -1', n_segs=-1)
    refused('n_segments = %d' % ((1 << 24) + 1), n_segs=(1 << 24) + 1)
    refused('segments NULL', segs=[], n_segs=1, probs=[P(seg_count=0)])
    accepted(segs=[], probs=[P(seg_count=0)])
    # shape
    refused('problem 0: a map of 0 x 9', probs=[P(rows=0, seg_count=0)])
    refused('problem 1: a map of 8 x -2', probs=[P(), P(out_offset=100, cols=-2, seg_count=0)])
    refused('problem 0: a map of 16384 x 16384 (rows, cols >= 1, rows * cols < 2^28)', probs=[P(rows=1 << 14, cols=1 << 14)], out_floats=1 << 29)
    accepted(probs=[P(rows=1 << 14, cols=(1 << 14) - 1)], out_floats=1 << 29)
    # radius
    refused('problem 0: radius = -1', probs=[P(radius=-1)])
    refused('problem 1: radius = 9', probs=[P(), P(out_offset=100, radius=9)])
    accepted(probs=[P(radius=0), P(out_offset=100, radius=8)])
    # a segment end at rows_p / cols_p against rows_p - 1 / cols_p - 1
    refused('problem 0: segment 0: (1, 2) -> (8, 7) leaves the 8 x 9 map', segs=[segment(im, r1=8)])
    refused('problem 0: segment 0: (1, 9) -> (6, 7) leaves the 8 x 9 map', segs=[segment(im, c0=9)])
    refused('leaves the 8 x 9 map', segs=[segment(im, r0=-1)])
    accepted(segs=[segment(im, r1=7, c0=8)])
    # one range shared by a 40 x 33 and an 8 x 9 problem, a segment inside the first only: the second problem is named
    shared = [P(rows=40, cols=33), P(out_offset=2000)]
    refused('problem 1: segment 0: (1, 2) -> (39, 7) leaves the 8 x 9 map', probs=shared, segs=[segment(im, r1=39)])
    refused('problem 1: segment 0: (1, 2) -> (6, 32) leaves the 8 x 9 map', probs=shared, segs=[segment(im, c1=32)])
    refused('problem 1: segment 1', probs=[P(rows=40, cols=33, seg_count=2), P(out_offset=2000, seg_begin=1)], segs=[segment(im, r1=39), segment(im, c1=9)])
    accepted(probs=[P(rows=40, cols=33, seg_count=2), P(out_offset=2000, seg_begin=1)], segs=[segment(im, r1=39, c1=32), segment(im)])
    accepted(probs=shared)
    # segment ranges
    refused('problem 0: segments [0, 0 + 2) outside the 1 given', probs=[P(seg_count=2)])
    refused('problem 0: segments [1, 1 + 1) outside the 1 given', probs=[P(seg_begin=1)])
    refused('outside the 1 given', probs=[P(seg_begin=-1)])
    refused('outside the 1 given', probs=[P(seg_count=-1)])
    accepted(probs=[P(seg_begin=1, seg_count=0)])
    # the place in d_out
    refused('problem 0: floats [-1, -1 + 72)', probs=[P(out_offset=-1)])
    refused('problem 0: floats [0, 0 + 72) of its 8 x 9 map lie outside the 71 of d_out', out_floats=71)
    accepted(out_floats=72)
    refused('problem 1: floats [100, 100 + 72)', probs=[P(), P(out_offset=100)], out_floats=171)
    accepted(probs=[P(), P(out_offset=100)], out_floats=172)
    # two problems sharing one float against sharing none, in either order of the table
    refused('the maps of problems 0 and 1 overlap in d_out (floats [0, 72) and [71, 143))', probs=[P(), P(out_offset=71)])
    refused('the maps of problems 1 and 0 overlap in d_out', probs=[P(out_offset=71), P()])
    refused('overlap in d_out', probs=[P(out_offset=500), P(), P(out_offset=200), P(out_offset=571)])
    accepted(probs=[P(), P(out_offset=72)])
    accepted(probs=[P(out_offset=72), P()])
    # a written range against d_desc sharing one element; d_desc in a gap between two maps is fine
    need = L.lib.c.simq_intention_shapes_desc_bytes(1, 1)
    assert need == 56 + 32 + 8
    refused('problem 0: its map at float 0 of d_out overlaps d_desc', out=DESC + need - 4, desc_bytes=need)
    accepted(out=DESC + need, desc_bytes=need)
    refused('problem 0: its map at float 0 of d_out overlaps d_desc', out=DESC - 72 * 4 + 4, desc_bytes=need)
    accepted(out=DESC - 72 * 4, desc_bytes=need)
    need2 = L.lib.c.simq_intention_shapes_desc_bytes(1, 2)
    gap = [P(), P(out_offset=72 + need2 // 4)]
    accepted(probs=gap, out=DESC - 72 * 4, desc_bytes=need2)
    refused('problem 1: its map at float %d of d_out overlaps d_desc' % (72 + need2 // 4 - 1), out=DESC - 72 * 4, desc_bytes=need2,
            probs=[P(), P(out_offset=72 + need2 // 4 - 1)])
    # alignment and the size of d_desc
    refused('aligned', desc=DESC + 4)
    refused('aligned', out=OUT + 2)
    refused('d_desc holds %d bytes, the descriptors and the tile table take %d' % (need - 1, need), desc_bytes=need - 1)
    accepted(desc_bytes=need)
    # modes, flags, doubles of a ramp, value of a store: the rules of simq_intention_maps under this entry's name
    refused('intention_maps_shapes: segment 0: mode 2', segs=[segment(im, mode=2)])
    refused('drop_last = 2', segs=[segment(im, drop_last=2)])
    refused('intention_maps_shapes: segment 0: start / stop / step is not finite', segs=[segment(im, step=float('nan'))])
    refused('not finite', segs=[segment(im, start=float('inf'))])
    accepted(segs=[segment(im, mode=im.STORE, value=0.0, step=float('nan'))])               # (a store does not read the doubles)
    refused('intention_maps_shapes: segment 0: stored value -0', segs=[segment(im, mode=im.STORE, value=-0.0)])
    refused('stored value', segs=[segment(im, mode=im.STORE, value=float('nan'))])
    accepted(segs=[segment(im, mode=im.STORE, value=0.0)])


def test_the_workgroup_count_is_bounded(L):
    """2^20 problems of 2047 tiles each fit 2^31 - 1 workgroups, of 2048 tiles do not (maps of 65 504 x 1 and 65 505 x 1)."""
    from simq import intention_drawing as im
    table = np.zeros(1 << 20, im.SHAPED_PROBLEM)
    table['cols'] = 1

    def call(rows):
        table['rows'] = rows
        table['out_offset'] = np.arange(len(table), dtype=np.int64) * rows
        return L.lib.c.simq_intention_maps_shapes(None, 0, table.ctypes.data_as(ctypes.c_void_p), len(table), ctypes.c_void_p(DESC), 1 << 30,
                                                  ctypes.c_void_p(0x100000000), len(table) * rows, None)
    assert call(65505) == -1 and 'workgroups (at most 2^31 - 1)' in L.last_error(), L.last_error()
    if not torch.cuda.is_available():
        assert call(65504) == -2, L.last_error()


def test_python_checks_lists_of_shapes_and_thicknesses_before_a_device_is_needed(L, monkeypatch):
    import simq
    from simq import intention_drawing as im
    calls = []
    monkeypatch.setattr(L.Lib, 'call', staticmethod(lambda *a, **k: calls.append(a)))
    path = [[(0.0, 0.0, 0.0), (0.5, 0.25, 0.0)]]
    two = [path, path]

    def refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            simq.intention_maps(*a, **kw)

    refused('3 map shapes for 2 problems', two, [(184, 232), (232, 232), (8, 8)], 'ramp')
    refused('1 map shapes for 2 problems', two, [(184, 232)], 'ramp')
    refused('3 line thicknesses for 2 problems', two, [(184, 232), (232, 232)], 'ramp', line_thickness=[1, 2, 3])
    refused('1 line thicknesses for 2 problems', two, (184, 232), 'ramp', line_thickness=[2])
    refused('3 encodings for 2 problems', two, [(184, 232), (232, 232)], ['ramp'] * 3)
    refused('line_thickness = 10', two, [(184, 232), (232, 232)], 'ramp', line_thickness=[2, 10])
    refused('line_thickness = 10', two, (184, 232), 'ramp', line_thickness=[10, 2])
    refused('line_thickness = 1.5', two, (184, 232), 'ramp', line_thickness=[1.5, 2])
    refused('line_thickness = 0', two, [(184, 232), (232, 232)], 'ramp', line_thickness=0)
    refused('map_shape is \\(rows, cols\\)', two, [(184, 232), (232,)], 'ramp')
    refused('rows, cols >= 1', two, [(184, 232), (0, 232)], 'ramp')
    refused('scale', two, [(184, 232), (232, 232)], 'ramp', scale=-1.0)
    refused('at least one problem', [], [], 'ramp')
    refused('flat float32 tensor of at least %d elements' % (184 * 232 + 232 * 232), two, [(184, 232), (232, 232)], 'ramp',
            out=torch.empty((2, 232, 232)))
    refused('flat float32 tensor', two, [(184, 232), (232, 232)], 'ramp', out=torch.empty(184 * 232 + 232 * 232 - 1))
    refused('flat float32 tensor', two, [(184, 232), (232, 232)], 'ramp', out=torch.empty(2 * 232 * 232, dtype=torch.float64))
    refused('flat float32 tensor', two, [(184, 232), (232, 232)], 'ramp', out=np.zeros(2 * 232 * 232, np.float32))
    assert not calls
    if not torch.cuda.is_available():
        # no quiet CPU path: with its arguments in order a call says that it needs the device
        for kw in (dict(map_shape=[(184, 232), (232, 232)]), dict(map_shape=(184, 232), line_thickness=[1, 3]),
                   dict(map_shape=[(184, 232), (232, 232)], out=torch.empty(2 * 232 * 232))):
            with pytest.raises(L.SimqError, match='need an MI355X'):
                simq.intention_maps(two, encoding='ramp', **kw)
        assert not calls
    # the one-shape, one-thickness call is the one it was
    assert not im._shape_list((184, 232)) and not im._shape_list([184, 232]) and im._shape_list([(184, 232)]) and im._shape_list([[184, 232]])


def test_the_mapper_option_is_a_bool_and_off_by_default(golden_dir):
    import test_device_transitions_cpu as tdc
    bm, _ = tdc.mapper_fixture(golden_dir)
    assert bm.one_drawing_launch is False
    import simq
    with pytest.raises(ValueError, match='one_drawing_launch must be True or False'):
        simq.BatchedMapper(1.0, 1.0, [['pushing_robot']], {}, one_drawing_launch=1)
