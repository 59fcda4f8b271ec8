"""GPU: simq_observation_update_sequences (csrc/observation_maps.hip) -- several camera frames per pair of maps in one launch, applied
in the order given -- against the reference's own three successive updates (tests/golden/observation_maps_*.npz), against the numpy
oracle applied frame by frame (tests/observation_maps_oracle.py; a frame with a point that is not finite is skipped) and against
successive simq_observation_update launches on a twin pair of maps; simq.observation_update_sequences; BatchedMapper.defer / flush."""
import glob
import os

import numpy as np
import pytest

import mapper_oracle
import observation_maps_oracle as oracle

pytestmark = pytest.mark.gpu
F = np.float32
FILES = ('observation_maps_184x232.npz', 'observation_maps_232x232.npz')
CAMERAS = {'overhead': (0.1, 10, 1), 'forward': (0.001, 1, 16.0 / 9)}
RANGES = oracle.IdRanges(3, 9, 10, 11, 20)                          # ids: 0 floor 1/8, 3 .. 9 obstacle 2/8, 10 receptacle 3/8, 11 .. 20 cube 4/8
ID_PALETTE = np.asarray([-1, 0, 0, 0, 0, 1, 2, 3, 5, 9, 10, 10, 11, 20, 21], np.int32)
SMALL = (40, 300)                                                   # two tile rows (32) and two tile columns (256)
SENTINEL = F(-3.0)


@pytest.fixture(scope='module')
def S():
    import torch
    import simq
    from simq import observation
    assert torch.cuda.is_available()
    return simq, observation, torch


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == F else a


def prefilled(rng, shape):
    return np.full(shape, SENTINEL, F), np.where(rng.rand(*shape) < 0.3, 7, 0).astype(np.uint8)


def down(i, j, px, py, shape=SMALL):
    """A camera that looks straight down from the centre of map pixel (i, j) (or of the point between pixels for fractional i, j):
    x = cx + d * px[w], y = cy + d * py[h], z = 1 - d with the depth d = 1 / (10 - 8 * buffer)."""
    cx, cy = (j + 0.5 - shape[1] / 2) / 96.0, (shape[0] / 2 - (i + 0.5)) / 96.0
    return oracle.Geometry(F([cx, cy, 1]), F([0, 0, -1]), F([1, 0, 0]), F([0, 1, 0]), np.asarray(px, F), np.asarray(py, F), F(1), F(10), F(8))


# buffer values whose depth, and so whose height z = 1 - d, is exact: z = 0.75, 0.5, 0, -1
Z75, Z50, Z0, ZM1 = F(0.75), F(1.0), F(1.125), F(1.1875)


def on_pixel(i, j, buffer, ids, ranges=RANGES, shape=SMALL):
    """A frame whose points all land on map pixel (i, j): the tables are zero, only the heights and ids differ."""
    buffer, ids = np.asarray(buffer, F), np.asarray(ids, np.int32)
    return buffer, ids, down(i, j, np.zeros(buffer.shape[1]), np.zeros(buffer.shape[0]), shape), ranges


def landing(frame, shape):
    """(i, j, z, seg) of every point of a frame, flat, as the oracle has them."""
    buffer, ids, g, r = frame
    pts = oracle.points_of(buffer, g).reshape(-1, 3)
    i, j = oracle.pixel_indices(pts[:, 0], pts[:, 1], shape)
    return i, j, pts[:, 2] + F(0), oracle.segmentation(ids, r).reshape(-1)


def small_random(rng, k, shape, height=4):
    """tests/test_gpu_observation_maps.py's random_problem with a frame of `height` rows: either camera at a pose up to the border of
    a map of `shape`, depths from a few levels so that points of equal height and different seg share pixels."""
    kind = ('overhead', 'forward')[k % 2]
    near, far, aspect = CAMERAS[kind]
    heading = rng.uniform(-np.pi, np.pi)
    x, y = rng.uniform(-shape[1] / 192.0, shape[1] / 192.0), rng.uniform(-shape[0] / 192.0, shape[0] / 192.0)
    if kind == 'overhead':
        g = oracle.camera_geometry((x, y, 1), (x, y, 0), (np.cos(heading), np.sin(heading), 0), near, far, aspect, height)
        levels = ((far - far * near / np.asarray([1.0, 0.956, 0.9, 0.8])) / (far - near)).astype(F)
        buffer = levels[rng.randint(0, 4, (height, g.pixel_x.size))]
    else:
        c = np.cos(np.radians(60))
        g = oracle.camera_geometry((x, y, 0.08), (x + 0.14 * np.cos(heading), y + 0.14 * np.sin(heading), 0),
                                   (c * np.cos(heading), c * np.sin(heading), np.sin(np.radians(60))), near, far, aspect, height)
        buffer = np.where(rng.rand(height, g.pixel_x.size) < 0.2, 1.0, rng.uniform(0.99, 1.0, (height, g.pixel_x.size))).astype(F)
    ids = ID_PALETTE[rng.randint(0, ID_PALETTE.size, buffer.shape)]
    r = oracle.IdRanges(3, 9, None if k % 5 == 0 else 10, 11, 20)
    return np.ascontiguousarray(buffer, F), np.ascontiguousarray(ids, np.int32), g, r


def apply_oracle(host, sequences):
    """The oracle frame by frame on the numpy maps `host` [(overhead, occupancy)]; returns the status words, sequence by sequence."""
    return [[oracle.update(over, occ, *f) for f in frames] for (over, occ), frames in zip(host, sequences)]


def flat(S, sequences, interleave=False):
    """The arguments of observation_update_sequences for `sequences` (a list of frame lists): map by map, or round-robin over the maps."""
    simq, ob, torch = S
    order = [(s, k) for s, frames in enumerate(sequences) for k in range(len(frames))]
    if interleave:
        order.sort(key=lambda sk: (sk[1], sk[0]))
    fr = [sequences[s][k] for s, k in order]
    return ([f[0] for f in fr], [f[1] for f in fr], [ob.CameraGeometry(*f[2]) for f in fr], [ob.IdRanges(*f[3]) for f in fr]), [s for s, _ in order], order


def launch(S, sequences, host, interleave=False):
    """One observation_update_sequences call on device copies of `host`; returns the maps as numpy arrays and the status words in
    the caller's order (read through the wrapper's own enqueue, which is what the public function reads back)."""
    simq, ob, torch = S
    overs = [torch.from_numpy(o.copy()).cuda() for o, _ in host]
    occs = [torch.from_numpy(c.copy()).cuda() for _, c in host]
    args, index, order = flat(S, sequences, interleave)
    status, where = ob._enqueue_sequences(*args, overs, occs, index)
    codes = status.cpu().numpy()[where].tolist()
    return [(o.cpu().numpy(), c.cpu().numpy()) for o, c in zip(overs, occs)], codes, order


def successive(S, sequences, host):
    """The same frames as successive simq_observation_update launches on a twin set of maps: launch k holds the k-th frame of every
    sequence that has one and whose k-th frame is finite (the per-launch rule leaves the maps of a frame that is not unchanged)."""
    simq, ob, torch = S
    from simq._lib import SimqError
    overs = [torch.from_numpy(o.copy()).cuda() for o, _ in host]
    occs = [torch.from_numpy(c.copy()).cuda() for _, c in host]
    for k in range(max(len(frames) for frames in sequences)):
        mine = [s for s, frames in enumerate(sequences) if len(frames) > k]
        fr = [sequences[s][k] for s in mine]
        try:
            simq.observation_update([f[0] for f in fr], [f[1] for f in fr], [ob.CameraGeometry(*f[2]) for f in fr], [ob.IdRanges(*f[3]) for f in fr],
                                    [overs[s] for s in mine], [occs[s] for s in mine])
        except SimqError as e:
            assert 'not finite' in str(e)
    return [(o.cpu().numpy(), c.cpu().numpy()) for o, c in zip(overs, occs)]


def check(S, sequences, shapes, seed=0, with_successive=True, interleave=False):
    """One launch of `sequences` on sentinel-filled maps of `shapes` equals the oracle -- and successive launches -- bit for bit.
    Returns (maps, maps before, status words per sequence)."""
    rng = np.random.RandomState(seed)
    before = [prefilled(rng, s) for s in shapes]
    want = [(o.copy(), c.copy()) for o, c in before]
    want_status = apply_oracle(want, sequences)
    got, codes, order = launch(S, sequences, before, interleave)
    assert codes == [want_status[s][k] for s, k in order]
    twin = successive(S, sequences, before) if with_successive else got
    for s in range(len(sequences)):
        assert np.array_equal(bits(got[s][0]), bits(want[s][0])), ('overhead', s)
        assert np.array_equal(got[s][1], want[s][1]), ('occupancy', s)
        assert np.array_equal(bits(got[s][0]), bits(twin[s][0])) and np.array_equal(got[s][1], twin[s][1]), ('successive', s)
    return got, before, want_status


# ---- the reference's own successive updates, and every fixture frame as one sequence -------------------------------------------------
@pytest.mark.parametrize('fname', FILES)
def test_the_three_successive_updates_of_the_reference_as_one_sequence(S, golden_dir, fname):
    simq, ob, torch = S
    top, cases = oracle.load_fixture(os.path.join(golden_dir, fname))
    rec = dict(cases)
    steps = [rec['successive_step%d' % k] for k in range(3)]
    frames = [(s['depth'], s['ids'], s['geometry'], s['ranges']) for s in steps]
    shape = steps[0]['overhead_before'].shape
    # on the reference's own maps: the golden maps after the third update
    host = [(steps[0]['overhead_before'].copy(), steps[0]['occupancy_before'].copy())]
    got, codes, _ = launch(S, [frames], host)
    assert codes == [0, 0, 0]
    assert np.array_equal(bits(got[0][0]), bits(steps[2]['overhead_after'])) and np.array_equal(got[0][1], steps[2]['occupancy_after'])
    assert (steps[2]['overhead_after'] != steps[0]['overhead_after']).any()
    # on sentinel-filled maps, as int32: the oracle and three launches on a twin pair
    got, before, _ = check(S, [frames], [shape], seed=1)
    assert (got[0][0] == SENTINEL).any() and (got[0][0] != SENTINEL).any()


@pytest.mark.parametrize('fname', FILES)
def test_all_sixteen_fixture_frames_as_one_sequence_equal_sixteen_launches(S, golden_dir, fname):
    top, cases = oracle.load_fixture(os.path.join(golden_dir, fname))
    assert len(cases) == 16
    frames = [(r['depth'], r['ids'], r['geometry'], r['ranges']) for _, r in cases]
    assert len(set(f[0].shape for f in frames)) == 2                # overhead and forward-facing frames in one sequence
    check(S, [frames], [cases[0][1]['overhead_before'].shape], seed=2)


# ---- what a wrong key order gets wrong --------------------------------------------------------------------------------------------------
def test_the_order_of_frames_decides_and_heights_of_earlier_frames_do_not(S):
    P = (10, 20)
    cube_high = on_pixel(*P, [[Z75, Z50], [Z0, ZM1]], [[12, 0], [0, 0]])           # 4/8 at z = 0.75
    floor_low = on_pixel(*P, [[ZM1, ZM1], [ZM1, ZM1]], [[0, 0], [0, 0]])           # 1/8 at z = -1
    elsewhere = on_pixel(5, 7, [[Z0, Z0], [Z0, Z0]], [[3, 3], [3, 3]])             # an obstacle on another pixel
    no_class = on_pixel(*P, [[Z0, Z0], [Z0, Z0]], [[99, -1], [2, 99]])            # ids of no class: seg 0
    # equal greatest heights: in `tie8` index 7 (3/8) is the last of them, in `tie4` index 3 (1/8); index 7 > 3 must not carry over
    tie8 = on_pixel(*P, [[Z0, Z0, Z0, Z0], [Z0, Z0, Z0, Z0]], [[12, 12, 12, 12], [12, 12, 12, 10]])
    tie4 = on_pixel(*P, [[Z0, Z0], [Z0, Z0]], [[12, 3, 10, 0][:2], [10, 0]])
    sequences = [[cube_high, floor_low],                            # 0: a later, lower point wins
                 [cube_high, elsewhere],                            # 1: a later frame that misses the pixel leaves it
                 [cube_high, no_class],                             # 2: seg 0 over 4/8
                 [tie8, tie4],                                      # 3: the largest index of the LAST frame
                 [tie4, tie8],                                      # 4: and the other way round
                 [cube_high, floor_low, cube_high, floor_low],      # 5: the same physical frames given twice
                 [floor_low, floor_low],                            # 6: one frame twice
                 [elsewhere, cube_high]]
    for f in (cube_high, floor_low, no_class, tie8, tie4):
        i, j, z, seg = landing(f, SMALL)
        assert set(i.tolist()) == {P[0]} and set(j.tolist()) == {P[1]}
    assert landing(cube_high, SMALL)[2].max() == F(0.75) and landing(floor_low, SMALL)[2].max() == F(-1) and set(landing(no_class, SMALL)[3].tolist()) == {0.0}
    assert (landing(tie8, SMALL)[2] == 0).all() and (landing(tie4, SMALL)[2] == 0).all()
    got, before, status = check(S, sequences, [SMALL] * len(sequences), seed=3)
    value = lambda s, p=P: float(got[s][0][p])
    assert value(0) == 0.125 and value(1) == 0.5 and value(1, (5, 7)) == 0.25 and value(2) == 0.0
    assert value(3) == 0.125 and value(4) == 0.375 and value(5) == 0.125 and value(6) == 0.125
    assert got[1][1][5, 7] == 1 and got[0][1][P] == before[0][1][P]
    for s in range(len(sequences)):                                 # nothing else was touched
        untouched = np.ones(SMALL, bool)
        untouched[P], untouched[5, 7] = False, False
        assert (got[s][0][untouched] == SENTINEL).all() and np.array_equal(got[s][1][untouched], before[s][1][untouched])


def test_cameras_of_different_sizes_in_one_sequence_and_points_on_tile_edges_and_corners(S):
    rng = np.random.RandomState(4)
    half = 0.5 / 96
    # the four pixels around the corner between the tiles: (31, 255), (31, 256), (32, 255), (32, 256)
    edge = (np.full((2, 2), Z0, F), np.asarray([[12, 3], [10, 0]], np.int32), down(31.5, 255.5, [-half, half], [half, -half]), RANGES)
    i, j, _, _ = landing(edge, SMALL)
    assert sorted(zip(i.tolist(), j.tolist())) == [(31, 255), (31, 256), (32, 255), (32, 256)]
    # points far outside the map clip to its four corners
    corners = (np.full((2, 2), Z0, F), np.asarray([[3, 12], [0, 10]], np.int32), down(20, 150, [-1000, 1000], [1000, -1000]), RANGES)
    i, j, _, _ = landing(corners, SMALL)
    assert sorted(zip(i.tolist(), j.tolist())) == [(0, 0), (0, 299), (39, 0), (39, 299)]
    later = (np.full((2, 2), Z50, F), np.asarray([[0, 0], [3, 12]], np.int32)) + edge[2:]
    mixed = [small_random(rng, k, SMALL, height) for k, height in enumerate((4, 4, 6, 3, 2, 5))]
    assert len(set(f[0].shape for f in mixed)) >= 5 and {f[0].shape[1] == f[0].shape[0] for f in mixed} == {True, False}
    got, before, _ = check(S, [[edge, corners, later], mixed, [corners, edge] + mixed], [SMALL] * 3, seed=5)
    assert [float(got[0][0][p]) for p in ((31, 255), (31, 256), (32, 255), (32, 256))] == [0.125, 0.125, 0.25, 0.5]
    assert [float(got[0][0][p]) for p in ((0, 0), (0, 299), (39, 0), (39, 299))] == [0.25, 0.5, 0.125, 0.375]
    assert got[0][1][0, 0] == 1 and got[0][1][32, 255] == 1 and got[0][1][31, 256] == 1


# ---- a frame with a point that is not finite is skipped as a whole -----------------------------------------------------------------------
def test_a_frame_that_is_not_finite_is_skipped_and_the_rest_of_its_sequence_applied(S):
    rng = np.random.RandomState(6)
    good = [small_random(rng, 2 * k, SMALL, 4) for k in range(3)]
    # the bad frame: 3 x 4 points, one NaN depth in its LAST point; before it an obstacle on a pixel of its own and a cube on another
    alone, obstacle = (3, 290), (36, 9)
    px = np.asarray([0, 0, 0, 0], F)
    bad = (np.full((3, 4), Z0, F), np.full((3, 4), 12, np.int32), down(*alone, px, [0, 0, 0]), RANGES)
    bad[0][2, 3] = np.nan
    bad_obstacle = on_pixel(*obstacle, [[Z0, np.nan]], [[3, 3]])
    for f in good:
        i, j, _, _ = landing(f, SMALL)
        assert alone not in set(zip(i.tolist(), j.tolist())) and obstacle not in set(zip(i.tolist(), j.tolist()))
    neighbours = [[small_random(rng, k, SMALL, 4) for k in range(3)], [small_random(rng, 7, SMALL, 5)]]
    all_bad = [bad, bad_obstacle]
    four = [good[0], bad, good[1], good[2]]
    sequences = [neighbours[0], four, neighbours[1], [good[0], bad_obstacle, good[1], good[2]], all_bad, good]
    got, before, status = check(S, sequences, [SMALL] * len(sequences), seed=7)
    assert status[1] == [0, 1, 0, 0] and status[3] == [0, 1, 0, 0] and status[4] == [1, 1] and status[0] == [0, 0, 0] and status[2] == [0]
    # the maps of the sequence of four are those of the three good frames on the same maps
    three, _, _ = launch(S, [good], [before[1]])
    assert np.array_equal(bits(got[1][0]), bits(three[0][0])) and np.array_equal(got[1][1], three[0][1])
    assert got[1][0][alone] == SENTINEL and got[3][1][obstacle] == before[3][1][obstacle] and got[3][0][obstacle] == SENTINEL
    # a sequence whose every frame is bad changes nothing
    assert np.array_equal(bits(got[4][0]), bits(before[4][0])) and np.array_equal(got[4][1], before[4][1])
    # and the public function names the frames, in the caller's order, after everything else is applied
    simq, ob, torch = S
    from simq._lib import SimqError
    args, index, order = flat(S, sequences, interleave=True)
    overs = [torch.from_numpy(o.copy()).cuda() for o, _ in before]
    occs = [torch.from_numpy(c.copy()).cuda() for _, c in before]
    named = [n for n, (s, k) in enumerate(order) if status[s][k] == 1]
    with pytest.raises(SimqError, match=r'4 frame\(s\) hold a point that is not finite.*frames %s' % str(named).replace('[', r'\[').replace(']', r'\]')):
        simq.observation_update_sequences(*args, overs, occs, index)
    for s in range(len(sequences)):
        assert np.array_equal(bits(overs[s].cpu().numpy()), bits(got[s][0])) and np.array_equal(occs[s].cpu().numpy(), got[s][1])


# ---- one launch of mixed sequences ----------------------------------------------------------------------------------------------------
def test_one_launch_of_sequences_of_lengths_1_2_7_and_40_over_both_rooms(S):
    simq, ob, torch = S
    rng = np.random.RandomState(8)
    shapes = [(184, 232), (232, 232)] * 4
    lengths = [1, 1, 2, 2, 7, 7, 40, 40]
    sequences = [[small_random(rng, k + n, shape, 4 + (k + n) % 3) for k in range(n)] for n, shape in zip(lengths, shapes)]
    got, before, _ = check(S, sequences, shapes, seed=9, with_successive=False)
    n_written = sum(int((g[0] != SENTINEL).sum()) for g in got)
    border = sum(int((g[0][0] != SENTINEL).sum() + (g[0][-1] != SENTINEL).sum() + (g[0][:, 0] != SENTINEL).sum() + (g[0][:, -1] != SENTINEL).sum()) for g in got)
    assert n_written > 1000 and border > 10
    # the sequences of one frame equal simq_observation_update on the same frames
    ones = [s for s, n in enumerate(lengths) if n == 1]
    overs = [torch.from_numpy(before[s][0].copy()).cuda() for s in ones]
    occs = [torch.from_numpy(before[s][1].copy()).cuda() for s in ones]
    fr = [sequences[s][0] for s in ones]
    simq.observation_update([f[0] for f in fr], [f[1] for f in fr], [ob.CameraGeometry(*f[2]) for f in fr], [ob.IdRanges(*f[3]) for f in fr], overs, occs)
    for k, s in enumerate(ones):
        assert np.array_equal(bits(overs[k].cpu().numpy()), bits(got[s][0])) and np.array_equal(occs[k].cpu().numpy(), got[s][1])
    # every sequence against successive launches too (40 launches of up to 8 problems)
    twin = successive(S, sequences, before)
    for s in range(len(sequences)):
        assert np.array_equal(bits(twin[s][0]), bits(got[s][0])) and np.array_equal(twin[s][1], got[s][1]), s


# ---- the cap ---------------------------------------------------------------------------------------------------------------------------
def cap_frames(rng, n):
    """n frames of 2 x 2 points that fall on an 8 x 8 map, each around a random pixel with random heights and ids."""
    half = 1.0 / 96
    out = []
    for _ in range(n):
        buffer = np.asarray([Z75, Z50, Z0, ZM1], F)[rng.randint(0, 4, (2, 2))]
        ids = ID_PALETTE[rng.randint(0, ID_PALETTE.size, (2, 2))]
        out.append((buffer, np.ascontiguousarray(ids), down(rng.randint(0, 8), rng.randint(0, 8), [-half, half], [half, -half], (8, 8)), RANGES))
    return out


def test_the_cap_1023_frames_in_one_launch_and_1030_in_two(S, monkeypatch):
    simq, ob, torch = S
    from simq import _lib as L
    rng = np.random.RandomState(10)
    frames = cap_frames(rng, 1030)
    names = []
    real = L.Lib.call
    monkeypatch.setattr(L.Lib, 'call', staticmethod(lambda name, *a, **k: names.append(name) or real(name, *a, **k)))
    for n, launches in ((1023, 1), (1030, 2)):
        # two maps: the capped one and a short neighbour, given round-robin
        sequences = [frames[:n], frames[5:8]]
        before = [prefilled(rng, (8, 8)) for _ in sequences]
        want = [(o.copy(), c.copy()) for o, c in before]
        assert sum(sum(st) for st in apply_oracle(want, sequences)) == 0
        args, index, order = flat(S, sequences, interleave=True)
        overs = [torch.from_numpy(o.copy()).cuda() for o, _ in before]
        occs = [torch.from_numpy(c.copy()).cuda() for _, c in before]
        del names[:]
        simq.observation_update_sequences(*args, overs, occs, index)
        assert names == ['simq_observation_update_sequences'] * launches
        for s in range(2):
            assert np.array_equal(bits(overs[s].cpu().numpy()), bits(want[s][0])) and np.array_equal(occs[s].cpu().numpy(), want[s][1]), (n, s)
        assert (want[0][0] != SENTINEL).all()
    # the library itself refuses 1024 frames of one map
    from simq._lib import SimqError
    probs = (ob.ObservationProblem * 1024)()
    with pytest.raises(SimqError, match='at most 1023 frames per sequence'):
        ob.call_sequences(torch.zeros(8, dtype=torch.int32, device='cuda'), 8, probs, np.asarray([0, 1024], np.int32),
                          (overs[0].data_ptr(), 64, occs[0].data_ptr(), 64), torch.zeros(1024, dtype=torch.int32, device='cuda'), overs[0].device)


# ---- frames of several maps given round-robin ------------------------------------------------------------------------------------------
def test_interleaved_map_index_keeps_the_order_per_map_and_the_status_in_the_callers_order(S):
    rng = np.random.RandomState(11)
    bad = on_pixel(3, 3, [[Z0, np.nan]], [[3, 3]])
    ordered = [on_pixel(20, 100, [[Z0]], [[12]]), on_pixel(20, 100, [[Z0]], [[0]])]        # (frames whose order shows in the map)
    sequences = [[small_random(rng, k, SMALL, 4) for k in range(3)] + ordered, [small_random(rng, k + 1, SMALL, 3) for k in range(3)] + [bad],
                 [small_random(rng, k, SMALL, 5) for k in range(2)]]
    got, _, status = check(S, sequences, [SMALL] * 3, seed=12, interleave=True)           # (check compares the status in the caller's order)
    straight, _, _ = check(S, sequences, [SMALL] * 3, seed=12, interleave=False, with_successive=False)
    for a, b in zip(got, straight):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    assert status == [[0] * 5, [0, 0, 0, 1], [0, 0]]
    # the order within a map matters in these frames: the reversed sequences give other maps
    reverse, _, _ = launch(S, [frames[::-1] for frames in sequences], [prefilled(np.random.RandomState(12), SMALL) for _ in range(3)])
    assert any(not np.array_equal(bits(a[0]), bits(b[0])) for a, b in zip(got, reverse))


# ---- refusals: nothing is written ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_the_single_frame_entry_still_refuses_one_map_twice(S):
    simq, ob, torch = S
    from simq._lib import SimqError
    rng = np.random.RandomState(13)
    a, b = small_random(rng, 0, SMALL, 4), small_random(rng, 2, SMALL, 4)
    over = torch.full((2,) + SMALL, float(SENTINEL), dtype=torch.float32, device='cuda')
    occ = torch.zeros((2,) + SMALL, dtype=torch.uint8, device='cuda')
    args = ([a[0], b[0]], [a[1], b[1]], [ob.CameraGeometry(*a[2]), ob.CameraGeometry(*b[2])], ob.IdRanges(*RANGES))

    def untouched():
        torch.cuda.synchronize()
        return bool((over == float(SENTINEL)).all()) and not bool(occ.any())
    # two sequences naming one overhead map, one occupancy map
    for overs, occs in (([over[0], over[0]], [occ[0], occ[1]]), ([over[0], over[1]], [occ[1], occ[1]])):
        with pytest.raises(SimqError, match='simq_observation_update_sequences.*share memory'):
            simq.observation_update_sequences(*args, overs, occs, [0, 1])
        assert untouched()
        with pytest.raises(SimqError, match=r'simq_observation_update\b.*share memory at address .* \(every problem needs an overhead map and an '
                                            r'occupancy map of its own: the order of two updates of one map matters\)'):
            simq.observation_update(*args, overs, occs)
        assert untouched()
    # the frames of one sequence differ in rows: the descriptors by hand
    parts, words, tables, offsets = ob._layout(args[0], args[1], args[2])
    frames = torch.from_numpy(np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.int32) for p in parts])).cuda()
    probs = (ob.ObservationProblem * 2)()
    for k in range(2):
        ob._describe(probs[k], args[2][k], args[3], offsets[k], tables[id(args[2][k])], args[0][k].shape, 0, 0, (SMALL[0] - k, SMALL[1]))
    status = torch.full((2,), -1, dtype=torch.int32, device='cuda')
    with pytest.raises(SimqError, match=r'sequence 0: frame 1 names rows 39, frame 0 names 40'):
        ob.call_sequences(frames, words, probs, [0, 2], (over.data_ptr(), over.numel(), occ.data_ptr(), occ.numel()), status, over.device)
    assert untouched() and status.cpu().tolist() == [-1, -1]
    # the same descriptors as two sequences of one frame name one map twice; with rows agreeing they are one good sequence
    with pytest.raises(SimqError, match='share memory'):
        ob.call_sequences(frames, words, probs, [0, 1, 2], (over.data_ptr(), over.numel(), occ.data_ptr(), occ.numel()), status, over.device)
    assert untouched() and status.cpu().tolist() == [-1, -1]
    probs[1].rows = SMALL[0]
    ob.call_sequences(frames, words, probs, [0, 2], (over.data_ptr(), over.numel(), occ.data_ptr(), occ.numel()), status, over.device)
    assert status.cpu().tolist() == [0, 0] and not untouched()


# ---- BatchedMapper.defer / flush -------------------------------------------------------------------------------------------------------
KINDS = ('overhead', 'occupancy', 'configuration_space', 'cspace_thin', 'closest_cspace_indices')


@pytest.fixture(scope='module')
def episodes(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, 'mapper_*.npz')))
    assert len(files) == 2, files
    return [mapper_oracle.load_fixture(f) for f in files]


def build(simq, episodes, cfg):
    masks = {name: episodes[0]['masks'][k] for k, name in enumerate(episodes[0]['mask_names'])}
    flags = {f: cfg[f] for f in mapper_oracle.FLAGS}
    rest = {k: v for k, v in cfg.items() if k not in mapper_oracle.FLAGS}
    return simq.BatchedMapper([f['room_width'] for f in episodes], [f['room_length'] for f in episodes], [f['types'] for f in episodes], masks,
                              [f['groups'] for f in episodes], [f['receptacle_position'] for f in episodes], **flags, **rest)


def round_frames(ob, episodes, t):
    """(depth, ids, geometries, id_ranges) of round t: the six mappers of both rooms."""
    fr = [f for ep in episodes for f in ep['rounds'][t]['frames']]
    return [f['depth'] for f in fr], [f['ids'] for f in fr], [ob.CameraGeometry(*f['geometry']) for f in fr], [ob.IdRanges(*f['ranges']) for f in fr]


def robot_states(simq, episodes, t):
    return [[simq.RobotState(r['position'], r['heading'], r['type'], r['lift_state'], r['idle'], r['target'], r['intention_path'], r['history_path'])
             for r in ep['rounds'][t]['robots']] for ep in episodes]


def same_maps(a, b, mappers=range(6)):
    for kind in KINDS + ('room_masks',):
        for m in mappers:
            x, y = getattr(a, kind)[m].cpu().numpy(), getattr(b, kind)[m].cpu().numpy()
            if not np.array_equal(bits(x), bits(y)):
                return False
    return True


def test_three_rounds_deferred_and_one_flush_equal_three_updates(S, episodes, monkeypatch):
    simq, ob, torch = S
    from simq import _lib as L
    cfg = mapper_oracle.configurations()['full_spatial']
    bm, twin = build(simq, episodes, cfg), build(simq, episodes, cfg)
    assert bm.num_mappers == 6 and not bm.uniform and len(episodes[0]['rounds']) == 3
    for t in range(3):
        frames = round_frames(ob, episodes, t)
        twin.update(*frames)
        mine = [np.array(a) for a in frames[0]], [np.array(a) for a in frames[1]], frames[2], frames[3]
        if t == 1:                                                  # in two calls over shuffled subsets
            for ms in ([4, 1, 5, 0], [3, 2]):
                bm.defer(*[[part[m] for m in ms] for part in mine], mappers=ms)
        else:
            bm.defer(*mine)
        for a in mine[0]:                                           # the caller's arrays are the caller's again
            a.fill(np.nan)
        for a in mine[1]:
            a.fill(-7)
    assert bm.pending.tolist() == [3] * 6
    names, reads = [], []
    real, real_cpu = L.Lib.call, torch.Tensor.cpu
    with monkeypatch.context() as mp:
        mp.setattr(L.Lib, 'call', staticmethod(lambda name, *a, **k: names.append(name) or real(name, *a, **k)))
        mp.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: reads.append(1) or real_cpu(self, *a, **k))
        L.lib.c.simq_launch_counts_reset()
        bm.flush()
        assert L.launch_counts() == {'observation_sequences': 1, 'occupancy_maps': 1}
    assert names == ['simq_observation_update_sequences', 'simq_occupancy_maps'] and len(reads) == 1
    assert bm.pending.tolist() == [0] * 6 and same_maps(bm, twin)
    assert np.array_equal(bm.occupancy_status.cpu().numpy(), twin.occupancy_status.cpu().numpy()) and bm.occupancy_status.cpu().tolist() == [0] * 6
    got = bm.get_states(robot_states(simq, episodes, 2)).cpu().numpy()
    want = np.stack([mapper_oracle.expected_state(cfg, episodes[m // 3]['rounds'][2]['images'], m % 3, 3) for m in range(6)])
    assert np.array_equal(bits(got), bits(want))
    bm.flush()                                                      # nothing is pending: nothing happens
    assert same_maps(bm, twin)


def test_flush_of_named_mappers_leaves_the_others_pending_and_reads_of_pending_mappers_raise(S, episodes):
    simq, ob, torch = S
    from simq._lib import SimqError
    cfg = mapper_oracle.configurations()['full_spatial']
    bm, twin = build(simq, episodes, cfg), build(simq, episodes, cfg)
    frames = [round_frames(ob, episodes, t) for t in range(3)]
    pick = lambda fr, ms: [[part[m] for m in ms] for part in fr]
    robots = robot_states(simq, episodes, 1)
    bm.defer(*frames[0])
    bm.defer(*pick(frames[1], [5, 2]), mappers=[5, 2])
    assert bm.pending.tolist() == [1, 1, 2, 1, 1, 2]
    for call in (lambda: bm.update(*pick(frames[1], [2]), mappers=[2]), lambda: bm.get_states(robots, mappers=[0, 2]),
                 lambda: bm.get_states(simq.RobotArrays.from_states(bm, robots), mappers=[5]),
                 lambda: bm.shortest_paths([(0, 0)], [(0.1, 0.1)], mappers=[4]), lambda: bm.distances_to_receptacle([[(0, 0)]], mappers=[1])):
        with pytest.raises(SimqError, match=r'have deferred frames.*flush'):
            call()
    assert not bool(bm.overhead[2].any()) and bm.occupancy_status.cpu().tolist() == [4] * 6        # nothing was queued
    bm.flush(mappers=[2, 0, 4])
    assert bm.pending.tolist() == [0, 1, 0, 1, 0, 2]
    twin.update(*pick(frames[0], [0, 2, 4]), mappers=[0, 2, 4])
    twin.update(*pick(frames[1], [2]), mappers=[2])
    assert same_maps(bm, twin) and bm.occupancy_status.cpu().tolist() == [0, 4, 0, 4, 0, 4]
    bm.get_states(robots, mappers=[0, 2, 4])                        # the flushed mappers are readable
    # what waited keeps its order and its content while other frames come and go
    bm.defer(*pick(frames[2], [5, 0]), mappers=[5, 0])
    bm.flush(mappers=[0])
    bm.flush()
    twin.update(*pick(frames[0], [1, 3, 5]), mappers=[1, 3, 5])
    twin.update(*pick(frames[1], [5]), mappers=[5])
    twin.update(*pick(frames[2], [5, 0]), mappers=[5, 0])
    assert bm.pending.tolist() == [0] * 6 and same_maps(bm, twin)
    # reset drops the deferred frames of its environments only
    bm.defer(*frames[1])
    bm.reset([0])
    assert bm.pending.tolist() == [0, 0, 0, 1, 1, 1] and not bool(bm.overhead[1].any())
    bm.flush()
    twin.reset([0])
    twin.update(*pick(frames[1], [3, 4, 5]), mappers=[3, 4, 5])
    assert same_maps(bm, twin) and bm.occupancy_status.cpu().tolist() == [4, 4, 4, 0, 0, 0]


def test_a_deferred_frame_that_is_not_finite_is_named_and_every_other_mapper_updated(S, episodes):
    simq, ob, torch = S
    from simq._lib import SimqError
    cfg = mapper_oracle.configurations()['full_spatial']
    bm, twin = build(simq, episodes, cfg), build(simq, episodes, cfg)
    frames = [round_frames(ob, episodes, t) for t in range(3)]
    bad = frames[1][0][4].copy()
    bad[77, 5] = np.nan
    for t in range(3):
        depth = list(frames[t][0])
        if t == 1:
            depth[4] = bad
        bm.defer(depth, *frames[t][1:])
        if t == 1:
            others = [0, 1, 2, 3, 5]
            twin.update(*[[part[m] for m in others] for part in frames[t]], mappers=others)
        else:
            twin.update(*frames[t])
    with pytest.raises(SimqError, match=r'BatchedMapper.flush: simq_observation_update_sequences: mapper 4 \(environment 1, robot 1\) frame 1 hold a point '
                                        r'that is not finite'):
        bm.flush()
    assert bm.pending.tolist() == [0] * 6 and same_maps(bm, twin) and bm.occupancy_status.cpu().tolist() == [0] * 6
