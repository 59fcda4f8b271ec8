"""numpy restatement of the reference Mapper's global intention / history maps (envs.py:2301-2346) and of the global maps behind its
spatial intention channels (envs.py:2360-2366), used by the intention-map tests.

A map is described by segments (r0, c0, r1, c1, mode, drop_last, value, start, stop, step), the form the C-ABI takes (include/simq.h):
`line_points` is the closed form of skimage.draw.line, `ramp_values` np.linspace's float64 sequence written out operation by
operation, `dilate` the maximum over the disk's offsets with the pixels outside the map left out.  `segments` computes the descriptors
from waypoint positions in the reference's order of float64 operations.  `sequential_line` is the published sequential
(Bresenham) algorithm skimage implements, kept for the tests that pin the closed form to it and for the fixture generator, which uses
it where the reference imports skimage.
"""
import math

import numpy as np

PIXELS_PER_METER = 96.0
ENCODINGS = ('circle', 'ramp', 'binary', 'line', 'history')
STORE, RAMP = 0, 1


def position_to_pixel_indices(position_x, position_y, image_shape):
    """envs.py:2391-2396."""
    pixel_i = np.floor(image_shape[0] / 2 - position_y * PIXELS_PER_METER).astype(np.int32)
    pixel_j = np.floor(image_shape[1] / 2 + position_x * PIXELS_PER_METER).astype(np.int32)
    return int(np.clip(pixel_i, 0, image_shape[0] - 1)), int(np.clip(pixel_j, 0, image_shape[1] - 1))


def sequential_line(r0, c0, r1, c1):
    """The integer line of skimage.draw.line: one pixel per step along the major axis, the error term deciding when the minor axis
    advances; the last pixel is the end point."""
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sr, sc = (1 if r1 > r0 else -1), (1 if c1 > c0 else -1)
    steep = dr > dc
    major, minor = (r0, c0) if steep else (c0, r0)
    n, m = (dr, dc) if steep else (dc, dr)
    s_major, s_minor = (sr, sc) if steep else (sc, sr)
    rr, cc = np.zeros(n + 1, np.intp), np.zeros(n + 1, np.intp)
    err = 2 * m - n
    for i in range(n):
        rr[i], cc[i] = (major, minor) if steep else (minor, major)
        while err >= 0:
            minor += s_minor
            err -= 2 * n
        major += s_major
        err += 2 * m
    rr[n], cc[n] = r1, c1
    return rr, cc


def line_points(r0, c0, r1, c1):
    """The same pixels in closed form: point i is i steps along the major axis and (2 * m * i + n) // (2 * n) along the minor one."""
    dr, dc = abs(r1 - r0), abs(c1 - c0)
    sr, sc = (1 if r1 > r0 else -1), (1 if c1 > c0 else -1)
    n, m = max(dr, dc), min(dr, dc)
    i = np.arange(n + 1, dtype=np.int64)
    minor = (2 * m * i + n) // (2 * n) if n > 0 else np.zeros(1, np.int64)
    if dr > dc:
        return r0 + sr * i, c0 + sc * minor
    return r0 + sr * minor, c0 + sc * i


def ramp_values(start, stop, step, num):
    """(float32) clip(np.linspace(start, stop, num), 0, 1) from its stored parameters: y_i = i * step + start with the product and the
    sum rounded separately, y_{num - 1} = stop."""
    y = np.arange(num, dtype=np.float64) * np.float64(step)
    y = y + np.float64(start)
    if num > 1:
        y[-1] = stop
    return np.clip(y, 0, 1).astype(np.float32)


def disk(radius):
    """skimage.morphology.disk: the (2 * radius + 1)^2 uint8 footprint x^2 + y^2 <= radius^2."""
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return np.asarray(X**2 + Y**2 <= radius**2, np.uint8)


def dilate(image, radius):
    """Grey dilation with disk(radius); pixels outside the image take no part."""
    rows, cols = image.shape
    out = image.copy()
    for di in range(-radius, radius + 1):
        for dj in range(-radius, radius + 1):
            if di * di + dj * dj > radius * radius or (di == 0 and dj == 0):
                continue
            src = image[max(di, 0):rows + min(di, 0), max(dj, 0):cols + min(dj, 0)]
            dst = out[max(-di, 0):rows + min(-di, 0), max(-dj, 0):cols + min(-dj, 0)]
            np.maximum(dst, src, out=dst)
    return out


def _length(a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    return math.sqrt(dx**2 + dy**2)


def segments(robots, map_shape, encoding, scale=1.0):
    """The descriptors of one map.  robots: per drawn robot its target position ('circle') or its waypoint list
    (get_intention_path() for 'ramp' / 'binary' / 'line', get_history_path() for 'history')."""
    assert encoding in ENCODINGS, encoding
    out = []
    for waypoints in robots:
        if encoding == 'circle':
            i, j = position_to_pixel_indices(waypoints[0], waypoints[1], map_shape)
            out.append((i, j, i, j, STORE, 0, scale, 0.0, 0.0, 0.0))
            continue
        waypoints = list(waypoints)
        if encoding == 'line':
            waypoints = [waypoints[0], waypoints[-1]]
        elif encoding == 'history':
            waypoints = waypoints[::-1]
        path_length = 0
        for k in range(1, len(waypoints)):
            a, b = waypoints[k - 1], waypoints[k]
            segment_length = scale * _length(a, b)
            r0, c0 = position_to_pixel_indices(a[0], a[1], map_shape)
            r1, c1 = position_to_pixel_indices(b[0], b[1], map_shape)
            drop_last = int(k < len(waypoints) - 1)
            if encoding in ('binary', 'line'):
                out.append((r0, c0, r1, c1, STORE, drop_last, scale, 0.0, 0.0, 0.0))
            else:
                start, stop = 1 - path_length, 1 - (path_length + segment_length)
                div = max(abs(r1 - r0), abs(c1 - c0))
                out.append((r0, c0, r1, c1, RAMP, drop_last, 0.0, float(start), float(stop), float((stop - start) / div if div else 0.0)))
            path_length += segment_length
    return out


def draw(segs, map_shape, radius):
    """The global map of the given segments, dilated with disk(radius)."""
    image = np.zeros(map_shape, np.float32)
    for r0, c0, r1, c1, mode, drop_last, value, start, stop, step in segs:
        rr, cc = line_points(int(r0), int(c0), int(r1), int(c1))
        values = ramp_values(start, stop, step, len(rr)) if mode == RAMP else np.full(len(rr), np.float32(value), np.float32)
        if drop_last:
            rr, cc, values = rr[:-1], cc[:-1], values[:-1]
        image[rr, cc] = np.maximum(image[rr, cc], values)
    return dilate(image, radius) if radius > 0 else image


def global_map(robots, map_shape, encoding, scale=1.0, line_thickness=2):
    """Mapper._create_global_intention_or_history_map(encoding) for the drawn robots' paths; with 'circle' and one target also the
    global map of a spatial intention channel."""
    return draw(segments(robots, map_shape, encoding, scale), map_shape, line_thickness - 1)


def load_fixture(path):
    """A tests/golden/intention_maps_*.npz file (tools/gen_intention_maps_golden.py): per problem its encoding, scale, line
    thickness, the drawn robots' paths as simq.intention_maps takes them, the number of robots the reference skipped as idle, whether
    the map is a spatial intention channel, the stored segment descriptors, the mapper robot's pose, the expected global map and the
    expected 96 x 96 local image."""
    z = np.load(path)
    P = len(z['prob_encoding'])
    problems = []
    for p in range(P):
        enc = ENCODINGS[int(z['prob_encoding'][p])]
        robots = []
        for r in np.nonzero(z['robot_prob'] == p)[0]:
            pts = [tuple(float(x) for x in w) for w in z['way_xyz'][z['way_robot'] == r]]
            robots.append(pts[0] if enc == 'circle' else pts)
        segs = [(int(a[0]), int(a[1]), int(a[2]), int(a[3]), int(mode), int(drop), float(value), float(start), float(stop), float(step))
                for a, mode, drop, value, start, stop, step, q in zip(z['seg_px'], z['seg_mode'], z['seg_drop_last'], z['seg_value'],
                                                                      z['seg_start'], z['seg_stop'], z['seg_step'], z['seg_prob']) if q == p]
        problems.append({'encoding': enc, 'scale': float(z['prob_scale'][p]), 'thickness': int(z['prob_thickness'][p]), 'robots': robots,
                         'idle': int(z['prob_idle'][p]), 'spatial': bool(z['prob_spatial'][p]), 'segments': segs,
                         'position': tuple(float(x) for x in z['prob_position'][p]), 'heading': float(z['prob_heading'][p]),
                         'tag': str(z['prob_tag'][p])})
    return {'shape': tuple(z['maps'].shape[1:]), 'problems': problems, 'maps': z['maps'], 'local': z['local']}
