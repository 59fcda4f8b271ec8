"""Numpy oracle of the observation maps: a camera frame into the overhead and occupancy maps, as the reference's
Camera.capture_image (envs.py:1926-1954), Mapper.update (envs.py:2053-2061) and OccupancyMap.update (envs.py:2444-2449) compute them.

Everything is float32, one numpy operation per product, sum and quotient.  The one thing the reference leaves open is the order of
points of equal height (np.argsort's default sort is not stable); this project fixes it as the stable order, so that among the highest
points of a pixel the one with the largest row-major frame index is assigned last and stays.  `update` is written as the reference is:
sort, then assign in that order -- not as a per-pixel maximum.  A frame with a point that is not finite changes nothing (status 1); the
reference would let a NaN height win or lose pixels by the accident of its sort.
"""
import collections
import math

import numpy as np

Geometry = collections.namedtuple('Geometry', ('position', 'principal', 'right', 'up', 'pixel_x', 'pixel_y', 'far_near', 'far', 'far_minus_near'))
IdRanges = collections.namedtuple('IdRanges', ('min_obstacle', 'max_obstacle', 'receptacle', 'min_cube', 'max_cube'))
F = np.float32
OBSTACLE_SEG = F(2.0 / 8)


def camera_geometry(camera_position, camera_target, camera_up, near, far, aspect, image_height, fov=60):
    """The float32 camera vectors, pixel tables and depth constants, in the order of operations of envs.py:1931-1943."""
    near, far, aspect, fov = float(near), float(far), float(aspect), float(fov)   # (Python scalars, as the class constants are)
    height = int(image_height)
    width = int(aspect * height)
    position = np.array(camera_position, dtype=F)
    principal = np.array(camera_target, dtype=F) - position
    principal = principal / np.linalg.norm(principal)
    up = np.array(camera_up, dtype=F)
    up = up - np.dot(up, principal) * principal
    up = up / np.linalg.norm(up)
    right = np.cross(principal, up)
    right = right / np.linalg.norm(right)
    limit_y = math.tan(math.radians(fov / 2))
    limit_x = limit_y * aspect
    pixel_x = (2 * limit_x) * (np.arange(width, dtype=F) / width - 0.5)
    pixel_y = (2 * limit_y) * (0.5 - (np.arange(height, dtype=F) + 1) / height)
    out = [np.asarray(a, F) for a in (position, principal, right, up, pixel_x, pixel_y)]
    assert all(a.dtype == F for a in (position, principal, right, up, pixel_x, pixel_y))
    return Geometry(*out, F(far * near), F(far), F(far - near))


def depth_of(buffer, g):
    buffer = np.asarray(buffer, F)
    scaled = F(g.far_minus_near) * buffer
    denom = F(g.far) - scaled
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return (F(g.far_near) / denom).astype(F)


def points_of(buffer, g):
    """[height, width, 3] float32: p_c = cam_c + depth * ((principal_c + px[w] * right_c) + py[h] * up_c)."""
    depth = depth_of(buffer, g)
    px, py = np.asarray(g.pixel_x, F)[None, :], np.asarray(g.pixel_y, F)[:, None]
    out = np.empty(depth.shape + (3,), F)
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(3):
            side = px * F(g.right[c])
            vert = py * F(g.up[c])
            direction = (F(g.principal[c]) + side) + vert
            out[:, :, c] = F(g.position[c]) + depth * direction
    return out


def segmentation(ids, r):
    ids = np.asarray(ids)
    seg = F(1.0 / 8) * (ids == 0).astype(F)
    seg = seg + F(2.0 / 8) * np.logical_and(ids >= r.min_obstacle, ids <= r.max_obstacle).astype(F)
    if r.receptacle is not None:
        seg = seg + F(3.0 / 8) * (ids == r.receptacle).astype(F)
    seg = seg + F(4.0 / 8) * np.logical_and(ids >= r.min_cube, ids <= r.max_cube).astype(F)
    assert seg.dtype == F
    return seg


def pixel_indices(x, y, shape):
    """Mapper.position_to_pixel_indices on float32 coordinates; the clip is taken before the conversion to int."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    fi = np.floor(F(shape[0] / 2) - y * F(96.0))
    fj = np.floor(F(shape[1] / 2) + x * F(96.0))
    assert fi.dtype == F and fj.dtype == F
    return (np.clip(fi, 0, shape[0] - 1).astype(np.int32), np.clip(fj, 0, shape[1] - 1).astype(np.int32))


def update(overhead, occupancy, buffer, ids, g, r):
    """Update both maps in place with one frame; returns the status word (0, or 1: a point is not finite and nothing changed)."""
    assert overhead.dtype == F and occupancy.dtype == np.uint8 and overhead.shape == occupancy.shape
    points = points_of(buffer, g).reshape(-1, 3)
    if not np.isfinite(points).all():
        return 1
    seg = segmentation(ids, r).reshape(-1)
    z = points[:, 2] + F(0)                                          # -0 -> +0: one height
    order = np.argsort(z, kind='stable')
    i, j = pixel_indices(points[order, 0], points[order, 1], overhead.shape)
    overhead[i, j] = seg[order]                                     # repeated indices: the last assignment stays
    obstacle = seg == OBSTACLE_SEG
    i, j = pixel_indices(points[obstacle, 0], points[obstacle, 1], occupancy.shape)
    occupancy[i, j] = 1
    return 0


def tied_pixels(shape, buffer, ids, g, r):
    """(written [rows, cols] bool, ambiguous [rows, cols] bool, tied: {(i, j): set of seg values among the highest points of an
    ambiguous pixel}) of one frame on a map of `shape`."""
    points = points_of(buffer, g).reshape(-1, 3)
    seg = segmentation(ids, r).reshape(-1)
    i, j = pixel_indices(points[:, 0], points[:, 1], shape)
    cell = i.astype(np.int64) * shape[1] + j
    z = points[:, 2] + F(0)
    top = np.full(shape[0] * shape[1], -np.inf, F)
    np.maximum.at(top, cell, z)
    highest = z == top[cell]
    lo = np.full(shape[0] * shape[1], np.inf, F)
    hi = np.full(shape[0] * shape[1], -np.inf, F)
    np.minimum.at(lo, cell[highest], seg[highest])
    np.maximum.at(hi, cell[highest], seg[highest])
    written = np.zeros(shape[0] * shape[1], bool)
    written[cell] = True
    ambiguous = written & (lo != hi)
    tied = {}
    for k in np.flatnonzero(highest & ambiguous[cell]):
        tied.setdefault((int(i[k]), int(j[k])), set()).add(float(seg[k]))
    return written.reshape(shape), ambiguous.reshape(shape), tied


def load_fixture(path):
    """tests/golden/observation_maps_*.npz as (file-level arrays, [(name, record)]): a record holds the arrays of one frame
    (tools/gen_observation_maps_golden.py) plus 'geometry' and 'ranges' rebuilt from the stored vectors."""
    z = np.load(path)
    top = {k: z[k] for k in z.files if '/' not in k}
    out = []
    for name in top['names'].tolist():
        rec = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        v, c, ids = rec['vectors'], rec['depth_constants'], rec['id_ranges'].tolist()
        rec['geometry'] = Geometry(v[0], v[1], v[2], v[3], rec['pixel_x'], rec['pixel_y'], c[0], c[1], c[2])
        rec['ranges'] = IdRanges(ids[0], ids[1], ids[2] if ids[3] else None, ids[4], ids[5])
        out.append((name, rec))
    return top, out
