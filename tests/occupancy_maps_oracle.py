"""numpy restatement of what the reference's OccupancyMap.update derives from the occupancy map (envs.py:2453-2455), used by the
occupancy-map tests and by tools/gen_occupancy_maps_golden.py.

    configuration_space     1 - max(1 - room_mask, binary_dilation(occupancy_map, disk(radius)))
    cspace_thin             1 - binary_dilation(min(room_mask, occupancy_map), disk(thin_radius))
    closest_cspace_indices  distance_transform_edt(1 - configuration_space, return_distances=False, return_indices=True)

The dilation is an explicit loop over the offsets of the disk x^2 + y^2 <= r^2 with cells outside the map absent (the border value 0
of scipy.ndimage.binary_dilation).  The closest free cell follows the two one-dimensional passes of scipy's feature transform: the
nearest free row of every column (the earlier row on a tie), then over those column sites the nearest one (the earlier column on a
tie) -- among the nearest free cells the smallest column, then the smallest row.  The CPU tests pin both to scipy on fresh grids.
"""
import numpy as np


def disk(radius):
    """skimage.morphology.disk: the (2 r + 1)^2 uint8 footprint x^2 + y^2 <= r^2."""
    x = np.arange(-radius, radius + 1)
    return (x[:, None] ** 2 + x[None, :] ** 2 <= radius * radius).astype(np.uint8)


def dilate(image, radius):
    """Binary dilation of `image` (set where nonzero) with disk(radius); bool [rows, cols]."""
    src = np.asarray(image) != 0
    R, C = src.shape
    out = np.zeros((R, C), bool)
    for di in range(-radius, radius + 1):
        for dj in range(-radius, radius + 1):
            if di * di + dj * dj > radius * radius or abs(di) >= R or abs(dj) >= C:
                continue
            # out[i, j] |= src[i + di, j + dj] wherever the neighbour lies inside the map
            i0, i1, j0, j1 = max(0, -di), min(R, R - di), max(0, -dj), min(C, C - dj)
            out[i0:i1, j0:j1] |= src[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return out


def configuration_space(occupancy, room_mask, radius):
    return ((np.asarray(room_mask) != 0) & ~dilate(occupancy, radius)).astype(np.uint8)


def cspace_thin(occupancy, room_mask, thin_radius):
    return (~dilate((np.asarray(occupancy) != 0) & (np.asarray(room_mask) != 0), thin_radius)).astype(np.uint8)


def nearest_free_rows(free):
    """f0[i, j]: the nearest free row of column j seen from row i, the smaller row on a tie (columns without a free cell: 0), and
    the bool [cols] of the columns that hold a free cell."""
    R, C = free.shape
    f0 = np.zeros((R, C), np.int64)
    rows = np.arange(R)
    for j in range(C):
        fr = np.flatnonzero(free[:, j])
        if fr.size == 0:
            continue
        k = np.searchsorted(fr, rows)                                  # fr[k - 1] < i <= fr[k]
        above = fr[np.clip(k - 1, 0, fr.size - 1)]
        below = fr[np.clip(k, 0, fr.size - 1)]
        take_above = (k > 0) & ((k == fr.size) | (rows - above <= below - rows))
        f0[:, j] = np.where(take_above, above, below)
    return f0, free.any(axis=0)


def closest_free(cspace):
    """int32 [2, rows, cols]: the free cell (cspace != 0) nearest to every pixel; all -1 when no cell is free."""
    free = np.asarray(cspace) != 0
    R, C = free.shape
    out = np.full((2, R, C), -1, np.int32)
    if not free.any():
        return out
    f0, has = nearest_free_rows(free)
    sites = np.flatnonzero(has)                                        # ascending columns
    dj2 = (sites[None, :] - np.arange(C)[:, None]) ** 2                # [j, site]
    for i in range(R):
        d = dj2 + ((f0[i, sites] - i) ** 2)[None, :]
        k = d.argmin(axis=1)                                           # the first minimum: an equal distance keeps the earlier column
        out[1, i] = sites[k]
        out[0, i] = f0[i, sites[k]]
    return out


def update(occupancy, room_mask, radius, thin_radius):
    """(configuration_space, cspace_thin, closest_cspace_indices) of one map."""
    cs = configuration_space(occupancy, room_mask, radius)
    return cs, cspace_thin(occupancy, room_mask, thin_radius), closest_free(cs)


def load_fixture(path):
    """A fixture of tools/gen_occupancy_maps_golden.py as a list of dicts: name, occupancy, room_mask, radius, thin_radius and the
    reference's configuration_space, cspace_thin, closest."""
    z = np.load(path)
    return [dict(name=str(z['names'][k]), occupancy=z['occupancy'][k], room_mask=z['room_mask'][k], radius=int(z['radius'][k]),
                 thin_radius=int(z['thin_radius'][k]), configuration_space=z['configuration_space'][k], cspace_thin=z['cspace_thin'][k],
                 closest=z['closest'][k]) for k in range(len(z['names']))]
