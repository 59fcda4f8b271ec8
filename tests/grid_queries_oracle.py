"""numpy restatement of the reference's shortest-path point queries, used by the grid-query tests.

OccupancyMap.shortest_path_distance (envs.py:2506-2511): both positions to pixels (Mapper.position_to_pixel_indices,
envs.py:2391-2396), both pixels through closest_cspace_indices (envs.py:2522-2523), GridGraph.shortest_path_distance
(shortest_paths.pyx:150-158: the fp32 label of the target in the SPFA from the source, -1 where unreachable, returned as a Python
float), divided by Mapper.LOCAL_MAP_PIXELS_PER_METER, a Python float.  The distances are those of tests/grid_paths_oracle.py.
Mapper.distance_to_receptacle (envs.py:2189-2194) calls it with the receptacle as the source, or the Euclidean distance()
(envs.py:2556-2557) without shortest-path partial rewards.
"""
import math

import numpy as np

import grid_paths_oracle

PIXELS_PER_METER = 96.0                            # Mapper.LOCAL_MAP_PIXELS_PER_METER = 96 / 1.0 (envs.py:2010-2012)


def position_to_pixel_indices(position_x, position_y, image_shape):
    """Mapper.position_to_pixel_indices (envs.py:2391-2396)."""
    pixel_i = np.floor(image_shape[0] / 2 - position_y * PIXELS_PER_METER).astype(np.int32)
    pixel_j = np.floor(image_shape[1] / 2 + position_x * PIXELS_PER_METER).astype(np.int32)
    pixel_i = np.clip(pixel_i, 0, image_shape[0] - 1)
    pixel_j = np.clip(pixel_j, 0, image_shape[1] - 1)
    return int(pixel_i), int(pixel_j)


def snap(closest, pixel):
    """OccupancyMap._closest_valid_cspace_indices; closest None: the pixel as given."""
    if closest is None:
        return int(pixel[0]), int(pixel[1])
    i, j = closest[:, pixel[0], pixel[1]]
    return int(i), int(j)


def pixel_distances(grid, closest, source, targets, cache=None):
    """float32 [len(targets)]: GridGraph.shortest_path_distance(snap(source), snap(target)) per target.  cache: {snapped source:
    distance image}, the reference's _spfa_with_cache."""
    s = snap(closest, source)
    cache = {} if cache is None else cache
    if s not in cache:
        cache[s] = grid_paths_oracle.distance_image(grid, s)
    image = cache[s]
    return np.asarray([image[snap(closest, t)] for t in targets], np.float32)


def shortest_path_distance(cspace, closest, source_position, target_position, cache=None):
    """OccupancyMap.shortest_path_distance (envs.py:2506-2511) as a Python float."""
    source = position_to_pixel_indices(source_position[0], source_position[1], cspace.shape)
    target = position_to_pixel_indices(target_position[0], target_position[1], cspace.shape)
    return float(pixel_distances(cspace, closest, source, [target], cache)[0]) / PIXELS_PER_METER


def distance(p1, p2):
    """envs.py:2556-2557."""
    return math.sqrt((p2[0] - p1[0])**2 + (p2[1] - p1[1])**2)


def distance_to_receptacle(cspace, closest, receptacle_position, position, shortest_path=True, cache=None):
    """Mapper.distance_to_receptacle (envs.py:2189-2194)."""
    if shortest_path:
        return shortest_path_distance(cspace, closest, receptacle_position, position, cache)
    return distance(position, receptacle_position)
