"""Robot.store_new_action (envs.py:856-902) in scalar Python, one robot at a time, on top of grid_waypoints_oracle's
OccupancyMap.shortest_path with the exact rule of grid_simplify_oracle as its simplifier: the rule of include/simq.h
(simq_action_waypoints), step by step.  tests/golden/store_new_action.npz holds what the reference's own function returned for the
same inputs; this restatement must equal it byte for byte (tests/test_store_new_action_cpu.py).
"""
import functools
import math
import os

import numpy as np

import grid_simplify_oracle as so
import grid_waypoints_oracle as wo

WIDTH = 96                                              # Mapper.LOCAL_MAP_PIXEL_WIDTH
CUBE_WIDTH = 0.044                                      # envs.py:25
ROBOT_TYPES = ('pushing_robot', 'lifting_robot', 'throwing_robot', 'rescue_robot')
ROOMS = ('184x232', '232x232')
BACKPACK_OFFSET, BASE_LENGTH = -0.0135, 0.065           # envs.py:804-805
END_EFFECTOR_LOCATION = {                               # envs.py:807, 1059-1060, 1279-1280
    'pushing_robot': BACKPACK_OFFSET + (BASE_LENGTH + 0.005), 'lifting_robot': BACKPACK_OFFSET + BASE_LENGTH,
    'throwing_robot': BACKPACK_OFFSET + (BASE_LENGTH + 0.006), 'rescue_robot': BACKPACK_OFFSET + BASE_LENGTH,
}
NUM_OUTPUT_CHANNELS = {'pushing_robot': 1, 'lifting_robot': 2, 'throwing_robot': 2, 'rescue_robot': 2}
CLASSES = ('straight', 'straight_back', 'three', 'four_or_more', 'traced_back')


def restrict_heading_range(h):
    return (h + math.pi) % (2 * math.pi) - math.pi      # envs.py:2566-2567


def distance(p1, p2):
    return math.sqrt((p2[0] - p1[0])**2 + (p2[1] - p1[1])**2)


def store_new_action(action, position, heading, robot_type, shortest_path=None):
    """(action, target_end_effector_position, waypoint_positions, waypoint_headings, signed_dist) of one robot.  shortest_path:
    callable(position, target) -> list of positions, None for use_shortest_path_movement = False."""
    action = tuple(np.unravel_index(action, (NUM_OUTPUT_CHANNELS[robot_type], WIDTH, WIDTH)))
    dx, dy = wo.pixel_indices_to_position(action[1], action[2], (WIDTH, WIDTH))
    dist = math.sqrt(dx**2 + dy**2)
    theta = heading + math.atan2(-dx, dy)
    target = (position[0] + dist * math.cos(theta), position[1] + dist * math.sin(theta), 0)
    waypoints = shortest_path(position, target) if shortest_path is not None else [position, target]
    headings = [heading]
    for i in range(1, len(waypoints)):
        headings.append(restrict_heading_range(math.atan2(waypoints[i][1] - waypoints[i - 1][1], waypoints[i][0] - waypoints[i - 1][0])))
    signed_dist = distance(waypoints[-2], waypoints[-1]) - (END_EFFECTOR_LOCATION[robot_type] + CUBE_WIDTH / 2)
    waypoints[-1] = (waypoints[-2][0] + signed_dist * math.cos(headings[-1]), waypoints[-2][1] + signed_dist * math.sin(headings[-1]), 0)
    if len(waypoints) > 2 and signed_dist < 0:
        waypoints[-2] = waypoints[-1]
        headings[-2] = restrict_heading_range(math.atan2(waypoints[-2][1] - waypoints[-3][1], waypoints[-2][0] - waypoints[-3][0]))
    return action, target, waypoints, headings, signed_dist


def kinds(n_waypoints, signed_dist, traced):
    """The classes of CLASSES a result belongs to."""
    if not traced:
        return ('straight_back',) if signed_dist < 0 else ('straight',)
    return ('three' if n_waypoints == 3 else 'four_or_more',) + (('traced_back',) if signed_dist < 0 else ())


@functools.lru_cache(maxsize=None)
def maps(golden_dir, room):
    z = np.load(os.path.join(golden_dir, 'occupancy_maps_%s.npz' % room))
    return z['configuration_space'], z['cspace_thin'], z['closest']


_PARENTS = {}                                           # (golden_dir, room, map): {source pixel: parents}, shared by every test of a session


def shortest_path_on(golden_dir, room, m):
    """OccupancyMap.shortest_path of map m of a room's occupancy fixture, its searches cached per source pixel."""
    cspace, thin, closest = maps(golden_dir, room)
    cache = _PARENTS.setdefault((golden_dir, room, int(m)), {})
    return lambda a, b: wo.occupancy_shortest_path(cspace[m], thin[m], closest[m], a, b, so.exact, cache)


def pixel_waypoints(cspace, thin, closest, source, target, cache=None):
    """What simq_action_waypoints returns for one problem: (status, int32 [count, 2] waypoint pixels source first, the end pixels the
    search used)."""
    if wo.is_straight(thin, source, target):
        return 1, np.zeros((0, 2), np.int32), tuple(source) + tuple(target)
    s = (int(closest[0][source]), int(closest[1][source]))
    t = (int(closest[0][target]), int(closest[1][target]))
    cache = {} if cache is None else cache
    if s not in cache:
        cache[s] = wo.spfa(cspace, s)[1]
    return 0, so.waypoints(cspace, wo.dense_path(cache[s], s, t)), s + t


def load_cases(golden_dir):
    """The cases of tests/golden/store_new_action.npz as dicts: room, map, robot_type, use_shortest_path_movement, a, position (a
    3-tuple of floats and the int 0), heading, and the four attributes: action (3 ints), target (x, y, 0), waypoints [(x, y, z)],
    headings [float]."""
    z = np.load(os.path.join(golden_dir, 'store_new_action.npz'))
    cases = []
    off = z['offsets']
    for k in range(len(z['a'])):
        way = z['waypoint_positions'][off[k]:off[k + 1]]
        cases.append(dict(room=ROOMS[z['room'][k]], map=int(z['map'][k]), robot_type=ROBOT_TYPES[z['robot_type'][k]],
                          use_shortest_path_movement=bool(z['use_shortest_path_movement'][k]), a=int(z['a'][k]),
                          position=(float(z['position'][k, 0]), float(z['position'][k, 1]), 0), heading=float(z['heading'][k]),
                          action=tuple(int(x) for x in z['action'][k]), target=(float(z['target'][k, 0]), float(z['target'][k, 1]), 0),
                          waypoints=[(float(w[0]), float(w[1]), 0) for w in way],
                          headings=[float(h) for h in z['waypoint_headings'][off[k]:off[k + 1]]]))
    return cases


def same_bits(a, b):
    """Two nested tuples / lists of numbers are equal with every float equal in its bytes (-0.0 is not 0.0) and every int an int."""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, (float, np.floating)) or isinstance(b, (float, np.floating)):
        return isinstance(a, (float, np.floating)) and isinstance(b, (float, np.floating)) and \
            np.float64(a).tobytes() == np.float64(b).tobytes()
    return int(a) == int(b)
