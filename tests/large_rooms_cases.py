"""What the large-room tests and tools/gen_large_rooms_golden.py share: the two rooms of tests/golden/large_rooms.npz, its loader, and the
descriptor tables of the two large entry points for raw calls through the C ABI.

The rooms are (room_width, room_length) in metres: 0.5 x 1.3 pads to a 184 x 262 map -- only its columns are over
SIMQ_OCCUPANCY_MAX_DIM, and its room-mask box stays under the action cap -- and 1.6 x 1.6 to 290 x 290 with a 148 x 148 box, over both.
"""
import functools
import os

import numpy as np

ROOMS = ((0.5, 1.3), (1.6, 1.6))
SHAPES = ((184, 262), (290, 290))
ROBOT_TYPES = ('pushing_robot', 'lifting_robot', 'throwing_robot', 'rescue_robot')
PER_CLASS_LARGEST = 3                                   # cases of every class of store_new_action_oracle.CLASSES in the 1.6 m room


@functools.lru_cache(maxsize=None)
def load(golden_dir):
    """(rooms, cases).  rooms: per room a dict of shape, room_mask and maps, a list of dicts (name, robot_type, occupancy, radius,
    thin_radius and the reference's configuration_space, cspace_thin, closest).  cases: dicts as store_new_action_oracle.load_cases
    gives them, `room` an index into ROOMS and `map` one into that room's maps."""
    z = np.load(os.path.join(golden_dir, 'large_rooms.npz'))
    rooms = []
    for r in range(len(ROOMS)):
        k = 'room%d_' % r
        maps = [dict(name=str(z[k + 'names'][m]), robot_type=ROBOT_TYPES[int(z[k + 'robot_type'][m])], occupancy=z[k + 'occupancy'][m],
                     radius=int(z[k + 'radius'][m]), thin_radius=int(z[k + 'thin_radius'][m]),
                     configuration_space=z[k + 'configuration_space'][m], cspace_thin=z[k + 'cspace_thin'][m], closest=z[k + 'closest'][m])
                for m in range(len(z[k + 'names']))]
        rooms.append(dict(shape=tuple(int(x) for x in z[k + 'shape']), room_mask=z[k + 'room_mask'], maps=maps))
    off, cases = z['offsets'], []
    for c in range(len(z['a'])):
        way = z['waypoint_positions'][off[c]:off[c + 1]]
        cases.append(dict(room=int(z['room'][c]), map=int(z['map'][c]), robot_type=ROBOT_TYPES[int(z['robot_type'][c])],
                          use_shortest_path_movement=bool(z['use_shortest_path_movement'][c]), a=int(z['a'][c]),
                          position=(float(z['position'][c, 0]), float(z['position'][c, 1]), 0), heading=float(z['heading'][c]),
                          action=tuple(int(x) for x in z['action'][c]), target=(float(z['target'][c, 0]), float(z['target'][c, 1]), 0),
                          waypoints=[(float(w[0]), float(w[1]), 0) for w in way],
                          headings=[float(h) for h in z['waypoint_headings'][off[c]:off[c + 1]]]))
    return rooms, cases
