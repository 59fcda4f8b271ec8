"""simq -- MI355X-native spatial-action-map DQN learner (hot path only).

Host-side mirror of the reference's Python interface for the path
train.py / networks.py / policies.py; the arithmetic lives in hand-written HIP
kernels behind the C-ABI of ``include/simq.h`` (libsimq.so).  Submodules that
need torch / the HIP library are imported lazily so that ``simq.arch`` and
``simq.synth`` stay importable on a bare CPU box.
"""
import importlib

_LAZY = {
    'FCN': ('.fcn', 'FCN'),
    'DQNPolicy': ('.policy', 'DQNPolicy'),
    'DQNIntentionPolicy': ('.policy', 'DQNIntentionPolicy'),
    'ReplayBuffer': ('.learner', 'ReplayBuffer'),
    'DeviceReplayBuffer': ('.learner', 'DeviceReplayBuffer'),
    'AliasedDeviceReplayBuffer': ('.learner', 'AliasedDeviceReplayBuffer'),
    'TransitionTracker': ('.tracker', 'TransitionTracker'),
    'Transition': ('.learner', 'Transition'),
    'train': ('.learner', 'train'),
    'train_step': ('.learner', 'train_step'),
    'train_groups': ('.learner', 'train_groups'),
    'StepOptions': ('.learner', 'StepOptions'),
    'learner_streams': ('.learner', 'learner_streams'),
    'train_step_dataparallel': ('.learner', 'train_step_dataparallel'),
    'train_intention': ('.learner', 'train_intention'),
    'train_intention_step': ('.learner', 'train_intention_step'),
    'lib': ('._lib', 'lib'),
    'Collector': ('.collector', 'Collector'),
    'CollectWorker': ('.collector', 'CollectWorker'),
    'save_policy': ('.checkpoint', 'save_policy'),
    'save_checkpoint': ('.checkpoint', 'save_checkpoint'),
    'load_checkpoint': ('.checkpoint', 'load_checkpoint'),
    'resume': ('.checkpoint', 'resume'),
    'GridGraph': ('.grid_paths', 'GridGraph'),
    'grid_distance_images': ('.grid_paths', 'grid_distance_images'),
    'WaypointGraph': ('.waypoints', 'WaypointGraph'),
    'grid_dense_paths': ('.waypoints', 'grid_dense_paths'),
    'shortest_paths': ('.waypoints', 'shortest_paths'),
    'grid_waypoints': ('.waypoints', 'grid_waypoints'),
    'approximate_polygon_exact': ('.waypoints', 'approximate_polygon_exact'),
    'store_new_actions': ('.actions', 'store_new_actions'),
    'NewActions': ('.actions', 'NewActions'),
    'grid_distance_queries': ('.grid_queries', 'grid_distance_queries'),
    'shortest_path_distances': ('.grid_queries', 'shortest_path_distances'),
    'distances_to_receptacle': ('.grid_queries', 'distances_to_receptacle'),
    'local_state_images': ('.local_maps', 'local_state_images'),
    'local_map': ('.local_maps', 'local_map'),
    'local_distance_map': ('.local_maps', 'local_distance_map'),
    'intention_maps': ('.intention_drawing', 'intention_maps'),
    'intention_map': ('.intention_drawing', 'intention_map'),
    'occupancy_maps': ('.occupancy', 'occupancy_maps'),
    'configuration_space': ('.occupancy', 'configuration_space'),
    'camera_geometry': ('.observation', 'camera_geometry'),
    'observation_update': ('.observation', 'observation_update'),
    'observation_update_sequences': ('.observation', 'observation_update_sequences'),
    'observe': ('.observation', 'observe'),
    'BatchedMapper': ('.mapper', 'BatchedMapper'),
    'RobotState': ('.mapper', 'RobotState'),
    'RobotArrays': ('.mapper', 'RobotArrays'),
    'state_output_visualizations': ('.visualization', 'state_output_visualizations'),
    'state_output_visualization': ('.visualization', 'state_output_visualization'),
    'state_visualization': ('.visualization', 'state_visualization'),
    'jet_table': ('.visualization', 'jet_table'),
}


def __getattr__(name):
    if name in _LAZY:
        mod, attr = _LAZY[name]
        return getattr(importlib.import_module(mod, __name__), attr)
    raise AttributeError(name)
