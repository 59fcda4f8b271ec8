"""Architecture table of the spatial-action-map Q-network (host side, no torch).

Mirrors the reference's ``DataParallel(FCN).state_dict()`` naming so checkpoints
interchange (reference: networks.py:7-14, resnet.py:52-91, policies.py:39).
The device-side layout (flat NHWC/OHWI parameter buffer) comes from the C-ABI
(`simq_param_tensor_info`); this module only knows reference names and shapes.
"""
import math

PREFIX = 'module.'
STATE_WIDTH = 96                       # envs.py:2010 Mapper.LOCAL_MAP_PIXEL_WIDTH
NUM_OUTPUT_CHANNELS = {                # envs.py:810 (pushing), envs.py:1090 (robots with hooks)
    'pushing_robot': 1, 'lifting_robot': 2, 'throwing_robot': 2, 'rescue_robot': 2,
}


def get_num_output_channels(robot_type):
    """envs.py:370-372."""
    if robot_type not in NUM_OUTPUT_CHANNELS:
        raise Exception(robot_type)
    return NUM_OUTPUT_CHANNELS[robot_type]


def get_action_space(robot_type):
    """envs.py:374-376."""
    return get_num_output_channels(robot_type) * STATE_WIDTH * STATE_WIDTH


# ---- what Mapper / OccupancyMap read of the robot classes and the camera (simq.BatchedMapper) ---------------------------------------
ROBOT_HALF_WIDTH = 0.03                # envs.py:803 Robot.HALF_WIDTH
ROBOT_BACKPACK_OFFSET = -0.0135        # envs.py:804 Robot.BACKPACK_OFFSET
ROBOT_BASE_LENGTH = {                  # envs.py:805 Robot.BASE_LENGTH, 1059 (5 mm blade), 1279 (6 mm offset)
    'pushing_robot': 0.065 + 0.005, 'lifting_robot': 0.065, 'throwing_robot': 0.065 + 0.006, 'rescue_robot': 0.065,
}
LOCAL_MAP_PIXELS_PER_METER = 96.0      # envs.py:2012 Mapper.LOCAL_MAP_PIXELS_PER_METER
SEG_VALUES = {                         # envs.py:1880-1889 Camera.SEG_VALUES
    'floor': 1.0 / 8, 'obstacle': 2.0 / 8, 'receptacle': 3.0 / 8, 'cube': 4.0 / 8,
    'robot_group_1': 5.0 / 8, 'robot_group_2': 6.0 / 8, 'robot_group_3': 7.0 / 8, 'robot_group_4': 8.0 / 8,
}


CUBE_WIDTH = 0.044                     # envs.py:25 VectorEnv.CUBE_WIDTH


def get_end_effector_location(robot_type):
    """The class's END_EFFECTOR_LOCATION: envs.py:807 (Robot), 1060 (PushingRobot), 1280 (ThrowingRobot)."""
    if robot_type not in ROBOT_BASE_LENGTH:
        raise Exception(robot_type)
    return ROBOT_BACKPACK_OFFSET + ROBOT_BASE_LENGTH[robot_type]


def get_robot_radius(robot_type):
    """The class's RADIUS: envs.py:807-808 (Robot), 1060-1061 (PushingRobot), 1280-1281 (ThrowingRobot)."""
    end_effector_location = get_end_effector_location(robot_type)
    return math.sqrt(ROBOT_HALF_WIDTH**2 + end_effector_location**2)


def _bn(name, c):
    return [(name + '.weight', (c,), 'bn_weight'), (name + '.bias', (c,), 'bn_bias'),
            (name + '.running_mean', (c,), 'bn_mean'), (name + '.running_var', (c,), 'bn_var'),
            (name + '.num_batches_tracked', (), 'bn_count')]


def state_spec(num_input_channels, num_output_channels):
    """Ordered [(reference key, reference shape, kind)] -- 138 entries."""
    spec = []
    r = PREFIX + 'resnet18.'
    spec.append((r + 'conv1.weight', (64, num_input_channels, 7, 7), 'conv_w'))
    spec += _bn(r + 'bn1', 64)
    inplanes = 64
    for li, planes in enumerate((64, 128, 256, 512), start=1):
        for bi in range(2):
            b = '%slayer%d.%d.' % (r, li, bi)
            cin = inplanes if bi == 0 else planes
            spec.append((b + 'conv1.weight', (planes, cin, 3, 3), 'conv_w'))
            spec += _bn(b + 'bn1', planes)
            spec.append((b + 'conv2.weight', (planes, planes, 3, 3), 'conv_w'))
            spec += _bn(b + 'bn2', planes)
            if bi == 0 and cin != planes:
                spec.append((b + 'downsample.0.weight', (planes, cin, 1, 1), 'conv_w'))
                spec += _bn(b + 'downsample.1', planes)
        inplanes = planes
    spec.append((r + 'fc.weight', (1000, 512), 'fc_w'))
    spec.append((r + 'fc.bias', (1000,), 'fc_b'))
    p = PREFIX
    spec.append((p + 'conv1.weight', (128, 512, 1, 1), 'conv_w'))
    spec.append((p + 'conv1.bias', (128,), 'conv_b'))
    spec += _bn(p + 'bn1', 128)
    spec.append((p + 'conv2.weight', (32, 128, 1, 1), 'conv_w'))
    spec.append((p + 'conv2.bias', (32,), 'conv_b'))
    spec += _bn(p + 'bn2', 32)
    spec.append((p + 'conv3.weight', (num_output_channels, 32, 1, 1), 'conv_w'))
    spec.append((p + 'conv3.bias', (num_output_channels,), 'conv_b'))
    return spec


TRAINABLE_KINDS = ('conv_w', 'conv_b', 'bn_weight', 'bn_bias')   # tensors that receive a gradient
