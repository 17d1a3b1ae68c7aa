"""Config classes of the OccupancyGridSensor tests (selected through GYM_CONFIG_PATH / GYM_CONFIG_CLASS like
tests/env_configs.py, on whose classes they build): the static map on, with 'occupancy_grid' in the observation."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location("_env_configs", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                            "env_configs.py"))
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)


class OccLaser4(_mod._Eval):       # map + laser scan + occupancy grid, four agents
    N_MAX = 4

    def __init__(self):
        self.USE_STATIC_MAP = True
        self.STATES_IN_OBS = ['is_learning', 'num_other_agents', 'dist_to_goal', 'heading_ego_frame', 'pref_speed',
                              'radius', 'other_agents_states', 'laserscan', 'occupancy_grid']
        _mod._Eval.__init__(self)


class Occ4(_mod._Eval):            # the occupancy grid alone beside the agent states
    N_MAX = 4

    def __init__(self):
        self.USE_STATIC_MAP = True
        self.STATES_IN_OBS = ['is_learning', 'num_other_agents', 'dist_to_goal', 'heading_ego_frame', 'pref_speed',
                              'radius', 'other_agents_states', 'occupancy_grid']
        _mod._Eval.__init__(self)
