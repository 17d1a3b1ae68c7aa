"""Config singleton, selected exactly like the reference does it (gym_collision_avoidance/envs/__init__.py:4-18):
env var GYM_CONFIG_PATH (default: this package's config.py) + GYM_CONFIG_CLASS (default "Config"), instantiated once
at import time; every module then does `from gym_collision_avoidance_amd.envs import Config`."""
import importlib.util
import os

_here = os.path.dirname(os.path.realpath(__file__))
gym_config_path = os.environ.get("GYM_CONFIG_PATH", os.path.join(_here, "config.py"))
gym_config_class = os.environ.get("GYM_CONFIG_CLASS", "Config")

_spec = importlib.util.spec_from_file_location(gym_config_class, gym_config_path)
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)
_cls = getattr(_mod, gym_config_class, None)
assert callable(_cls), "config class %r not found in %s" % (gym_config_class, gym_config_path)
Config = _cls()

# The sensor registry (`test_cases.sensor_dict`, reference test_cases.py:56-66) is completed here, once Config exists:
# OccupancyGridSensor joins it under "occupancy_grid", so that every way of importing `envs.test_cases` (the parent
# package runs first) finds the three sensors of the reference registered.
from gym_collision_avoidance_amd.envs import test_cases as _test_cases  # noqa: E402
from gym_collision_avoidance_amd.envs.sensors.OccupancyGridSensor import OccupancyGridSensor as _OccupancyGridSensor  # noqa: E402

_test_cases.sensor_dict.setdefault("occupancy_grid", _OccupancyGridSensor)
