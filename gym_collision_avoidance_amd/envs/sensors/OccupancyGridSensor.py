from gym_collision_avoidance_amd.envs import Config
from .Sensor import Sensor


class OccupancyGridSensor(Sensor):
    """Ego-centred crop of the env's dynamic map (reference sensors/OccupancyGridSensor.py): a bool window of
    int(y_width / cell) x int(x_width / cell) map cells -- 50 x 50 with the reference's 5 m x 5 m on the 0.1 m map -- of the
    static grid with every agent drawn in as a disc (Map.add_agents_to_map; the agent's own disc included), zeros outside
    the map.  Computed for every agent of every env by the crop kernel (`cagpu_occupancy_grid`, csrc/cagpu_occ.inc);
    `sense` returns this agent's block of the env's window tensor (`env.occupancy_grid`).

    The window is anchored at its top-left map cell, i0 = floor(origin_r - (py + y_width / 2) / cell),
    j0 = floor(origin_c + (px - x_width / 2) / cell), and out[a, b] = map[i0 + a, j0 + b].  Where this differs from the
    reference, on purpose:
      * the reference computes the window's two corners independently and raises `ValueError: could not broadcast ...`
        whenever their floors span 49 or 51 cells, which happens at some "round" positions (e.g. px = -8.8 or py = 8.8 on
        the 16 m map); here the window is always H x W, and identical to the reference's wherever the reference returns one;
      * the reference class cannot be instantiated as shipped (it reads `Config` without importing it and sets no `name`, so
        Agent.sense could not store its result); here the sensor is named "occupancy_grid";
      * `grid_cell_size` ("currently ignored" in the reference) and `resize` (a copy) are kept for API parity only.
    All agents of a batch must agree on x_width / y_width (the windows are one tensor); set them with `set_args` before
    `env.reset()`."""

    def __init__(self):
        if not Config.USE_STATIC_MAP:
            raise AssertionError("OccupancyGridSensor needs Config.USE_STATIC_MAP (reference OccupancyGridSensor.py:16-18)")
        Sensor.__init__(self)
        self.name = "occupancy_grid"
        self.x_width = 5
        self.y_width = 5
        self.grid_cell_size = 0.01  # currently ignored (as in the reference)

    def sense(self, agents, agent_index, top_down_map=None):
        return self.resize(agents[agent_index].get_sensor_data(self.name))

    def resize(self, og_map):
        """a copy, as in the reference (:84-88)"""
        return None if og_map is None else og_map.copy()
