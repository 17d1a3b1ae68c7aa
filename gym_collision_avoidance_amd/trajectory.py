"""Host-side assembly of the device trajectory tape (core.BatchedSim.trajectories, include/cagpu.h CaTraj).

The tape is step-major -- rows [T, E, N, 12], one row per (step, env, agent slot), column 11 the row's index in the
agent's history or -1 where the agent did not move -- because that is the order the step kernels produce it in.  What the
reference's tooling reads is agent-major: `Agent.global_state_history[:step_num]`, a [len, 11] array per agent and
episode (agent.py:257-289).  `episodes()` turns one into the other; `dataset_samples()` builds the per-timestep records
of the reference's trajectory dataset (experiments/src/run_trajectory_dataset_creator.py) from two such histories.
Pure numpy: no GPU, no torch import (device tensors are accepted and copied to the host).
"""
import numpy as np

COLUMNS = ("t", "px", "py", "gx", "gy", "radius", "pref_speed", "vx", "vy", "speed", "heading")
T_, PX, PY, GX, GY, RADIUS, PREF_SPEED, VX, VY, SPEED, HEADING, INDEX = range(12)


def _host(x):
    if x is None:
        return None
    if hasattr(x, "detach"):     # a torch tensor, wherever it lives
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def episodes(rows, episode, env, epoch=None):
    """The episodes of ONE env of a tape, in the order they were run.

    rows [T, E, N, 12], episode [T, E] (the env's auto-reset count as each step started), epoch [T, E] or None (its
    host-side resets, see BatchedSim.trajectories).  Returns a list over episodes; each episode is a list over the N
    agent slots of float64 [len, 11] arrays -- the reference's `global_state_history[:step_num]` of that agent: the rows
    with column 11 >= 0, ordered by it, without it.  A slot that never moved in the episode (an absent slot of a ragged
    batch, an agent that was done from the start) gives [0, 11].  A new episode starts wherever `episode` or `epoch`
    differs from the step before.  The last episode of the list is the one still running (or cut by the tape's end)."""
    rows, episode, epoch = _host(rows), _host(episode), _host(epoch)
    if rows.ndim != 4 or rows.shape[3] != 12:
        raise ValueError("rows of shape %s: expected [T, E, N, 12]" % (rows.shape,))
    T, E, N = rows.shape[:3]
    if episode.shape != (T, E) or (epoch is not None and epoch.shape != (T, E)):
        raise ValueError("episode / epoch must be [T, E] = [%d, %d]" % (T, E))
    if T == 0:
        return []
    r = rows[:, env]
    key = episode[:, env].astype(np.int64)
    if epoch is not None:
        key = key + (epoch[:, env].astype(np.int64) << 32)
    cuts = [0] + [int(s) for s in np.nonzero(key[1:] != key[:-1])[0] + 1] + [T]
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        agents = []
        for a in range(N):
            seg = r[lo:hi, a]
            seg = seg[seg[:, INDEX] >= 0]
            order = np.argsort(seg[:, INDEX], kind="stable")
            agents.append(np.ascontiguousarray(seg[order, :11], dtype=np.float64))
        out.append(agents)
    return out


def _wrap(a):
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def dataset_samples(history_ego, history_other, goal, dt, horizon_secs=3.0, initial_heading=None, angular="delta"):
    """One record per row of the ego agent's history -- the fields of the reference's two-agent trajectory dataset:

      control_command   [2]     the ego's linear speed (column `speed`) and angular speed at this row
      predicted_cmd     [1,h,2] the same pair for this row and the following ones, h = min(rows left, horizon steps)
      future_positions  [h,2]   the ego's positions over the same rows
      pedestrian_state  dict    position [2] and velocity [2] of the other agent at this row
      robot_state       [3]     the ego's px, py, heading
      goal_position     [2]     `goal`

    horizon steps = int(horizon_secs / dt); the window is clipped at the end of the episode.
    angular = "delta" (default): angular speed = the change of heading over the step, wrapped to [-pi, pi), divided by dt;
    the heading before the first row is `initial_heading` (None: the first row's own heading, i.e. no turn in step 0 --
    the log does not hold the reset heading).  angular = "heading": the logged heading itself divided by dt, which is
    what the reference's script computes from column 10 of the history.
    The other agent's history may be shorter than the ego's (it was done earlier): beyond its end it stands at its last
    logged position with zero velocity (the reference reads the zero rows of its preallocated log there)."""
    ego = np.asarray(history_ego, dtype=np.float64).reshape(-1, 11)
    other = np.asarray(history_other, dtype=np.float64).reshape(-1, 11)
    goal = np.asarray(goal, dtype=np.float64).reshape(2)
    n = ego.shape[0]
    steps = int(horizon_secs / dt)
    if angular == "heading":
        ang = ego[:, HEADING] / dt
    elif angular == "delta":
        h0 = ego[0, HEADING] if (initial_heading is None and n) else initial_heading
        prev = np.concatenate([[h0], ego[:-1, HEADING]]) if n else np.zeros((0,))
        ang = _wrap(ego[:, HEADING] - prev) / dt
    else:
        raise ValueError("angular must be 'delta' or 'heading', got %r" % (angular,))
    cmd = np.stack([ego[:, SPEED], ang], axis=1)
    out = []
    for t in range(n):
        hi = min(n, t + steps)
        if t < other.shape[0]:
            ped_pos, ped_vel = other[t, [PX, PY]].copy(), other[t, [VX, VY]].copy()
        elif other.shape[0]:
            ped_pos, ped_vel = other[-1, [PX, PY]].copy(), np.zeros(2)
        else:
            ped_pos, ped_vel = np.full(2, np.nan), np.zeros(2)
        out.append({"control_command": cmd[t].copy(), "predicted_cmd": cmd[t:hi][None].copy(),
                    "future_positions": ego[t:hi, [PX, PY]].copy(),
                    "pedestrian_state": {"position": ped_pos, "velocity": ped_vel},
                    "robot_state": ego[t, [PX, PY, HEADING]].copy(), "goal_position": goal.copy()})
    return out
