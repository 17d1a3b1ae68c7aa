"""The two rules behind the per-slot map sensors of a fused launch (include/cagpu.h: cagpu_tape_poses,
cagpu_laserscan_history), in plain NumPy.

THE POSE RULE.  Per agent slot, over the slots of a launch in step order:
  1. a tape row whose column 11 is >= 0 replaces position (columns 1, 2) and heading (column 10); step_num = column 11 + 1;
  2. any other row keeps the carried pose -- nothing else of such a row is read;
  3. where the slot's game_over is set and a table is attached, the pose becomes the START pose of the env's next episode
     (the table row of the auto-reset's case; the heading towards the goal, or the heading draw; zeros for an absent slot
     of a ragged table) and step_num 0;
  4. with a map key the slot's env_map entry is the map drawn at that auto-reset.

THE HISTORY RULE.  Row j of slot t's scan history is the index row of slot max(t - j, s), s the latest slot <= t whose
step_num is 0 (LaserScanSensor.py:84-88: the first measurement of an episode fills every row); a slot before the launch is
the history the launch found, slot -1 - r being its row r."""
import numpy as np


def table_case(env, k, n_cases, env_id_offset=0, case_stride=None, num_envs=None):
    """the table row env `env` loads at its k-th auto-reset (CaAutoReset)"""
    stride = num_envs if case_stride is None else case_stride
    return (env_id_offset + env + k * stride) % n_cases


def start_pose(case_rows, ragged=False, headings=None):
    """case_rows [N, 6] = px, py, gx, gy, pref_speed, radius -> (px, py, heading, radius) [N] of the reset state"""
    c = np.asarray(case_rows, np.float64)
    px, py, rad = c[:, 0].copy(), c[:, 1].copy(), c[:, 5].copy()
    hd = np.arctan2(c[:, 3] - c[:, 1], c[:, 2] - c[:, 0]) if headings is None else np.asarray(headings, np.float64).copy()
    if ragged:
        absent = ~(rad > 0.0)
        px[absent] = py[absent] = hd[absent] = rad[absent] = 0.0
    return px, py, hd, rad


def poses(start, rows, game_over, reset_count=None, next_start=None, next_map=None, env_map=None):
    """start: dict of pos_x, pos_y, heading, radius (float64 [E, N]) and step_num (int [E, N]) as the launch found them;
    rows [n, E, N, 12]; game_over [n, E]; reset_count [E] as the launch found it.
    next_start(e, k) -> (px, py, heading, radius) [N] of env e's episode k, or None: no table attached;
    next_map(e, k) -> the map drawn at env e's k-th auto-reset, or None: envs keep env_map [E].
    -> dict of [n, E, N] arrays (+ env_map [n, E] where env_map is given)"""
    rows, game_over = np.asarray(rows, np.float64), np.asarray(game_over)
    n, E, N = rows.shape[:3]
    cur = {f: np.array(start[f], dtype=np.float64) for f in ("pos_x", "pos_y", "heading", "radius")}
    sn = np.array(start["step_num"], dtype=np.int32)
    rc = np.zeros(E, np.int64) if reset_count is None else np.array(reset_count, dtype=np.int64)
    m = None if env_map is None else np.array(env_map, dtype=np.int32)
    out = {f: np.empty((n, E, N), np.float64) for f in cur}
    out["step_num"] = np.empty((n, E, N), np.int32)
    if m is not None:
        out["env_map"] = np.empty((n, E), np.int32)
    for t in range(n):
        c11 = rows[t, :, :, 11]
        moved = c11 >= 0
        cur["pos_x"][moved] = rows[t, :, :, 1][moved]
        cur["pos_y"][moved] = rows[t, :, :, 2][moved]
        cur["heading"][moved] = rows[t, :, :, 10][moved]
        sn[moved] = c11[moved].astype(np.int32) + 1
        if next_start is not None:
            for e in np.nonzero(game_over[t])[0]:
                rc[e] += 1
                px, py, hd, rad = next_start(int(e), int(rc[e]))
                cur["pos_x"][e], cur["pos_y"][e], cur["heading"][e], cur["radius"][e] = px, py, hd, rad
                sn[e] = 0
                if m is not None and next_map is not None:
                    m[e] = next_map(int(e), int(rc[e]))
        for f in cur:
            out[f][t] = cur[f]
        out["step_num"][t] = sn
        if m is not None:
            out["env_map"][t] = m
    return out


def history(idx, step_num, carried, t):
    """idx uint8 [n, A, B]: the slots' new index rows; step_num [n, A] of the pose ring; carried uint8 [A, H, B]: the history
    the launch found -> uint8 [A, H, B], the history after slot t's measurement"""
    idx, step_num, carried = np.asarray(idx), np.asarray(step_num), np.asarray(carried)
    A, H, B = carried.shape
    out = np.empty((A, H, B), np.uint8)
    for a in range(A):
        zeros = [u for u in range(t + 1) if step_num[u, a] == 0]
        s = zeros[-1] if zeros else None
        for j in range(H):
            u = t - j
            if s is not None and u < s:
                u = s
            out[a, j] = idx[u, a] if u >= 0 else carried[a, -1 - u]
    return out
