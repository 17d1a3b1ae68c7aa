"""Replay: any episode of a batch from its (env, episode) address (core.BatchedSim.episode_start / replay; DESIGN.md "Replay").

Every random choice of an on-device auto-reset is a pure function of (seed, global env id, episode number): the table row,
the scenario of a case stream, the training-mode heading, the policy draw, the map of a map set.  An episode that the log
names can therefore be rebuilt after the fact: its start state from the kernels' own rules, then a CHILD batch that runs it
alone and hands back the records, the tape and the pictures the original run would have given.

The first half of this file is the host-only planner -- argument checks, the address formulas, the refusals, the
relabelling of the child's records -- pure functions over numpy arrays that read a simulator's HOST attributes only and run
without a GPU (tests/test_replay_host.py).  The second half, run() and Replay, drives the child.
"""
import math

import numpy as np

from . import _native as nat

# policies whose action of a step came from outside the step kernels (CaParams / ext_actions): the batch did not keep it
EXTERNAL_POLICIES = (nat.POL_EXTERNAL, nat.POL_LEARNING, nat.POL_LEARNING_GA3C)
CHUNK = 32   # steps of the child per launch and per host read


# ---------------------------------------------------------------- the address of an episode (host only)
def table_row(env_id_offset, env, episode, case_stride, n_cases):
    """the fixture-table row env `env` of a shard loads at its `episode`-th auto-reset (cagpu_rules.inc reset_case; the
    episode log's `case`): (env_id_offset + env + episode * case_stride) % n_cases -- ints or int arrays -> int64"""
    return (int(env_id_offset) + np.asarray(env, np.int64) + np.asarray(episode, np.int64) * int(case_stride)) % int(n_cases)


def stream_index(env_id_offset, env, episode):
    """the 64-bit case index of that episode under a case stream: (global env id << 32) | episode"""
    return ((int(env_id_offset) + np.asarray(env, np.int64)) << 32) | np.asarray(episode, np.int64)


def pairs(env, episode, num_envs, env_id_offset=0):
    """the (env, episode) arguments of episode_start() / replay() -> two int64 arrays [M]; ints or int sequences of equal
    length, env a LOCAL index in [0, num_envs), episode >= 0, the global id env_id_offset + env inside [0, 2^32)"""
    env, episode = np.atleast_1d(np.asarray(env)), np.atleast_1d(np.asarray(episode))
    for name, v in (("env", env), ("episode", episode)):
        if v.size and not np.issubdtype(v.dtype, np.integer):
            raise ValueError("replay: %s must hold integers, got %s" % (name, v.dtype))
    if env.ndim != 1 or env.shape != episode.shape:
        raise ValueError("replay: env and episode must be ints or 1-D sequences of equal length, got shapes %s and %s"
                         % (env.shape, episode.shape))
    env, episode = env.astype(np.int64), episode.astype(np.int64)
    if env.size:
        if env.min() < 0 or env.max() >= int(num_envs):
            raise ValueError("replay: env index outside [0, %d) (a LOCAL index, as episodes() reports it)" % int(num_envs))
        if episode.min() < 0 or episode.max() > 0x7FFFFFFF:
            raise ValueError("replay: episode numbers must lie in [0, 2^31)")
        g = env + int(env_id_offset)
        if g.min() < 0 or g.max() >= 1 << 32:
            raise ValueError("replay: global env ids (env_id_offset + env) must lie in [0, 2^32)")
    return env, episode


def refuse(sim, env, episode, host_policies=False, host_dynamics=False):
    """Raise ValueError, naming the reason, where an episode depended on something the batch did not keep.  Reads HOST
    attributes of `sim` only (no library call, no launch): _rvo, _variants, _plugin_words, _draw, _ar, _start."""
    if host_policies:
        raise ValueError("replay: user Python policies are queried on the host, step by step; their answers were not kept")
    if host_dynamics:
        raise ValueError("replay: a custom Dynamics integrates the motion on the host; its states were not kept")
    if sim._rvo is not None:
        raise ValueError("replay: stochastic RVO draws (set_rvo_stochastic) come from a generator whose state was not kept")
    if sim._variants:
        raise ValueError("replay: per-agent sensor variants (set_sensor_variants) are rewritten on the host after every "
                         "launch; the child batch does not carry them")
    words = sim._plugin_words
    w = np.zeros((len(env), sim.N), np.int64) if words is None else np.asarray(words, np.int64)[env]
    pol = (w >> nat.POLICY_SHIFT) & 0xF
    if sim._draw is not None:   # (any pool entry may have been drawn)
        pol = np.concatenate([pol.reshape(-1), (np.asarray(sim._draw["pool"], np.int64) >> nat.POLICY_SHIFT) & 0xF])
    if np.isin(pol, EXTERNAL_POLICIES).any():
        raise ValueError("replay: agents with an external policy (actions handed to step()): that would need an action record")
    if (((w >> nat.DYNAMICS_SHIFT) & 0xF) == nat.DYN_EXTERNAL).any():
        raise ValueError("replay: a custom Dynamics (external dynamics) integrates the motion outside the step kernels")
    if (episode >= 1).any() and sim._ar is None:
        raise ValueError("replay: an episode >= 1 without a fixture table or case stream: the batch never auto-reset")
    zero = env[episode == 0]
    if zero.size:
        if sim._start is None:
            raise ValueError("replay: episode 0 of an env that was never reset(): nothing was loaded")
        col = sim._start[:, 0, 0]
        col = col.cpu().numpy() if hasattr(col, "cpu") else np.asarray(col)
        if np.isnan(col[zero]).any():
            raise ValueError("replay: episode 0 of an env that was never reset(): nothing was loaded")


def plan(sim, env, episode, **host):
    """pairs() + refuse() + the address formulas -> dict of int64 arrays [M]: env, episode, global_env, row (the table /
    window row, the episode log's `case`; -1 without a table), case (the row, or the 64-bit stream index)"""
    ar = sim._ar
    off = 0 if ar is None else int(ar.env_id_offset)
    env, episode = pairs(env, episode, sim.E, off)
    refuse(sim, env, episode, **host)
    row = np.full(env.shape, -1, np.int64) if ar is None else table_row(off, env, episode, ar.case_stride, ar.n_cases)
    case = stream_index(off, env, episode) if sim._cstream is not None else row
    return {"env": env, "episode": episode, "global_env": env + off, "row": row, "case": case}


def relabel(child, env, episode, row, maps=None):
    """the child's episode-0 records (a drain: numpy arrays or torch tensors, `env` = the child's env i, one record per
    child env in any order) under the parent's labels -> the same dict, ordered by i, with env / episode / case (/ map)
    those of pair i"""
    ci = child["env"]
    host = np.asarray(ci.cpu() if hasattr(ci, "cpu") else ci).astype(np.int64)
    if sorted(host.tolist()) != list(range(len(env))):
        raise ValueError("replay: the child finished episode 0 of envs %s, expected one record for each of %d"
                         % (sorted(host.tolist()), len(env)))
    order = np.argsort(host, kind="stable")

    def pick(v):
        if not hasattr(v, "shape") or not len(getattr(v, "shape", ())):
            return v
        if hasattr(v, "device"):
            import torch
            return v[torch.as_tensor(order, device=v.device)]
        return np.asarray(v)[order]

    def like(v, ref):
        if hasattr(ref, "device"):
            import torch
            return torch.as_tensor(np.asarray(v, np.int64), device=ref.device)
        return np.asarray(v, np.int64)

    out = {k: pick(v) for k, v in child.items()}
    out["env"], out["episode"], out["case"] = like(env, ci), like(episode, ci), like(row, ci)
    if maps is not None:
        out["map"] = like(np.asarray(maps.cpu() if hasattr(maps, "cpu") else maps), ci)
    return out


def step_bound(cases, dt, near_goal_threshold, max_time_ratio):
    """the largest number of steps an episode on any of the cases [M, N, 6] can take: an agent is out of time once its
    budget max(dt, max_time_ratio * straight-line time) is used up, and every game-over rule ends the episode by then"""
    c = np.asarray(cases, np.float64)
    here = c[..., 5] > 0
    slt = (np.hypot(c[..., 0] - c[..., 2], c[..., 1] - c[..., 3]) - near_goal_threshold) / np.where(here, c[..., 4], 1.0)
    tr = np.where(here, np.maximum(dt, max_time_ratio * slt), dt)
    return int(math.ceil(float(tr.max()) / dt)) + 2 if c.size else 1


# ---------------------------------------------------------------- the child's run
def run(parent, env, episode, record=True, max_steps=None, keep_outputs=False, host=None):
    """BatchedSim.replay's body: start states, the child, its steps, its records -> Replay"""
    import torch
    start = parent.episode_start(env, episode, _host=host or {})
    pl = start["plan"]
    M = len(pl["env"])
    if M == 0:
        raise ValueError("replay: no (env, episode) pair given")
    child = parent._replay_child(start, record, CHUNK + 1)
    p = child.p
    if max_steps is None:
        max_steps = step_bound(start["cases"].cpu().numpy(), p.dt, p.near_goal_threshold, p.max_time_ratio)
    max_steps = int(max_steps)
    dev, N, W = child.device, child.N, child.W
    ended = torch.zeros((M,), dtype=torch.bool, device=dev)
    fin_obs = torch.zeros((M, N, W), dtype=torch.float32, device=dev)
    fin_flags = torch.zeros((M, N), dtype=torch.int32, device=dev)
    outs = ([], [], []) if keep_outputs else None
    # every policy answered inside the step kernel: CHUNK steps per launch through the ring, whose slots keep every step's
    # game_over and final block (a rollout's final block holds an env's LAST ending of the launch only, and a short episode
    # may end twice in one); otherwise (the GA3C-CADRL network runs between steps) one launch per step
    ring = child.lookahead_ok()
    if ring:
        child.enable_lookahead(CHUNK, fresh=True)
    logs, mets, have, steps = [], [], 0, 0
    while have < M:
        if steps >= max_steps:
            raise nat.CagpuError("replay: %d of %d episodes have not ended after max_steps = %d steps" % (M - have, M, max_steps))
        for _ in range(CHUNK):
            if ring:
                obs, rew, done, over = child.step_lookahead()
                fo, ff = child.lookahead_final()
            else:
                child.step()
                obs, rew, done, over = child._obs, child._rewards, child._done.bool(), child._game_over.bool()
                fo, ff = child._fin_obs, child._fin_flags
            newly = over & ~ended
            fin_obs = torch.where(newly[:, None, None], fo, fin_obs)
            fin_flags = torch.where(newly[:, None], ff, fin_flags)
            ended = ended | newly
            if outs is not None:
                for lst, v in zip(outs, (obs, rew, done)):
                    lst.append(v.clone())
        steps += CHUNK
        lg = child.episodes()    # (the one host read of the chunk: how many records are new)
        if lg["dropped"]:
            raise nat.CagpuError("replay: the child's episode log dropped %d records" % lg["dropped"])
        keep = lg["episode"] == 0
        logs.append({k: v[keep] for k, v in lg.items() if k != "dropped"})
        have += int(keep.sum())
        if record:
            mt = child.episode_metrics()
            keep = mt["episode"] == 0
            mets.append({k: v[keep] for k, v in mt.items() if k != "dropped"})
    child.sync()
    log = {k: torch.cat([c[k] for c in logs]) for k in logs[0]}
    rec = relabel(log, pl["env"], pl["episode"], pl["row"], start.get("map"))
    if record:
        met = {k: torch.cat([c[k] for c in mets]) for k in mets[0]}
        met = relabel(met, pl["env"], pl["episode"], pl["row"])
        for k, v in met.items():
            if k not in ("env", "episode", "case"):
                rec[k] = v
    out = None if outs is None else {"obs": torch.stack(outs[0]), "rewards": torch.stack(outs[1]), "done": torch.stack(outs[2])}
    return Replay(child, start, rec, fin_obs, fin_flags, out, bool(record))


class Replay(object):
    """M replayed episodes.  `env`, `episode`, `case` (int64 numpy [M]: the pairs and the table row -- or 64-bit stream index
    -- each ran on); `record`: dict of device tensors [M, ...] with the columns of episodes() (env, episode, case, steps,
    outcome, total_reward, time_to_goal, extra_time_to_goal, flags, with a map set `map`) and, when recorded, of
    episode_metrics(), under the parent's labels; `final_observation` float32 [M, N, W] and `final_flags` int32 [M, N]: the
    terminal step's; `outputs` (replay(keep_outputs=True)): obs / rewards / done of every step the child ran, [T, M, ...] --
    pair i's episode is steps 0 .. record["steps"][i] - 1, its terminal step handing out the NEXT reset's observation as
    every auto-reset does; `sim`: the child batch."""

    def __init__(self, sim, start, record, final_observation, final_flags, outputs, recorded):
        pl = start["plan"]
        self.sim, self.start = sim, start
        self.env, self.episode, self.case = pl["env"], pl["episode"], pl["case"]
        self.record, self.final_observation, self.final_flags, self.outputs = record, final_observation, final_flags, outputs
        self._recorded = recorded
        self._steps, self._tape = None, None

    def __len__(self):
        return len(self.env)

    @property
    def steps(self):
        """int64 numpy [M]: the length of every replayed episode (record["steps"], read back once)"""
        if self._steps is None:
            self._steps = self.record["steps"].cpu().numpy().astype(np.int64)
        return self._steps

    def _need_tape(self):
        if not self._recorded:
            raise nat.CagpuError("replay(record=False) kept no tape: no trajectories, histories or frames")

    def trajectories(self):
        """the child's tape restricted to its episode 0 -> {"rows": float64 [T, M, N, 12], "steps": int64 [M]}: T the longest
        episode, pair i's rows at t < steps[i]; rows past an episode's end carry -1 in column 11 (the tape's mark of a row
        without content)"""
        import torch
        self._need_tape()
        if self._tape is None:
            tp = self.sim.trajectories()
            T = int(self.steps.max())
            rows = tp["rows"][:T].clone()
            later = tp["episode"][:T] != 0
            rows[..., 11] = torch.where(later[:, :, None], torch.full_like(rows[..., 11], -1.0), rows[..., 11])
            self._tape = {"rows": rows, "steps": self.record["steps"]}
        return self._tape

    def histories(self, i):
        """pair i's episode as trajectory.episodes / env.episode_histories give one: a list over the agent slots of
        [steps, 11] numpy arrays"""
        from . import trajectory
        self._need_tape()
        tp = self.trajectories()
        n = int(self.steps[i])
        return trajectory.episodes(tp["rows"][:n, i:i + 1], torch_zeros_like_counter(tp["rows"][:n, i:i + 1]), 0)[0]

    def frames(self, i, every=1, size=(128, 128), limits=None, circles_along_traj=True, draw_map=True):
        """render_episode of pair i's episode on the child: uint8 device tensor [F, H, W, 3], frame j showing the first
        (j + 1) * every recorded steps, the last frame all of them"""
        import torch
        from . import render as rd
        self._need_tape()
        sim, n = self.sim, int(self.steps[i])
        ids = torch.as_tensor([int(i)], dtype=torch.int64, device=sim.device)
        lasts = rd.prefix_lasts(n, every)
        rows = sim._render_rows(ids, 0, n)
        F = len(lasts)
        zero = torch.zeros((F,), dtype=torch.int32, device=sim.device)
        return sim._render_launch(ids.expand(F), zero, zero, torch.as_tensor(lasts, dtype=torch.int32, device=sim.device), rows,
                                  size, limits, circles_along_traj, draw_map)


    # what env.replay() fills in: the names save_plots() gives its files
    plot_policy, plot_case_offset, plot_defaults = "policy", 0, {}

    def save_plots(self, directory, test_cases=None, **kw):
        """The reference's episode plots of the replayed episodes (visualize.py:27-38, :138-149), through the plot writer
        behind env.save_episode_plots(): `{test_case:03d}_{policy}_{N}agents.png` in `directory` -- test_case the table row
        (+ the env's test_case_index), N the agents present -- and a copy under `collisions/` for every episode that ended
        in a collision.  test_cases: the suite's number of every table row, where the table is a selection of a suite
        (default: the row itself).  Keywords: frames()'s.  Returns the list of PNG paths."""
        import os
        from . import render as rd
        kw = dict(self.plot_defaults, **kw)
        flags = self.record["flags"].cpu().numpy()
        outcome = self.record["outcome"].cpu().numpy()
        rows = self.record["case"].cpu().numpy()
        paths = []
        for i in range(len(self)):
            # (every = the episode's length: one frame, the whole episode)
            frame = self.frames(i, every=max(1, int(self.steps[i])), **kw)[-1].cpu().numpy()
            case = int(rows[i]) if test_cases is None else int(test_cases[int(rows[i])])
            name = "%03d_%s_%dagents" % (self.plot_case_offset + case, self.plot_policy,
                                         int(((flags[i] & nat.ABSENT) == 0).sum()))
            paths.append(rd.save_frames(os.path.join(directory, name + ".png"), frame))
            if int(outcome[i]) == 0:
                rd.save_frames(os.path.join(directory, "collisions", name + ".png"), frame)
        return paths


def torch_zeros_like_counter(rows):
    """an all-zero episode counter [T, S] for a block of tape rows [T, S, N, 12] that holds ONE episode per env"""
    import torch
    return torch.zeros(rows.shape[:2], dtype=torch.int32, device=rows.device)
