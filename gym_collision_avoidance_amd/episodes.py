"""The host side of the episode log (include/cagpu.h CaEpLog): which slots of the per-env rings hold episodes that are new
since the last drain, which episodes were overwritten before anybody read them, and what a record's words mean.

Everything here is a pure function over arrays and works on numpy arrays and torch tensors alike (any device): the step
kernels write `rows` [E, C, N, 4] float64 and `head` [E, C, 4] int32, env e's k-th finished episode in slot k % C, stamped
with k in head[e, k % C, 0]; the caller keeps a read cursor per env (the index of the first episode not yet drained)."""
import numpy as np

HEAD_K, HEAD_STEPS, HEAD_CASE, HEAD_OUTCOME = 0, 1, 2, 3
ROW_REWARD, ROW_TIME, ROW_EXTRA, ROW_FLAGS = 0, 1, 2, 3
# CaEpLog.head[..., 3]: the env_stats[1..3] classification, in run_episode's words (experiments/src/env_utils.py:56-87)
OUTCOMES = ("collision", "all_at_goal", "stuck")
ABSENT = 1 << 16   # CA_ABSENT


def _is_torch(x):
    return hasattr(x, "device") and hasattr(x, "dtype") and not isinstance(x, np.ndarray)


def _repeat(x, n):
    return x.repeat_interleave(n) if _is_torch(x) else np.repeat(x, n)


def _arange(n, like):
    if _is_torch(like):
        import torch
        return torch.arange(n, dtype=torch.int64, device=like.device)
    return np.arange(n, dtype=np.int64)


def _i64(x):
    if _is_torch(x):
        import torch
        return x.to(torch.int64)
    return np.asarray(x).astype(np.int64)


def _where(c, a, b):
    if _is_torch(c):
        import torch
        return torch.where(c, a, b)
    return np.where(c, a, b)


def select(head, cursor, rc):
    """Which records does a drain return?  head: int [E, C, 4] (only the stamps head[..., 0] are read), cursor: int [E] (first
    episode index not drained yet), rc: int [E] (the env's reset count at the step last handed out = the number of episodes
    it has finished).  The candidates of env e are k in [max(cursor, rc - C), rc); a candidate whose slot is not stamped
    with k (overwritten by a later episode -- a ring that looked further ahead than the capacity covers --, or never
    written) counts as dropped, and so does everything in [cursor, rc - C).
    -> (env [M], k [M], slot [M], dropped: int, new_cursor [E]), the M records ordered by (env, k); all int64."""
    C = int(head.shape[1])
    cursor, rc = _i64(cursor), _i64(rc)
    lo = _where(rc - C > cursor, rc - C, cursor)
    n = rc - lo
    n = _where(n > 0, n, n * 0)
    lost = lo - cursor            # (>= 0: lo >= cursor)
    lost = _where((lost > 0) & (rc > cursor), lost, lost * 0)
    env_ids = _arange(int(head.shape[0]), head)
    env = _repeat(env_ids, n)
    start = n.cumsum(0) - n
    k = _repeat(lo - start, n) + _arange(int(env.shape[0]), head)
    slot = k % C
    ok = _i64(head[env, slot, HEAD_K]) == k
    dropped = int(lost.sum()) + int((~ok).sum())
    new_cursor = _where(rc > cursor, rc, cursor)
    return env[ok], k[ok], slot[ok], dropped, new_cursor


def flag_words(column):
    """column 3 of the rows (float64 whose 8 bytes hold the agent's flag word in the low 32 bits, zeros above) -> the words
    as int32 bit patterns (what CaFinal.flags / CaState.flags hold, what nat.decode_flags reads)"""
    if _is_torch(column):
        import torch
        return column.contiguous().view(torch.int64).to(torch.int32)
    return np.ascontiguousarray(column).view(np.int64).astype(np.int32)


def gather(rows, head, env, k, slot):
    """the records select() chose -> dict: env, episode, case, steps, outcome [M] int64; total_reward, time_to_goal,
    extra_time_to_goal [M, N] float64 (as stored: the addends of env_stats[5..7]); flags [M, N] int32"""
    h = _i64(head[env, slot])
    r = rows[env, slot]
    return {"env": env, "episode": k, "case": h[:, HEAD_CASE], "steps": h[:, HEAD_STEPS], "outcome": h[:, HEAD_OUTCOME],
            "total_reward": r[..., ROW_REWARD], "time_to_goal": r[..., ROW_TIME], "extra_time_to_goal": r[..., ROW_EXTRA],
            "flags": flag_words(r[..., ROW_FLAGS])}


def map_column(k, given_ep, given_map, key_from, keyed, drawn):
    """Which map of a map set did an episode run on?  All arguments per record [M]: k the episode's index, given_ep /
    given_map the episode the env was in when the host last GAVE it a map (reset, set_env_map) and that map, key_from the
    first episode whose map was decided under the key now in force (0: since the env's reset; a key replaced while the env
    was in episode c: c + 1), keyed whether that key is != 0, drawn the draw of (key, env, k) -- CaMapSet.map_seed's rule,
    read only where it applies.  The episode an env was given its map in ran on that map; a later one on its draw, or,
    without a key, still on the given map -- both only if the key in force has been since that episode's map was decided.
    Everything else is -1: the index cannot be known, and a wrong one is never reported.  -> int64 [M]"""
    k, given_ep, key_from = _i64(k), _i64(given_ep), _i64(key_from)
    given_map, drawn = _i64(given_map), _i64(drawn)
    unknown = k * 0 - 1
    later = (k > given_ep) & (k >= key_from)
    if keyed:
        after = _where(later, drawn, unknown)
    else:   # no draws since episode key_from - 1: the given map still holds if it was given in or after that episode
        after = _where(later & (key_from <= given_ep + 1), given_map, unknown)
    return _where(k == given_ep, given_map, after)


def drain(rows, head, cursor, rc):
    """select() + gather(): -> (dict of the new episodes + "dropped", new_cursor)"""
    env, k, slot, dropped, new_cursor = select(head, cursor, rc)
    out = gather(rows, head, env, k, slot)
    out["dropped"] = dropped
    return out, new_cursor


def clear(head, cursor, mask=None):
    """an explicit reset zeroes the reset count of the envs it touches (mask: [E] or None = all): their cursors go to 0,
    their stamps to -1 -- undrained records of those envs are discarded.  In place."""
    if mask is None:
        head[:, :, HEAD_K] = -1
        cursor[:] = 0
        return
    m = mask != 0   # (where-forms: no boolean indexing, which would synchronise with a device)
    stamps = head[:, :, HEAD_K]
    head[:, :, HEAD_K] = _where(m[:, None], stamps * 0 - 1, stamps)
    cursor[:] = _where(m, cursor * 0, cursor)


def outcome_of(flags):
    """the kernel's classification (CaEpLog.head[..., 3]) recomputed from an episode's flag words [..., N]: 0 = some agent in
    collision, 1 = every slot at its goal (absent slots carry the bit), 2 = stuck -- int64 [...]"""
    f = _i64(flags)
    coll = ((f & 4) != 0).any(-1)
    goal = ((f & 1) != 0).all(-1)
    one, two = _i64(coll) * 0 + 1, _i64(coll) * 0 + 2
    return _where(coll, one * 0, _where(goal, one, two))


def suite_columns(ep):
    """a drained dict (numpy) -> the columns of run_suite's rows (experiments/run_full_test_suite.py): num_agents (slots
    without CA_ABSENT), the three per-agent arrays with absent slots 0, total_time_to_goal, collision / all_at_goal /
    any_stuck, outcome (the three strings)"""
    fl = np.asarray(ep["flags"]).astype(np.int64)
    here = (fl & ABSENT) == 0
    coll, goal = ((fl & 4) != 0) & here, ((fl & 1) != 0) | ~here
    per = {n: np.where(here, np.asarray(ep[n], np.float64), 0.0) for n in ("total_reward", "time_to_goal", "extra_time_to_goal")}
    oc = np.asarray(ep["outcome"]).astype(np.int64)
    out = {"env": np.asarray(ep["env"]).astype(np.int64), "episode": np.asarray(ep["episode"]).astype(np.int64),
           "test_case": np.asarray(ep["case"]).astype(np.int64), "num_agents": here.sum(-1).astype(np.int64),
           "steps": np.asarray(ep["steps"]).astype(np.int64)}
    out.update(per)
    out["total_time_to_goal"] = per["time_to_goal"].sum(-1) if fl.size else np.zeros((0,), np.float64)
    out["collision"] = oc == 0
    out["all_at_goal"] = oc == 1
    out["any_stuck"] = (~coll & ~goal).any(-1) if fl.size else np.zeros((0,), bool)
    out["outcome"] = np.array([OUTCOMES[i] for i in oc], dtype=object)
    out["dropped"] = int(ep["dropped"])
    return out
