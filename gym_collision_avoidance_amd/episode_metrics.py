"""The host side of the episode metrics (include/cagpu.h CaEpMetrics): which slots of the per-env rings hold episodes that
are new since the last drain, which were overwritten first, and what a record's words mean.

Pure functions over arrays, numpy arrays and torch tensors alike (any device), like episodes.py -- whose slot rule this
is: cagpu_episode_metrics writes `vals` [E, C, N, 4] float64, `cnts` [E, C, N, 4] int32 and the stamps `head` [E, C] int32,
env e's k-th episode in slot k % C, stamped with k; the caller keeps a read cursor per env."""
from . import episodes

VAL_PATH, VAL_GAP, VAL_TURN, VAL_GAP_T = 0, 1, 2, 3
CNT_MOVED, CNT_CLOSE, CNT_PARTNER = 0, 1, 2
FLOAT_COLUMNS = ("path_length", "min_gap", "turn_sum", "min_gap_t")
INT_COLUMNS = ("moved_steps", "close_steps", "min_gap_partner")


def select(head, cursor, rc):
    """episodes.select on the metrics' stamps: head int [E, C], cursor int [E] (first episode index not drained yet), rc
    int [E] (the episodes the env has finished at the step last handed out)
    -> (env [M], k [M], slot [M], dropped: int, new_cursor [E]), ordered by (env, k).  A finished episode whose slot carries
    another stamp -- overwritten by a later episode, the RUNNING one included: it takes its slot with its first processed
    step -- counts as dropped."""
    return episodes.select(head[:, :, None], cursor, rc)


def gather(vals, cnts, env, k, slot):
    """the records select() chose -> dict: env, episode [M] int64; path_length, min_gap, turn_sum, min_gap_t [M, N] float64;
    moved_steps, close_steps, min_gap_partner [M, N] int32"""
    v, c = vals[env, slot], cnts[env, slot]
    out = {"env": env, "episode": k}
    for i, n in enumerate(FLOAT_COLUMNS):
        out[n] = v[..., i]
    for i, n in enumerate(INT_COLUMNS):
        out[n] = c[..., i]
    return out


def drain(vals, cnts, head, cursor, rc):
    """select() + gather(): -> (dict of the new episodes + "dropped", new_cursor)"""
    env, k, slot, dropped, new_cursor = select(head, cursor, rc)
    out = gather(vals, cnts, env, k, slot)
    out["dropped"] = dropped
    return out, new_cursor


def clear(head, cursor, carry, mask=None):
    """an explicit reset of the envs of mask ([E], or None = all): their carry ([E, bytes per env]) is zeroed -- the running
    episode is forgotten --, their stamps go to -1 and their cursors to 0: undrained records of those envs are discarded.
    In place."""
    if mask is None:
        head[:, :] = -1
        cursor[:] = 0
        carry[:, :] = 0
        return
    m = mask != 0   # (where-forms: no boolean indexing, which would synchronise with a device)
    head[:, :] = episodes._where(m[:, None], head * 0 - 1, head)
    cursor[:] = episodes._where(m, cursor * 0, cursor)
    carry[:, :] = episodes._where(m[:, None], carry * 0, carry)


def join(log, met):
    """the metric columns for the records of an episode-log drain (episodes.drain / suite_columns dicts, numpy) whose
    (env, episode) is in the metrics' drain `met` as well -> (index into log [J], dict of the columns [J, N])"""
    import numpy as np
    key = {(int(e), int(k)): i for i, (e, k) in enumerate(zip(np.asarray(met["env"]), np.asarray(met["episode"])))}
    pairs = [(i, key[(int(e), int(k))]) for i, (e, k) in enumerate(zip(np.asarray(log["env"]), np.asarray(log["episode"])))
             if (int(e), int(k)) in key]
    li = np.array([p[0] for p in pairs], np.int64)
    mi = np.array([p[1] for p in pairs], np.int64)
    return li, {n: np.asarray(met[n])[mi] for n in FLOAT_COLUMNS + INT_COLUMNS}
