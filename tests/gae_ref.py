"""Generalised advantage estimation as include/cagpu.h (cagpu_gae) states it -- test infrastructure: the float32 loop, every
product and sum rounded on its own (gae32: what the kernel must equal bit for bit), the same loop in float64 (gae64), and
the fixtures with their branch counts."""
import numpy as np


def _gae(reward, value, last_value, live, done, game_over, gamma, gl, f):
    reward, value = np.asarray(reward, f), np.asarray(value, f)
    n, E, N = reward.shape
    live = np.asarray(live, bool)
    end = np.asarray(done, bool) | np.asarray(game_over, bool)[:, :, None]
    gamma, gl = f(gamma), f(gl)
    adv, ret = np.zeros((n, E, N), f), np.zeros((n, E, N), f)
    carry, nv = np.zeros((E, N), f), np.asarray(last_value, f).copy()
    for t in range(n - 1, -1, -1):
        nv = np.where(end[t], f(0), nv)
        carry = np.where(end[t], f(0), carry)
        delta = ((reward[t] + (gamma * nv).astype(f)).astype(f) - value[t]).astype(f)
        carry = np.where(live[t], (delta + (gl * carry).astype(f)).astype(f), f(0))
        adv[t] = carry
        ret[t] = np.where(live[t], (carry + value[t]).astype(f), f(0))
        nv = np.where(live[t], value[t], f(0))
    return adv, ret


def gae32(reward, value, last_value, live, done, game_over, gamma, lam):
    """[n, E, N] arrays (game_over [n, E], last_value [E, N]) -> (advantage, returns) float32"""
    gl = np.float32(gamma) * np.float32(lam)     # multiplied once, in float32
    return _gae(reward, value, last_value, live, done, game_over, gamma, gl, np.float32)


def gae64(reward, value, last_value, live, done, game_over, gamma, lam):
    """the same loop in float64, on float32 gamma and gamma * lambda"""
    gl = np.float32(gamma) * np.float32(lam)
    return _gae(reward, value, last_value, live, done, game_over, float(np.float32(gamma)), float(gl), np.float64)


def branches(live, done, game_over):
    """how often each branch of the rule is taken: dict(not_live, done, game_over_only, plain)"""
    live, done = np.asarray(live, bool), np.asarray(done, bool)
    over = np.broadcast_to(np.asarray(game_over, bool)[:, :, None], live.shape)
    return dict(not_live=int((~live).sum()), done=int((live & done).sum()), game_over_only=int((live & ~done & over).sum()),
                plain=int((live & ~done & ~over).sum()))


def synthetic(n, E, N, seed):
    """arrays that place an ending at t = 0, at t = n - 1 and at consecutive steps, with live gaps (where n and E * N leave
    room for them) -> dict of the seven inputs"""
    rng = np.random.default_rng(seed)
    f = np.float32
    reward = rng.normal(0.0, 1.0, (n, E, N)).astype(f)
    value = rng.normal(0.0, 2.0, (n, E, N)).astype(f)
    last_value = rng.normal(0.0, 2.0, (E, N)).astype(f)
    live = rng.random((n, E, N)) < 0.8
    done = rng.random((n, E, N)) < 0.15
    game_over = rng.random((n, E)) < 0.1
    flat = lambda x: x.reshape(n, E * N)
    EN = E * N
    flat(live)[:, 0] = True
    flat(done)[0, 0] = True                 # an ending at t = 0
    flat(done)[n - 1, 0] = True             # ... and at t = n - 1
    if n >= 3 and EN >= 2:
        c = 1
        flat(live)[:, c] = True
        flat(done)[0:2, c] = True           # consecutive endings
        flat(live)[n - 1, c] = False        # a gap at the end: last_value must not be read
    if n >= 5 and EN >= 3:
        flat(live)[2:4, 2] = False          # a gap in the middle
        flat(live)[4, 2] = True
    game_over[n - 1, E - 1] = True
    flat(live)[n - 1, EN - 1] = True
    flat(done)[n - 1, EN - 1] = False       # ended by game_over only
    return dict(reward=reward, value=value, last_value=last_value, live=live, done=done, game_over=game_over)
