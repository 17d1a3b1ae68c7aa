"""The rules of the episode metrics (include/cagpu.h CaEpMetrics) in float64 NumPy: what
cagpu_episode_metrics (csrc/cagpu_metrics.inc) is held to, bit for bit.

Every expression is a chain of single IEEE float64 operations in the order written here -- numpy's elementwise `*`, `+`, `-`
and `sqrt` are correctly rounded and never fused, math.remainder is the (exact) IEEE remainder --, and every sum is added
in slot order, so there is exactly one right answer per output.

    m = Metrics(E, N, capacity, dt, getting_close_range)
    m.process(rows, episode)        # rows [T, E, N, 12], episode [T, E]: T consecutive tape slots; any number of calls
    m.vals, m.cnts, m.head          # [E, C, N, 4] float64, [E, C, N, 4] int32, [E, C] int32 -- the kernel's buffers
    m.clear(mask)                   # a host-side reset of some envs

Columns 0 - 10 of a row whose column 11 is < 0 are never read."""
import math

import numpy as np

PATH, GAP, TURN, GAP_T = 0, 1, 2, 3          # vals[..., i]
MOVED, CLOSE, PARTNER = 0, 1, 2              # cnts[..., i]
TWO_PI = 2.0 * math.pi


class Metrics:
    def __init__(self, E, N, capacity, dt, getting_close_range):
        self.E, self.N, self.C = int(E), int(N), int(capacity)
        self.dt, self.close_range = np.float64(dt), np.float64(getting_close_range)
        self.vals = np.zeros((E, capacity, N, 4), np.float64)
        self.cnts = np.zeros((E, capacity, N, 4), np.int32)
        self.head = np.full((E, capacity), -1, np.int32)
        self.started = np.zeros(E, bool)
        self.id = np.zeros(E, np.int64)
        self._fresh(np.ones(E, bool), first=True)

    def _fresh(self, envs, first=False):
        """the carry of a new episode for the envs of the boolean mask"""
        E, N = self.E, self.N
        if first:
            self.seen, self.has_heading = np.zeros((E, N), bool), np.zeros((E, N), bool)
            self.px, self.py, self.rad, self.heading = (np.zeros((E, N)) for _ in range(4))
            self.path, self.turn = np.zeros((E, N)), np.zeros((E, N))
            self.min_gap, self.min_gap_t = np.full((E, N), np.inf), np.full((E, N), np.nan)
            self.moved, self.close = np.zeros((E, N), np.int32), np.zeros((E, N), np.int32)
            self.partner = np.full((E, N), -1, np.int32)
            return
        for x, v in ((self.seen, False), (self.has_heading, False), (self.px, 0.0), (self.py, 0.0), (self.rad, 0.0),
                     (self.heading, 0.0), (self.path, 0.0), (self.turn, 0.0), (self.min_gap, np.inf),
                     (self.min_gap_t, np.nan), (self.moved, 0), (self.close, 0), (self.partner, -1)):
            x[envs] = v

    def clear(self, mask=None):
        """a host-side reset of the envs of `mask` (None: all): carry gone, stamps -1; the running episode is discarded"""
        m = np.ones(self.E, bool) if mask is None else np.asarray(mask) != 0
        self._fresh(m)
        self.started[m] = False
        self.id[m] = 0
        self.head[m] = -1

    def _write(self, e):
        k = int(self.id[e])
        s = k % self.C
        self.vals[e, s, :, PATH], self.vals[e, s, :, GAP] = self.path[e], self.min_gap[e]
        self.vals[e, s, :, TURN], self.vals[e, s, :, GAP_T] = self.turn[e], self.min_gap_t[e]
        self.cnts[e, s, :, MOVED], self.cnts[e, s, :, CLOSE] = self.moved[e], self.close[e]
        self.cnts[e, s, :, PARTNER], self.cnts[e, s, :, 3] = self.partner[e], 0
        self.head[e, s] = k

    def _slot(self, e, row, k):
        one = np.zeros(self.E, bool)
        one[e] = True
        if self.started[e] and k != self.id[e]:
            self._write(e)
            self._fresh(one)
        self.id[e], self.started[e] = k, True
        mv = np.flatnonzero(row[:, 11] >= 0)
        if mv.size == 0:
            return
        r = row[mv]                       # (only moved rows are touched from here on)
        self.px[e, mv], self.py[e, mv], self.rad[e, mv] = r[:, 1], r[:, 2], r[:, 5]
        self.seen[e, mv] = True
        self.moved[e, mv] += 1
        vx, vy = r[:, 7], r[:, 8]
        self.path[e, mv] = self.path[e, mv] + np.sqrt(vx * vx + vy * vy) * self.dt
        for i, a in enumerate(mv):
            if self.has_heading[e, a]:
                self.turn[e, a] = self.turn[e, a] + math.fabs(math.remainder(float(r[i, 10] - self.heading[e, a]), TWO_PI))
        self.heading[e, mv], self.has_heading[e, mv] = r[:, 10], True
        px, py, rad = self.px[e], self.py[e], self.rad[e]
        # all pairs (moved a, every j) at once; the pairs that do not count (j == a, j not seen) are +inf -- a real gap is finite
        dx, dy = px[None, :] - px[mv, None], py[None, :] - py[mv, None]
        with np.errstate(invalid="ignore"):
            g = (np.sqrt(dx * dx + dy * dy) - rad[mv, None]) - rad[None, :]
        counts = self.seen[e][None, :] & (np.arange(self.N)[None, :] != mv[:, None])
        g = np.where(counts, g, np.inf)
        w = np.argmin(g, axis=1)          # (first minimum: ties go to the lowest j)
        for i, a in enumerate(mv):
            if not counts[i].any():
                continue
            gm = g[i, w[i]]
            self.close[e, a] += int(gm <= self.close_range)
            if gm < self.min_gap[e, a]:
                self.min_gap[e, a], self.partner[e, a], self.min_gap_t[e, a] = gm, w[i], r[i, 0]

    def process(self, rows, episode):
        rows, episode = np.asarray(rows), np.asarray(episode)
        T = rows.shape[0]
        assert rows.shape == (T, self.E, self.N, 12) and episode.shape == (T, self.E)
        if T == 0:
            return self
        for e in range(self.E):
            for t in range(T):
                self._slot(e, rows[t, e], int(episode[t, e]))
            self._write(e)                # the running episode's record: a later call overwrites it
        return self


def episode_table(rows, episode, dt, getting_close_range):
    """every episode of a tape, however many: {(env, k): (vals [N, 4], cnts [N, 4])} -- a ring nobody overwrites"""
    rows, episode = np.asarray(rows), np.asarray(episode)
    T, E, N = rows.shape[:3]
    out = {}
    for e in range(E):
        m = Metrics(1, N, 1, dt, getting_close_range)
        last = None
        for t in range(T):
            k = int(episode[t, e])
            if last is not None and k != last:
                m._write(0)
                out[(e, last)] = (m.vals[0, 0].copy(), m.cnts[0, 0].copy())
            m._slot(0, rows[t, e], k)
            last = k
        if last is not None:
            m._write(0)
            out[(e, last)] = (m.vals[0, 0].copy(), m.cnts[0, 0].copy())
    return out
