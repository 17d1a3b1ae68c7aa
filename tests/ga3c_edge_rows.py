"""Inputs that drive the GA3C-CADRL kernel (csrc/cagpu_ga3c.inc) onto every LSTM variant and to the edges of its input
range (test infrastructure, pure numpy; no test file by itself).

  tile_plan        the kernel's tile_of restated: which rows share a workgroup tile, and how tall the tile is
  laid_out_batch   rows in ARRAY ORDER such that, where array order is tile order (cagpu_ga3c_query, cagpu_ga3c without the
                   packed list), consecutive tiles carry chosen sequence-length patterns -- and with them the variant of
                   the LSTM step the tile must take: lstm_steps<NRB, ALL_LIVE>
  edge_rows        labelled classes of rows at the edges of the input range: saturated gates, the cell-state bound, tiny
                   values, garbage behind the sequence length, odd counts, the range guard's edge, NaN

tests/test_ga3c_edge_rows_host.py holds these builders to what they promise (so that the GPU tests are not vacuous),
tests/test_gpu_ga3c_edges.py runs them through the kernel."""
import os

import numpy as np

from tests import ga3c_f64_ref as f64

NO, XIN = 19, 138
FP16_MAX = 65504.0
DEFAULT_WEIGHTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym_collision_avoidance_amd",
                               "data", "ga3c_cadrl", "IROS18", "network_01900000.npz")


# ---------------------------------------------------------------- the tile plan
def tile_plan(n_rows, slots):
    """-> [(row0, tm)]: the tiles ga3c_kernel cuts n_rows rows into with `slots` resident workgroups (tile_of with
    force_tile = 0; tiles that start behind the last row leave at once and are not listed).  The last tile may reach
    behind n_rows: its remaining rows are padding."""
    blocks = (n_rows + 15) >> 4
    if blocks == 0:
        return []
    rounds = (blocks + 4 * slots - 1) // (4 * slots)
    tiles = rounds * slots
    lo = blocks // tiles
    rem = blocks - lo * tiles
    plan = []
    if lo < 2:
        t = 0
        while t * 32 < n_rows:
            plan.append((t * 32, 32))
            t += 1
        return plan
    for t in range(tiles):
        row0 = 16 * (t * lo + min(t, rem))
        if row0 < n_rows:
            plan.append((row0, 16 * (lo + (1 if t < rem else 0))))
    return plan


# ---------------------------------------------------------------- plausible rows
def plausible_x(rng, num):
    """X [n, 138] (the policy vector: obs[1:]) as a simulator produces it: num_other = num[i], the first num[i] slots
    filled with positions within +-8 m etc., the rest zero -- the rows of tests/test_gpu_ga3c_query.py::_rows"""
    num = np.asarray(num, dtype=np.int64)
    n = num.shape[0]
    x = np.zeros((n, XIN), np.float32)
    x[:, 0] = num
    x[:, 1] = rng.uniform(0.1, 12.0, n)
    x[:, 2] = rng.uniform(-np.pi, np.pi, n)
    x[:, 3] = rng.uniform(0.5, 1.5, n)
    x[:, 4] = rng.uniform(0.2, 0.8, n)
    x[:, 5:] = (_slots(rng, n) * (np.arange(NO)[None, :] < num[:, None])[..., None]).reshape(n, 7 * NO)
    return x


def _slots(rng, n):
    """[n, 19, 7] float32: p_parallel, p_orthogonal, v_parallel, v_orthogonal, radius, combined radius, distance"""
    return np.stack([rng.uniform(-8, 8, (n, NO)), rng.uniform(-8, 8, (n, NO)), rng.uniform(-1.5, 1.5, (n, NO)),
                     rng.uniform(-1.5, 1.5, (n, NO)), rng.uniform(0.2, 0.8, (n, NO)), rng.uniform(0.4, 1.6, (n, NO)),
                     rng.uniform(0.0, 10.0, (n, NO))], axis=-1).astype(np.float32)


# ---------------------------------------------------------------- laid-out batches
PATTERNS = ("uniform 19", "uniform 0", "uniform 1", "uniform 7", "mixed with 0 and 19", "one row of the last block differs",
            "the last row differs")
TALL_TILES = len(PATTERNS)


def laid_out_rows(slots, target_nrb):
    """the row count of laid_out_batch.  NRB 2: 32 * 7 + 5 rows are 32-row tiles at any `slots` >= 8.  NRB 3 / 4: a tile of
    more than two blocks needs lo = target_nrb - 1 >= 2 blocks in EVERY tile of the round and a remainder on top; the
    remainder is the number of tiles that get the extra block (the first ones), so 16 * (lo * slots + 7) + 5 rows give
    the first EIGHT tiles (7 + the block the 5 rows open) target_nrb blocks -- one per sequence-length pattern and one more --
    and every other tile lo blocks.  (With a remainder of one only tile 0 would be tall, and one tile cannot be both an
    ALL_LIVE and a select tile.)  The + 5 leaves the last tile partial."""
    if target_nrb == 2:
        return 32 * TALL_TILES + 5
    if target_nrb not in (3, 4):
        raise ValueError("target_nrb must be 2, 3 or 4")
    return 16 * ((target_nrb - 1) * slots + TALL_TILES) + 5


def _pattern_seq(p, real, rng):
    """the sequence lengths of a tile's `real` rows under pattern p"""
    s = np.full(real, NO, np.int64)
    if p == 1:
        s[:] = 0
    elif p == 2:
        s[:] = 1
    elif p == 3:
        s[:] = 7
    elif p == 4:
        s = rng.integers(0, NO + 1, real)
        s[0] = 0
        s[real - 1] = NO
    elif p == 5:
        first = 16 * ((real - 1) // 16)          # the last row block that holds real rows
        s[rng.integers(first, real)] = 11
    elif p == 6:
        s[real - 1] = 5
    return s


def laid_out_batch(slots, target_nrb, rng):
    """-> {"x": [rows, 138] float32, "tiles": [...]}: plausible rows whose tiles (tile_plan(rows, slots)) carry PATTERNS in
    turn, tile t pattern t % 7.  Per tile: row0, tm (its height), real (rows that are not padding), pattern (index into
    PATTERNS), tmax, all_live -- the kernel takes lstm_steps<tm / 16, all_live> for it: ALL_LIVE iff the shortest sequence
    among the tile's real rows is at least the longest (misc[2] >= misc[1]; padding rows count as 0 for the longest only)."""
    rows = laid_out_rows(slots, target_nrb)
    plan = tile_plan(rows, slots)
    seq = np.zeros(rows, np.int64)
    tiles = []
    for t, (row0, tm) in enumerate(plan):
        real = min(tm, rows - row0)
        p = t % len(PATTERNS)
        s = _pattern_seq(p, real, rng)
        seq[row0:row0 + real] = s
        tiles.append(dict(row0=row0, tm=tm, real=real, pattern=p, tmax=int(s.max()), all_live=bool(s.min() >= s.max())))
    return dict(x=plausible_x(rng, seq), tiles=tiles, target_nrb=target_nrb, slots=slots)


# ---------------------------------------------------------------- edge classes
SATURATED_SCALES = (10, 100, 1000, 5000)
COUNT_EDGES = (-3.0, -0.5, 0.4, 2.9, 18.999, 19.0, 19.5, 25.0, 40.0)
GUARD_SLOTS = (0, 5, 11, 18)        # columns 5 + 7 s + f: one in each quarter of the row (the four threads that load a row)
GUARD_FEATURES = (2, 0)             # v_parallel (input_std 1) and p_parallel (input_std 5); input_mean 0 for both
BELOW_FP16_MAX = float(np.nextafter(np.float32(FP16_MAX), np.float32(0)))     # 65503.996: the largest healthy float32


def raw_for(w, col, target):
    """the float32 raw input whose float32 normalisation (x - input_mean[col]) / input_std[col] is `target` -- exactly where
    that is possible (searched among the neighbours of the float64 solution), else the closest of no larger magnitude (a
    healthy value must not be rounded up onto the guard's bound); +-inf passes through"""
    m, s = np.float32(w["input_mean"][col]), np.float32(w["input_std"][col])
    if not np.isfinite(target):
        return np.float32(target)
    best = np.float32(np.float64(m) + np.float64(target) * np.float64(s))
    cand = [best]
    for _ in range(4):
        cand = [np.nextafter(cand[0], np.float32(-np.inf))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
    got = [np.float64((c - m) / s) for c in cand]
    err = [abs(g - np.float64(target)) if abs(g) <= abs(target) else np.inf for g in got]
    return cand[int(np.argmin(err))]


def _with_value(w, rng, targets):
    """plausible rows with all 19 slots live, one row per (target, feature, slot): that other-agent column holds the raw
    value which normalises to `target`"""
    combos = [(t, f, s) for t in targets for f in GUARD_FEATURES for s in GUARD_SLOTS]
    x = plausible_x(rng, np.full(len(combos), NO))
    for r, (t, f, s) in enumerate(combos):
        col = 5 + 7 * s + f
        x[r, col] = raw_for(w, col, t)
    return x


def _cell_bound_rows(w, rng, candidates=2000, keep=16):
    """19 identical slots per row: of `candidates` random slots (a plausible slot times 10^U(0, 3.5), so that the gates
    saturate) the `keep` whose float64 cell state grows largest -- |c| <= number of steps = 19 is the LSTM's bound, and the
    kernel's scaled cell state c' = -2 log2(e) c its documented 2^c' <= 2^55"""
    slot = _slots(rng, candidates)[:, 0, :] * (10.0 ** rng.uniform(0.0, 3.5, (candidates, 1))).astype(np.float32)
    x = plausible_x(rng, np.full(candidates, NO))
    x[:, 5:] = np.repeat(slot[:, None, :], NO, axis=1).reshape(candidates, 7 * NO)
    cmax = f64.evaluate(w, x)[2]
    best = np.argsort(-cmax, kind="stable")[:keep]
    return x[best]


def edge_rows(rng, weights=None):
    """-> {label: X [n <= 64, 138] float32}.  Finite classes (FINITE): the network's answer is defined and the kernel owes
    the float64 reference the project's bar.  Paired classes: "dirty tail" / "dirty tail twin" (row i of one is row i of the
    other with zeros behind num_other), "count edges" / "count edges clipped" (the same rows with the count replaced by
    clip(trunc(count), 0, 19)).  "at the guard" and the NaN classes must raise the range guard instead."""
    w = f64.load_weights(DEFAULT_WEIGHTS) if weights is None else weights
    mean, std = w["input_mean"], w["input_std"]
    out = {}
    out["plausible"] = plausible_x(rng, rng.integers(0, NO + 1, 64))
    # saturated gates: the other-agent columns scaled (normalised magnitude up to 5e4 at x5000: inside fp16's 65 504)
    for sc in SATURATED_SCALES:
        x = plausible_x(rng, rng.integers(1, NO + 1, 64))
        x[:, 5:] *= np.float32(sc)
        out["saturated x%d" % sc] = x
    out["cell bound"] = _cell_bound_rows(w, rng)
    # tiny: normalised other-agent values of magnitude 1e-9 .. 1e-4, both signs.  Where input_mean is 0 that is raw =
    # value * input_std; a column with a mean cannot come closer to it than an ulp of the mean: it holds the mean + the value
    # rounded to float32 (mostly the mean itself: normalised 0)
    n = 64
    x = plausible_x(rng, rng.integers(1, NO + 1, n))
    tiny = (10.0 ** rng.uniform(-9, -4, (n, 7 * NO))) * rng.choice([-1.0, 1.0], (n, 7 * NO))
    livecol = np.repeat(np.arange(NO)[None, :] < x[:, :1].astype(np.int64), 7, axis=1)
    x[:, 5:] = np.where(livecol, (mean[5:].astype(np.float64) + tiny * std[5:].astype(np.float64)).astype(np.float32), 0.0)
    out["tiny"] = x
    # dirty tail: finite garbage |x| <= 50 in the slots at and behind num_other; the twin has zeros there
    n = 32
    twin = plausible_x(rng, rng.integers(0, NO, n))       # (num_other <= 18: there is a tail)
    dirty = twin.copy()
    tail = np.repeat(np.arange(NO)[None, :] >= twin[:, :1].astype(np.int64), 7, axis=1)
    dirty[:, 5:] = np.where(tail, rng.uniform(-50.0, 50.0, (n, 7 * NO)).astype(np.float32), twin[:, 5:])
    out["dirty tail"], out["dirty tail twin"] = dirty, twin
    # count edges: fractional, negative and too-large counts in front of 19 filled slots
    x = plausible_x(rng, np.full(7 * len(COUNT_EDGES), NO))
    x[:, 0] = np.repeat(np.asarray(COUNT_EDGES, np.float32), 7)
    clipped = x.copy()
    clipped[:, 0] = np.clip(np.trunc(x[:, 0]), 0, NO)
    out["count edges"], out["count edges clipped"] = x, clipped
    # the range guard (fault word bit 1): healthy values just below fp16's largest number on both sides ...
    out["near the guard"] = _with_value(w, rng, (65000.0, -65000.0, BELOW_FP16_MAX, -BELOW_FP16_MAX))
    # ... and values that must raise it: the bound itself on both sides, +inf
    out["at the guard"] = _with_value(w, rng, (FP16_MAX, -FP16_MAX, np.inf))
    # NaN: in an other-agent column of a live slot / in a host column (1 .. 4)
    x = _with_value(w, rng, (0.0,))
    for r, (f, s) in enumerate([(f, s) for f in GUARD_FEATURES for s in GUARD_SLOTS]):
        x[r, 5 + 7 * s + f] = np.nan
    out["nan other"] = x
    x = plausible_x(rng, rng.integers(0, NO + 1, 8))
    x[np.arange(8), 1 + np.arange(8) % 4] = np.nan
    out["nan host"] = x
    return out


FINITE = ("plausible",) + tuple("saturated x%d" % s for s in SATURATED_SCALES) + (
    "cell bound", "tiny", "dirty tail", "dirty tail twin", "count edges", "count edges clipped", "near the guard")
RAISES_GUARD = ("at the guard", "nan other", "nan host")
