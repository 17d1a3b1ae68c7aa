"""TEST INFRASTRUCTURE.  The ADDRESS of an episode restated in NumPy: everything an on-device auto-reset decides is a pure
function of (seed, global env id g, episode number k) -- the fixture-table row, the case-stream index, the training-mode
heading, the policy draw.  core.BatchedSim.episode_start / replay.py and the two draw kernels (cagpu_heading_draw,
cagpu_policy_draw_at) must agree with this file bit for bit.  Also the three scenarios the outcome tests replay."""
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import policy_draw_ref as pdr  # noqa: E402


def table_row(env_id_offset, e, k, case_stride, n_cases):
    """(env_id_offset + e + k * case_stride) % n_cases, in Python integers (no width to overflow)"""
    return np.array([(int(env_id_offset) + int(ei) + int(ki) * int(case_stride)) % int(n_cases)
                     for ei, ki in zip(np.atleast_1d(e), np.atleast_1d(k))], np.int64)


def stream_index(env_id_offset, e, k):
    """(g << 32) | k in Python integers, as the int64 bit pattern of that 64-bit word (g >= 2^31 sets the sign bit)"""
    words = [(((int(env_id_offset) + int(ei)) << 32) | int(ki)) & 0xFFFFFFFFFFFFFFFF for ei, ki in zip(np.atleast_1d(e), np.atleast_1d(k))]
    return np.array([w - (1 << 64) if w >> 63 else w for w in words], np.int64)


def headings(heading_seed, g, k, num_agents):
    """[M, N]: -pi + 2 pi uniform_at(heading_seed, g, k, a), the expression of reset_heading (csrc/cagpu_rules.inc)"""
    return np.array([[-math.pi + (2.0 * math.pi) * pdr.uniform_at(int(heading_seed), int(gi), int(ki), a)
                      for a in range(num_agents)] for gi, ki in zip(g, k)], np.float64).reshape(len(g), num_agents)


def policy_bits(seed, g, k, present, cdf, pool_bits, ensure=-1):
    """[M, N] uint32: bits 6..11 of the pool entry every present slot ends up with, 0xFFFFFFFF for an absent slot"""
    idx = pdr.draw_batch(int(seed), g, k, present, cdf, ensure)
    bits = np.asarray(pool_bits, np.int64)[np.maximum(idx, 0)] & pdr.DRAW_BITS
    return np.where(idx >= 0, bits, 0xFFFFFFFF).astype(np.uint32)


# ---------------------------------------------------------------- three scenarios, one per outcome
OUTCOME_COLLISION, OUTCOME_ALL_AT_GOAL, OUTCOME_STUCK = 0, 1, 2
POL_RVO, POL_NONCOOP, POL_STATIC = 0, 1, 2   # (CA_POL_*)
OUTCOME_MAX_TIME_RATIO = 1.5


def outcome_table():
    """-> (table [3, 2, 6], policies [3, 2], outcomes [3]): row 0, two non-cooperative agents head-on: they collide; row 1,
    two lone short trips far from each other: both arrive; row 2, an RVO agent whose goal lies under a static agent of
    radius 0.5: it cannot get within the goal threshold and runs out of time.  A batch of three envs with
    case_stride = 3 keeps env e on row e in every episode, so that the policies (per env slot) stay with their rows."""
    t = np.zeros((3, 2, 6))
    t[0, 0] = (-1.0, 0.0, 1.0, 0.0, 1.0, 0.3)
    t[0, 1] = (1.0, 0.0, -1.0, 0.0, 1.0, 0.3)
    t[1, 0] = (-3.0, -3.0, -2.3, -3.0, 1.0, 0.2)
    t[1, 1] = (3.0, 3.0, 3.0, 2.3, 1.0, 0.2)
    t[2, 0] = (-1.5, 0.0, 0.5, 0.0, 1.0, 0.2)
    t[2, 1] = (0.5, 0.0, 0.5, 0.05, 1.0, 0.5)
    pol = np.array([[POL_NONCOOP, POL_NONCOOP], [POL_RVO, POL_RVO], [POL_RVO, POL_STATIC]], np.int64)
    return t, pol, np.array([OUTCOME_COLLISION, OUTCOME_ALL_AT_GOAL, OUTCOME_STUCK], np.int64)
