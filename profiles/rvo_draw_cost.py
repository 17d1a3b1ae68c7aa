#!/usr/bin/env python3
"""What the RVO draw (CaRvoDraw, BatchedSim.set_rvo_draw) costs at 4096 x 10, fixture cases with auto-reset, microseconds per
step from device events: the median, fastest and slowest of 12 blocks, one JSON line per figure --

  without a draw   ca_kernel (pipeline=False) by single launches and by rollout(20): run once in a checkout of the parent commit
                   and once in this tree, alternating, to see what the feature costs a batch that does not use it
  with `draw`      every agent masked with noise_std = 0 (both Philox blocks and the normal are computed, the dynamics are those
                   of no draw): the draw's own cost; then c = -0.6, T = 1, every second agent masked: single launches,
                   rollout(20), a look-ahead ring of 20, and set_rvo_stochastic (torch draws before each of 20 single launches)
                   on the same configuration

    python profiles/rvo_draw_cost.py <root of the tree to import> <label> [draw]
"""
import json
import os
import sys

tree, label = os.path.abspath(sys.argv[1]), sys.argv[2]
with_draw = len(sys.argv) > 3
sys.path.insert(0, tree)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gym_collision_avoidance_amd import _native as nat, core  # noqa: E402

E, N, K, BLOCKS = 4096, 10, 20, 12
table = np.load(os.path.join(tree, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]


def sim(pipeline):
    s = core.BatchedSim(core.make_params(E, N), pipeline=pipeline)
    s.set_plugins(nat.POL_RVO)
    s.set_fixture_table(table)
    s.reset(table[np.arange(E) % table.shape[0]])
    return s


def timed(fn, steps_per_call, calls):
    """median / min / max us per step over BLOCKS blocks of `calls` calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(BLOCKS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / (calls * steps_per_call))
    out.sort()
    return dict(median=round(out[len(out) // 2], 3), min=round(out[0], 3), max=round(out[-1], 3))


def emit(what, r, s):
    r.update(label=label, what=what, kernel=nat.lib().cagpu_last_kernel().decode())
    print(json.dumps(r), flush=True)
    s.check_faults()


s = sim(False)
emit("ca_kernel single step, no draw", timed(s.step, 1, 200), s)
emit("ca_kernel rollout(20), no draw", timed(lambda: s.rollout(K), K, 10), s)

if with_draw:
    mask = np.zeros((E, N), bool)
    mask[:, ::2] = True
    s = sim(True)
    s.set_rvo_draw(12345, heading_noise=np.ones((E, N), bool), noise_std=0.0)
    emit("draw in kernel, every agent masked, noise_std = 0 (the dynamics of no draw): single step", timed(s.step, 1, 200), s)
    emit("draw in kernel, every agent masked, noise_std = 0 (the dynamics of no draw): rollout(20)", timed(lambda: s.rollout(K), K, 10), s)
    s = sim(True)
    s.set_rvo_draw(12345, heading_noise=mask, collab_coeff=-0.6, anti_collab_t=1.0)
    emit("draw in kernel: single step", timed(s.step, 1, 200), s)
    emit("draw in kernel: rollout(20)", timed(lambda: s.rollout(K), K, 10), s)
    s.enable_lookahead(K, fresh=True)

    def ring():
        for _ in range(K):
            s.step_lookahead()
    emit("draw in kernel: ring of 20", timed(ring, K, 10), s)
    s.enable_lookahead(0)
    s = sim(True)
    s.set_rvo_stochastic(heading_noise=mask, collab_coeff=-0.6, anti_collab_t=1.0, seed=5)
    emit("set_rvo_stochastic: 20 x (torch draws + single launch)", timed(lambda: s.rollout(K), K, 10), s)
