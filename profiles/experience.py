"""What an on-policy batch costs: BatchedSim.collect(20) + Experience.gae against the way the same arrays are produced
without the feature -- the loop of experiments/collect_regression_dataset.py::fill (clone, step, mask) with
torch.multinomial for the sample and a reversed torch loop for GAE -- at 4096 x 20 (bench config 3) and 256 x 4, the two
alternating in one process; plus the sampler's and the GAE kernel's own time per launch (device events around a run of
launches).  Prints one JSON line per figure.

    python profiles/experience.py [--rounds 7]

The baseline loop uses nothing this feature added (step(), ga3c_logits, ga3c_value), so it is what a user of the parent
commit would write; its sampled actions cost it the greedy step's bit-for-bit reproducibility, which is not measured here."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from gym_collision_avoidance_amd import _native as nat  # noqa: E402
from gym_collision_avoidance_amd import core  # noqa: E402

N_STEPS, GAMMA, LAM = 20, 0.99, 0.95


def build(E, N, K, sort, table, sample):
    sim = core.BatchedSim(core.make_params(E, N, max_obs=K, sort_mode=sort))
    sim.set_plugins(nat.POL_GA3C_CADRL, nat.DYN_UNICYCLE)
    sim.load_ga3c(keep_logits=True, keep_value=True)
    sim.set_fixture_table(table)
    if sample:
        sim.set_ga3c_sampling(0x5A3C)
    sim.reset_from_table()
    for _ in range(200):     # mixed episode phases
        sim.step()
    return sim


def with_feature(sim):
    xp = sim.collect(N_STEPS)
    adv, ret = xp.gae(GAMMA, LAM)
    return xp, adv, ret


def torch_loop(sim, gen):
    """fill()'s pattern with a sampled action: the network's greedy launch, then torch.multinomial on its logits"""
    S, A, LP, V, L, R, D, G = [], [], [], [], [], [], [], []
    for _ in range(N_STEPS):
        pre = sim.obs.clone()
        flags = sim.state["flags"].clone()
        ext = sim.ga3c()
        live = (((flags >> nat.POLICY_SHIFT) & 0xF) == nat.POL_GA3C_CADRL) & ((flags & nat.DONE) == 0)
        logp_all = torch.log_softmax(sim.ga3c_logits, dim=-1)
        act = torch.multinomial(logp_all.exp().reshape(-1, 11), 1, generator=gen).reshape(sim.E, sim.N)
        ext[..., 0] = torch.where(live, act.double(), ext[..., 0])
        sim._has_ga3c = False            # (the actions are in `ext`: the step must not query the network again)
        try:
            sim.step(ext)
        finally:
            sim._has_ga3c = True
        S.append(pre[..., 1:]); A.append(act); LP.append(logp_all.gather(-1, act[..., None])[..., 0]); V.append(sim.ga3c_value.clone())
        L.append(live); R.append(sim.rewards.clone()); D.append(sim.done.bool().clone()); G.append(sim.game_over.bool().clone())
    sim.ga3c()
    nv = sim.ga3c_value.clone()
    live, rew, val = torch.stack(L), torch.stack(R), torch.stack(V)
    end = torch.stack(D) | torch.stack(G)[:, :, None]
    adv = torch.zeros_like(rew)
    carry = torch.zeros_like(nv)
    for t in range(N_STEPS - 1, -1, -1):
        nv = torch.where(end[t], torch.zeros_like(nv), nv)
        carry = torch.where(end[t], torch.zeros_like(carry), carry)
        delta = rew[t] + GAMMA * nv - val[t]
        carry = torch.where(live[t], delta + GAMMA * LAM * carry, torch.zeros_like(carry))
        adv[t] = carry
        nv = torch.where(live[t], val[t], torch.zeros_like(nv))
    return torch.stack(S), torch.stack(A), torch.stack(LP), adv, adv + val


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def kernel_time(launch, reps=200):
    """device events around `reps` back-to-back launches -> microseconds per launch"""
    for _ in range(10):
        launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profiles/experience.py needs a GPU: a CPU run measures nothing")
    data = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))
    for E, N, K, sort in ((4096, 20, 19, nat.SORT_CLOSEST_LAST), (256, 4, 19, nat.SORT_CLOSEST_LAST)):
        table = data["n%d" % N]
        new, old = build(E, N, K, sort, table, True), build(E, N, K, sort, table, False)
        gen = torch.Generator(device=old.device)
        gen.manual_seed(1)
        for _ in range(2):
            with_feature(new)
            torch_loop(old, gen)
        a, b = [], []
        for _ in range(args.rounds):      # alternating
            a.append(timed(lambda: with_feature(new), 2) / N_STEPS * 1e6)
            b.append(timed(lambda: torch_loop(old, gen), 2) / N_STEPS * 1e6)
        step = []
        for _ in range(args.rounds):
            step.append(timed(new.step, 40) * 1e6)
        xp, _, _ = with_feature(new)
        ext = new._ga3c_ext
        t_sample = kernel_time(lambda: new._ga3c_sample(ext, new.ga3c_logits))
        t_gae = kernel_time(lambda: xp.gae(GAMMA, LAM))
        new._xp = {k: getattr(xp, k)[0].data_ptr() if k != "live" else xp.live.view(torch.uint8)[0].data_ptr()
                   for k in ("obs", "action", "logp", "value", "live", "address")}
        t_sample_slot = kernel_time(lambda: new._ga3c_sample(ext, new.ga3c_logits))
        new._xp = None
        print(json.dumps(dict(shape=[E, N], steps=N_STEPS, rounds=args.rounds,
                              collect_gae_us_per_step=dict(median=float(np.median(a)), min=float(min(a)), max=float(max(a))),
                              torch_loop_us_per_step=dict(median=float(np.median(b)), min=float(min(b)), max=float(max(b))),
                              sampled_step_us=dict(median=float(np.median(step)), min=float(min(step)), max=float(max(step))),
                              sampler_us_per_launch=t_sample, sampler_with_slot_us_per_launch=t_sample_slot,
                              gae_us_per_launch=t_gae, tape_bytes_per_step=new.experience_step_bytes(True))))
        sys.stdout.flush()
        new.check_faults()
        del new, old, xp


if __name__ == "__main__":
    main()
