"""On-policy training of the GA3C-CADRL policy without leaving the device: where collect_onpolicy.py ends, a learner begins.

A round is  collect -> gae -> net(x, live) -> a3c_loss -> backward -> opt.step() -> the env gets net.tensors():
the batch plays n steps with actions sampled on the device (BatchedSim.collect), cagpu_gae walks the tape, the network is
evaluated on the tape's rows by the kernel that acted (ga3c_train.TrainableGA3C.forward = cagpu_ga3c_query), its weight
gradients come from cagpu_ga3c_grad, a torch optimiser steps the parameters and BatchedSim.update_ga3c puts them into the
loaded network in place.  Nothing is read back (the loss is returned as a device tensor) and the graph is stated once.
The objective is ga3c_train.a3c_loss, this project's statement of A3C: the reference ships no training code.

    GYM_CONFIG_CLASS=EvaluateConfig python -m gym_collision_avoidance_amd.experiments.train_onpolicy
"""
import torch

from gym_collision_avoidance_amd import ga3c_train
from gym_collision_avoidance_amd.experiments import collect_onpolicy


def create_env(num_envs=64, num_agents=4, seed=0, sample_seed=0x5A3C, temperature=1.0, **kw):
    """collect_onpolicy.create_env's batch: every agent GA3C-CADRL, the value head on, actions sampled on the device"""
    return collect_onpolicy.create_env(num_envs=num_envs, num_agents=num_agents, seed=seed, sample_seed=sample_seed,
                                       temperature=temperature, **kw)


def train_round(env, net, opt, n, gamma=0.99, lam=0.95, beta=0.01, value_coef=0.5, temperature=1.0):
    """one round on `env` (reset() it once before the first) with the module `net` (TrainableGA3C.load(env._sim)) and the
    torch optimiser `opt` over net.parameters() -> the round's loss, a 0-d device tensor"""
    xp = env.collect_experience(n)
    adv, ret = xp.gae(gamma, lam)
    x, live = xp.rows()
    logits, value = net(x, live)
    loss = ga3c_train.a3c_loss(logits, value, xp.action, adv, ret, live=live, beta=beta, value_coef=value_coef,
                               temperature=temperature)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    env._sim.update_ga3c(net.tensors())
    return loss.detach()


def main(num_envs=64, num_agents=4, n=20, rounds=5, lr=1e-4):
    env = create_env(num_envs=num_envs, num_agents=num_agents)
    env.reset()
    net = ga3c_train.TrainableGA3C.load(env._sim)
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    loss = None
    for r in range(rounds):
        loss = train_round(env, net, opt, n)
        print("round %d: loss %.6f" % (r, float(loss)))
    return net, loss


if __name__ == "__main__":
    main()
