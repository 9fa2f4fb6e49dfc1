"""HIP-event time of one fused rollout launch (xa_mlp_rollout, the sequential step loop) per
dynamics env kind: CartPole-v1, Acrobot-v1, MountainCar-v0 at n_envs x n_steps (default
16 x 128, fused GAE returns, Philox sampling, random-init actor-critic MLP). The kinds are
timed in alternating rounds of 200 launches each in one process; us per launch, median and
minimum over the rounds. Acrobot's step is one RK4 step of four derivative evaluations in
f64 with the device library's sin / cos on the per-step dependency chain.
usage: python tools/rollout_env_kinds.py [n_envs [n_steps [rounds]]]"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    from xagents_amd import PPO, kernels
    from xagents_amd.envs import AcrobotVecEnv, CartPoleVecEnv, MountainCarVecEnv
    from xagents_amd.utils.common import create_model
    argv = [int(a) for a in sys.argv[1:]]
    n_envs, n_steps, rounds = (argv + [16, 128, 7][len(argv):])[:3]
    launches = 200
    dev = torch.device('cuda')
    agents = {}
    for name, cls in (('CartPole-v1', CartPoleVecEnv), ('Acrobot-v1', AcrobotVecEnv),
                      ('MountainCar-v0', MountainCarVecEnv)):
        envs = cls(n_envs, seed=55, device=dev)
        model = create_model(envs, 'ppo', 'model', seed=55, device=dev)
        agents[name] = PPO(envs, model, n_steps=n_steps, seed=55, quiet=True, use_graph=False)

    def run(agent, n):
        for _ in range(n):
            kernels.rollout(agent._rargs)
            kernels.counter_bump(agent.rng_counter)

    times = {name: [] for name in agents}
    for agent in agents.values():
        run(agent, 20)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, agent in agents.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(agent, launches)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    for name, t in times.items():
        done = float(agents[name].b_done[:, 1:].mean())
        print(f'{name}: {n_envs} envs x {n_steps} steps, rollout + counter bump '
              f'{np.median(t):.1f} us median, {min(t):.1f} us min over {rounds} rounds of '
              f'{launches} launches (done rate of the last rollout {done:.4f})', flush=True)


if __name__ == '__main__':
    main()
