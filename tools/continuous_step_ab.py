"""A/B of the env phase of TD3.train_step on Pendulum-v1 (default 16 envs): the fused env
step (ContinuousControlVecEnv fused=True: xa_td3_act, then ONE xa_continuous_env_step that
steps the env and appends to the replay ring, done / episode-return rows in mapped host
memory, one event wait) against the two-launch composition a dynamics env had before
(fused=False: xa_td3_act, the env's step kernel into the one-step record, xa_replay_env_step,
a device statistics row and a synchronous D2H copy of the done row).

Only the env phase is timed: update_weights is replaced by a no-op, so train_step is the
action launch, the env step, and the host's wait for the done flags -- what runs on every
step whether or not an episode ends. Both forms live in one process and are timed in
alternating rounds of `steps` train steps each after a warm-up; per round the host wall time
per step (perf_counter around steps that each end in a device wait) and the HIP-event time
per step. Launches per step are counted in a separate untimed pass by wrapping the modules'
`call`. One JSON line goes to profiles/continuous_step_ab.json (or argv[4]).
usage: python tools/continuous_step_ab.py [n_envs [steps [rounds [out.json]]]]"""
import json
import sys
import time
from collections import Counter
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def make_agent(n_envs, fused, dev):
    from xagents_amd import TD3
    from xagents_amd.envs import create_envs
    from xagents_amd.utils.common import create_buffers, create_model
    envs = create_envs('Pendulum-v1', n_envs, device=dev, seed=55, fused=fused)
    actor = create_model(envs, 'td3', 'actor_model', seed=55, device=dev)
    critic = create_model(envs, 'td3', 'critic_model', seed=55, device=dev)
    bufs = create_buffers('td3', 4096 * n_envs, 16 * n_envs, n_envs, initial_size=16 * n_envs)
    agent = TD3(envs, actor, critic, bufs, seed=55, quiet=True, gradient_steps=1)
    agent.fill_buffers()
    agent.update_weights = lambda steps: None  # the env phase only
    return agent


def count_launches(agent, steps=8):
    """C-ABI calls per train step, by name (an untimed pass)."""
    import xagents_amd.base as base
    import xagents_amd.ddpg.agent as ddpg
    import xagents_amd.envs as envs
    import xagents_amd.td3.agent as td3
    seen = Counter()
    mods = [m for m in (base, ddpg, envs, td3) if hasattr(m, 'call')]
    saved = [m.call for m in mods]

    def counting(orig):
        def call(name, *args):
            seen[name] += 1
            return orig(name, *args)
        return call

    for m in mods:
        m.call = counting(m.call)
    try:
        for _ in range(steps):
            agent.train_step()
    finally:
        for m, c in zip(mods, saved):
            m.call = c
    torch.cuda.synchronize()
    return {k: v / steps for k, v in sorted(seen.items())}


def main():
    argv = sys.argv[1:]
    n_envs, steps, rounds = ([int(a) for a in argv[:3]] + [16, 2000, 7][len(argv[:3]):])[:3]
    out = Path(argv[3]) if len(argv) > 3 else ROOT / 'profiles' / 'continuous_step_ab.json'
    if not torch.cuda.is_available():
        raise SystemExit('continuous_step_ab.py needs a HIP device')
    dev = torch.device('cuda')
    agents = {'fused': make_agent(n_envs, True, dev), 'composed': make_agent(n_envs, False, dev)}
    assert not agents['fused'].envs.has_pre_step and agents['composed'].envs.has_pre_step
    for agent in agents.values():  # warm-up: code objects, the lazy staging set-up
        for _ in range(200):
            agent.train_step()
    torch.cuda.synchronize()
    launches = {name: count_launches(agent) for name, agent in agents.items()}
    wall = {name: [] for name in agents}
    gpu = {name: [] for name in agents}
    for _ in range(rounds):
        for name, agent in agents.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(steps):
                agent.train_step()
            e1.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e6 / steps)
            gpu[name].append(e0.elapsed_time(e1) * 1e3 / steps)
    row = dict(tool='continuous_step_ab', agent='TD3', env='Pendulum-v1', n_envs=n_envs,
               steps_per_round=steps, rounds=rounds, unit='us per env-phase step')
    for name in agents:
        row[name] = dict(wall_median=float(np.median(wall[name])), wall_min=min(wall[name]),
                         wall_max=max(wall[name]), event_median=float(np.median(gpu[name])),
                         event_min=min(gpu[name]), event_max=max(gpu[name]),
                         launches_per_step=launches[name],
                         launch_count=sum(launches[name].values()))
    row['wall_ratio_fused_over_composed'] = row['fused']['wall_median'] / row['composed']['wall_median']
    line = json.dumps(row)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
