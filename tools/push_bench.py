"""What impulse pushes cost: the time of k_apply_impulse at 4096 envs with every env pushed, next to one control-step
launch of the same handle, and CopycatAgent.sample env-steps/s without a schedule, with interval=30 and with interval=1.  HIP events,
medians of 3 blocks.      python tools/push_bench.py [n_envs] [horizon]"""
import statistics
import sys
import time

import numpy as np
import torch

from _rows_bench import blocks as _blocks, dev, kpsim, std, t
from kinpoly_amd.push import PushSchedule
from kinpoly_amd.uhc_env import BatchedHumanoidEnv, CopycatAgent

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
horizon = int(sys.argv[2]) if len(sys.argv) > 2 else 32


def blocks(fn, reps):
    """median over 3 blocks of (event time of reps calls) / reps, in ms"""
    return _blocks(fn, reps, 3)[0]


# ---- the kernel
rng = np.random.default_rng(0)
qpos = np.tile(std["qpos"], (n, 1)); qpos[:, 7:] += rng.normal(size=(n, 69)) * 0.1
sim = kpsim.KpSim(kpsim.KpModel(), n)
sim.set_state(t(qpos), t(rng.normal(size=(n, 75)) * 0.3)); sim.set_target(t(np.tile(std["qpos"], (n, 1))))
act = t(rng.normal(size=(n, 75)) * 0.2)
ent = t(rng.integers(0, 24, n), torch.int32)
imp = t(rng.normal(size=(n, 6)) * [1, 1, 1, 0.1, 0.1, 0.1]); off = t(rng.uniform(-0.1, 0.1, (n, 3)))
none = torch.full((n,), -1, dtype=torch.int32, device=dev)
for _ in range(5):
    sim.step_ctrl(act, 15); sim.apply_impulse(ent, imp, off)
torch.cuda.synchronize()
print(f"# {n} envs, medians of 3 blocks")
print(f"k_apply_impulse, every env pushed   {blocks(lambda: sim.apply_impulse(ent, imp, off), 50) * 1e3:9.1f} us")
print(f"k_apply_impulse, no env pushed      {blocks(lambda: sim.apply_impulse(none, imp, off), 50) * 1e3:9.1f} us")
print(f"control-step launch (15 substeps)   {blocks(lambda: sim.step_ctrl(act, 15), 10) * 1e3:9.1f} us")
del sim

# ---- sampling throughput of the UHC agent on the sinusoid clips of scripts/train_uhc.py
T = 64
clips = np.tile(std["qpos"], (n, T, 1))
amp, freq, ph = rng.uniform(0, 0.15, (n, 1, 69)), rng.uniform(0.2, 1.0, (n, 1, 69)), rng.uniform(0, 2 * np.pi, (n, 1, 69))
clips[:, :, 7:] += amp * (np.sin(2 * np.pi * freq * (np.arange(T)[None, :, None] / 30.0) + ph) - np.sin(ph))
for label, interval in (("no schedule", None), ("interval=30", 30), ("interval=1", 1)):
    torch.manual_seed(1)
    sched = None if interval is None else PushSchedule(n, dev, interval, bodies=("Pelvis", "Chest"), impulse=(10.0, 30.0), seed=0)
    env = BatchedHumanoidEnv(n, 0, env_init_noise=0.0, seed=1, push_schedule=sched)
    env.load_expert(torch.tensor(clips, dtype=torch.float32))
    agent = CopycatAgent(env)
    agent.sample(4)
    rates = []
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        agent.sample(horizon)
        torch.cuda.synchronize(); rates.append(n * horizon / (time.perf_counter() - t0))
    pushes = "" if sched is None else f"   ({int(sched.count)} pushes drawn)"
    print(f"CopycatAgent.sample, {label:12s} {statistics.median(rates):12.0f} env-steps/s{pushes}")
    del agent, env
