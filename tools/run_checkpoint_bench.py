"""File size and wall time of save_run / load_run at the trainers' default ring (1024 envs x 4 agents, horizon 256)."""
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_uav_collision_avoidance_amd import UAVVectorEnv
from gym_uav_collision_avoidance_amd.checkpoint import load_run, save_run
from gym_uav_collision_avoidance_amd.learners import FusedSAC
from gym_uav_collision_avoidance_amd.replay import DeviceReplay

dev = torch.device("cuda", 0)
venv = UAVVectorEnv(1024, num_agents=4, device=dev, seed=0)
mem = DeviceReplay(venv.env, horizon=256)
mem.begin(venv.reset())
gen = torch.Generator(device=dev).manual_seed(0)
prioritized = 0.6 if "--prioritized" in sys.argv else None
agent = FusedSAC(device=dev, generator=gen, memory=mem, prioritized=prioritized)
for t in range(300):
    agent.select_action(mem.state, evaluate=False, out=mem.action_slot())
    mem.step(polar=True, auto_reset="agent0_done", step_cap=1500, track_returns=True)
    if t + 1 == 16:
        agent.capture(256)
    if t + 1 >= 16:
        agent.run(1)
torch.cuda.synchronize()
run = dict(env=venv.env, memory=mem, agent=agent, generator=gen)
with tempfile.TemporaryDirectory() as d:
    for name, kw, parts in (("whole", {}, run), ("include_memory=False", dict(include_memory=False),
                                                 {k: v for k, v in run.items() if k != "memory"})):
        path = os.path.join(d, "run.pt")
        save, load = [], []
        for _ in range(5):
            t0 = time.perf_counter()
            save_run(path, **run, extra={"t": 300}, **kw)
            save.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            load_run(path, **parts)
            load.append(time.perf_counter() - t0)
        print(f"{name} prioritized={prioritized}: file {os.path.getsize(path) / 2**20:.1f} MiB, save_run median "
              f"{statistics.median(save) * 1e3:.0f} ms (min {min(save) * 1e3:.0f}, max {max(save) * 1e3:.0f}), load_run median "
              f"{statistics.median(load) * 1e3:.0f} ms (min {min(load) * 1e3:.0f}, max {max(load) * 1e3:.0f}), 5 runs each",
              flush=True)
agent.close()
venv.close()
