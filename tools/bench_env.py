"""Environment steps per second of a sprite task at 64 x 64: step_device of the environment make_env builds (state, step and frames on
the GPU, no host read) against a host environment, for which the numpy restatement of tests/sprite_env_ref.py (tests/oddoneout_ref.py
for Odd-One-Out) stands in: it steps and draws every
environment in numpy and uploads the frames, with the actions read back from the device first, as a host VecEnv behind
``actions.cpu().numpy()`` would.

    python tools/bench_env.py [--env target-N4C4S3S1] [--envs 16 64 256] [--steps 200] [--host-steps 5]

Prints one JSON line per E.  Actions are uniform random in both runs; the policy is left out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocrl_amd import envs  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from tests import oddoneout_ref as O, sprite_env_ref as R  # noqa: E402


def device_rate(cfg, E, steps, warmup=20):
    env = envs.make_env(cfg, num_envs=E, seed=0, device="cuda")
    env.reset()
    actions = torch.randint(0, 4, (steps + warmup, E), device="cuda")
    for t in range(warmup):
        env.step_device(actions[t])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(warmup, warmup + steps):
        env.step_device(actions[t])
    torch.cuda.synchronize()
    return E * steps / (time.perf_counter() - t0)


def host_rate(cfg, E, steps):
    d = envs.env_desc(cfg.env, E)
    s, Env = (O.spec_from_desc(d), O.Env) if d.task == 1 else (R.spec_from_desc(d), R.Env)
    refs = [Env(s, lambda k, e=e: (np.floor(np.random.RandomState(1000 * e + k).rand(4096) * 2 ** 24) / 2 ** 24).astype(np.float32)) for e in range(E)]
    actions = torch.randint(0, 4, (steps + 1, E), device="cuda")
    for t in range(steps + 1):
        if t == 1:                                            # step 0 warms the copies up and is not timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        a = actions[t].cpu().numpy()
        frames = np.empty((E, 64, 64, 3), dtype=np.uint8)
        for e in range(E):
            refs[e].step(int(a[e]))
            frames[e] = R.render(refs[e].rows, 64)[0]
        torch.from_numpy(frames).cuda().permute(0, 3, 1, 2).contiguous()
    torch.cuda.synchronize()
    return E * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="target-N4C4S3S1", help="a file of configs/env")
    ap.add_argument("--envs", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=5)
    args = ap.parse_args()
    cfg = compose(os.path.join(ROOT, "configs"), "train_sb3", ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", f"env={args.env}"])
    for E in args.envs:
        dev, host = device_rate(cfg, E, args.steps), host_rate(cfg, E, args.host_steps)
        print(json.dumps({"env": args.env, "envs": E, "obs_size": 64, "device_steps_per_s": round(dev, 1), "host_steps_per_s": round(host, 1),
                          "device_us_per_call": round(1e6 * E / dev, 2)}), flush=True)


if __name__ == "__main__":
    main()
