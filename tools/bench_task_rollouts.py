"""What the random walk adds to a task dataset's batch (dataset.only_initial=False; include/ocrl_hip_rollout.h).

Time per call at B = 128, H = 64 of ocrl_task_scenes_batch (the first frames) and of ocrl_task_scenes_rollout_batch with the step drawn in
[0, max_step] (default 99, what dataset.only_initial=False asks for at task.max_steps = 100) and with max_step = 0 (the same kernel, no
step walked): device events around `--calls` back-to-back calls into preallocated outputs after a warm-up.  The forms alternate within a
repeat, `--repeats` times, and the spread is printed.  With --parent-lib <libocrl_hip.so of another build, e.g. the parent commit's> that
library's ocrl_task_scenes_batch is timed in the same alternation.

    python tools/bench_task_rollouts.py [--task target-N4C4S3S1] [--max-step 99] [--calls 200] [--repeats 5] [--masks] [--parent-lib PATH]

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocrl_amd import _lib  # noqa: E402
from tools.bench_scenes import task_desc, timed  # noqa: E402

B, H = 128, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="target-N4C4S3S1", help="an env file of configs/env")
    ap.add_argument("--max-step", type=int, default=99)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--masks", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_task_rollouts.py measures on the GPU; there is none")
    dev, L = torch.device("cuda:0"), _lib.lib()
    d = task_desc(args.task, H, 1)
    R = d.hi + 1
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    obs = torch.empty(B, 3, H, H, device=dev)
    masks = torch.empty(B, R + 1, H, H, device=dev) if args.masks else None
    taken = torch.empty(B, dtype=torch.int32, device=dev)
    st = _lib.stream(dev)
    ref = ctypes.byref(d)

    def first(lib):
        return lambda: _lib.check(lib.ocrl_task_scenes_batch(ref, 1, _lib.ptr(idx), B, _lib.ptr(obs), None, _lib.ptr(masks), None, None, st))

    def walked(max_step):
        return lambda: _lib.check(L.ocrl_task_scenes_rollout_batch(ref, 1, _lib.ptr(idx), None, max_step, B, _lib.ptr(obs), None, _lib.ptr(masks), None, None,
                                                                   _lib.ptr(taken), st))
    forms = {"first_frames": first(L), "rollout_max_step_0": walked(0), f"rollout_max_step_{args.max_step}": walked(args.max_step)}
    if args.parent_lib:
        P = ctypes.CDLL(os.path.abspath(args.parent_lib))
        P.ocrl_task_scenes_batch.restype, P.ocrl_task_scenes_batch.argtypes = _lib.ABI.functions["ocrl_task_scenes_batch"]
        forms = {"parent_first_frames": first(P), **forms}
    # the two entry points agree at step 0 before anything is timed
    forms["first_frames"]()
    a = obs.clone()
    forms["rollout_max_step_0"]()
    torch.cuda.synchronize()
    if not torch.equal(a, obs) or taken.any():
        raise RuntimeError("step 0 of the rollout is not the first frame")
    forms[f"rollout_max_step_{args.max_step}"]()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.repeats):
        for k, run in forms.items():
            times[k].append(timed(run, args.calls))
    print(json.dumps({"what": "task scenes per call", "task": args.task, "B": B, "H": H, "masks": args.masks, "calls": args.calls,
                      "mean_steps_taken": round(taken.float().mean().item(), 1), "max_steps_taken": int(taken.max()),
                      "us_per_call": {k: [round(1e6 * x, 2) for x in sorted(v)] for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
