"""What making the pre-training scenes on the GPU costs and buys (dataset.on_device, ocrl_amd/utils/device_scenes.py).

1. Time per ocrl_scenes_batch call at B = 128, H = 64 and 128, with and without masks: device events around `--calls` back-to-back calls
   into preallocated outputs after a warm-up, repeated `--repeats` times (the spread is printed), and the store rate the time amounts to.
2. The images/s train_ocr.py logs for ocr=slate dataset=random-N5C4S4S2 dataset.obs_size=128 batch_size=128 after a warm-up, with
   dataset.on_device=True and with the host loader at num_workers=1 and num_workers=8, each as a fresh child process, the three
   alternating, `--repeats` times each.  train_ocr.py logs a cumulative rate; the rate after the warm-up is taken from two of its log
   lines: images between them over the time between them.

3. With --task <env file> (e.g. target-N4C4S3S1) instead: the task dataset's fused launch, ocrl_task_scenes_batch, timed as in 1., beside
   the same batch composed of the entry points that predate it: ocrl_sprite_env_reset, ocrl_sprite_render mode 1 (and mode 2 with
   masks), ocrl_obs_u8_to_f32 and the masks cast to fp32.  The composition is the baseline; its spread over the repeats is the
   allowance.  Then train_ocr.py's images/s on dataset=<env file> beside dataset=random-N5C4S4S2 dataset.on_device=True.

    python tools/bench_scenes.py [--calls 200] [--repeats 3] [--steps 200] [--warmup 50] [--skip-train] [--task target-N4C4S3S1]

Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import ctypes

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocrl_amd import _bridge, _lib  # noqa: E402

B, K = 128, 5


def timed(run, calls, warmup=20):
    """-> seconds per run() over `calls` back-to-back calls after a warm-up, by device events"""
    for _ in range(warmup):
        run()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def call_time(H, with_masks, calls):
    """-> seconds per ocrl_scenes_batch call (obs, and masks when asked for)"""
    dev = torch.device("cuda:0")
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    obs = torch.empty(B, 3, H, H, device=dev)
    masks = torch.empty(B, K + 1, H, H, device=dev) if with_masks else None
    desc = _lib.ScenesDesc(H=H, K=K)
    return timed(lambda: _bridge.launch(dev, _lib.lib().ocrl_scenes_batch, desc, 1, _lib.ptr(idx), B, _lib.ptr(obs), None, _lib.ptr(masks), None), calls)


def task_desc(task, H, E):
    from ocrl_amd import envs
    from ocrl_amd.utils.config import compose
    cfg = compose(os.path.join(ROOT, "configs"), "train_sb3", ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", f"env={task}"])
    d = envs.env_desc(cfg.env, E)
    d.H = H
    return d


def task_call_times(task, H, with_masks, calls):
    """-> (seconds per ocrl_task_scenes_batch call, seconds per composition of the older entry points) for the same B first frames:
    scene e << 24 of the fused launch is what environment e shows after ocrl_sprite_env_reset at episode 0"""
    dev, L = torch.device("cuda:0"), _lib.lib()
    d1, dE = task_desc(task, H, 1), task_desc(task, H, B)
    R = d1.hi + 1
    idx = torch.arange(B, dtype=torch.int64, device=dev) << 24
    obs = torch.empty(B, 3, H, H, device=dev)
    masks = torch.empty(B, R + 1, H, H, device=dev) if with_masks else None
    fused = lambda: _bridge.launch(dev, L.ocrl_task_scenes_batch, d1, 1, _lib.ptr(idx), B, _lib.ptr(obs), None, _lib.ptr(masks), None, None)
    state = torch.zeros(L.ocrl_sprite_env_state_floats(ctypes.byref(dE)), device=dev)
    u8 = torch.empty(B, H, H, 3, dtype=torch.uint8, device=dev)
    m8 = torch.empty(B, R + 1, H, H, dtype=torch.uint8, device=dev) if with_masks else None
    obs2 = torch.empty_like(obs)
    masks2 = torch.empty_like(masks) if with_masks else None

    def composed():
        _bridge.launch(dev, L.ocrl_sprite_env_reset, dE, _lib.ptr(state), 1, None, 0)
        _bridge.launch(dev, L.ocrl_sprite_render, _lib.ptr(state), B, R, H, 1, _lib.ptr(u8))
        _bridge.launch(dev, L.ocrl_obs_u8_to_f32, _lib.ptr(u8), _lib.ptr(obs2), B, H, H, 3)
        if with_masks:
            _bridge.launch(dev, L.ocrl_sprite_render, _lib.ptr(state), B, R, H, 2, _lib.ptr(m8))
            masks2.copy_(m8)                                       # the cast to fp32
    fused(), composed()
    torch.cuda.synchronize()
    if not torch.equal(obs, obs2) or (with_masks and not torch.equal(masks, masks2)):
        raise RuntimeError("the fused launch and the composition made different batches")
    return timed(fused, calls), timed(composed, calls)


def train_rate(extra, steps, warmup, log_every=10, dataset="random-N5C4S4S2"):
    """images/s of one train_ocr.py child between its log lines at steps `warmup` and the last one"""
    with tempfile.TemporaryDirectory() as run_dir:
        cmd = [sys.executable, os.path.join(ROOT, "train_ocr.py"), "ocr=slate", f"dataset={dataset}", "dataset.obs_size=128", f"batch_size={B}",
               f"max_steps={steps}", f"log_interval={log_every}", "eval_interval=1000000", f"run_dir={run_dir}"] + extra
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        lines = [json.loads(l) for l in open(os.path.join(run_dir, "metrics.jsonl"))]
    at = {l["step"]: (l["step"] + 1) * B / l["train/images_per_sec"] for l in lines if "train/images_per_sec" in l}      # step -> seconds since the start
    last = max(at)
    return (last - warmup) * B / (at[last] - at[warmup])


def task_main(args):
    med = lambda v: sorted(v)[len(v) // 2]
    for H in (64, 128):
        for with_masks in (False, True):
            pairs = [task_call_times(args.task, H, with_masks, args.calls) for _ in range(args.repeats)]
            fused, comp = sorted(p[0] for p in pairs), sorted(p[1] for p in pairs)
            planes = 3 + (task_desc(args.task, H, 1).hi + 2 if with_masks else 0)
            nbytes = B * H * H * 4 * planes
            spread = comp[-1] - comp[0]
            print(json.dumps({"what": "ocrl_task_scenes_batch", "task": args.task, "B": B, "H": H, "masks": with_masks,
                              "fused_us_per_batch": [round(1e6 * x, 2) for x in fused], "composed_us_per_batch": [round(1e6 * x, 2) for x in comp],
                              "composed_spread_us": round(1e6 * spread, 2), "bytes_written": nbytes, "bytes_per_scene": nbytes // B,
                              "fused_GB_per_s_at_median": round(nbytes / med(fused) / 1e9, 1),
                              "fused_not_slower": med(fused) <= med(comp) + spread}), flush=True)
    if args.skip_train:
        return
    runs = {args.task: dict(dataset=args.task, extra=[]), "random-N5C4S4S2": dict(dataset="random-N5C4S4S2", extra=["dataset.on_device=True"])}
    rates = {k: [] for k in runs}
    for _ in range(args.repeats):
        for name, r in runs.items():
            rates[name].append(round(train_rate(r["extra"], args.steps, args.warmup, dataset=r["dataset"]), 1))
            print(json.dumps({"what": "train_ocr.py images/s after warm-up", "dataset": name, "rates": rates[name]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50, help="a multiple of 10: the log line the timed window starts at")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--task", default=None, help="an env file of configs/env: measure that task's dataset instead (3. above)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scenes.py measures on the GPU; there is none")
    if args.task:
        return task_main(args)
    for H in (64, 128):
        for with_masks in (False, True):
            t = sorted(call_time(H, with_masks, args.calls) for _ in range(args.repeats))
            nbytes = B * H * H * 4 * (3 + (K + 1 if with_masks else 0))
            print(json.dumps({"what": "ocrl_scenes_batch", "B": B, "H": H, "masks": with_masks, "us_per_call": [round(1e6 * x, 2) for x in t],
                              "bytes_written": nbytes, "GB_per_s_at_median": round(nbytes / t[len(t) // 2] / 1e9, 1)}), flush=True)
    if args.skip_train:
        return
    runs = {"on_device": ["dataset.on_device=True"], "host_workers_1": ["num_workers=1"], "host_workers_8": ["num_workers=8"]}
    rates = {k: [] for k in runs}
    for _ in range(args.repeats):
        for name, extra in runs.items():
            rates[name].append(round(train_rate(extra, args.steps, args.warmup), 1))
            print(json.dumps({"what": "train_ocr.py images/s after warm-up", "loader": name, "rates": rates[name]}), flush=True)
    best = max(("host_workers_1", "host_workers_8"), key=lambda k: sorted(rates[k])[len(rates[k]) // 2])
    spread = max(rates[best]) - min(rates[best])
    print(json.dumps({"what": "summary", "steps": args.steps, "warmup": args.warmup, **{k: sorted(v) for k, v in rates.items()}, "better_host": best,
                      "host_spread": round(spread, 1),
                      "on_device_not_slower": sorted(rates["on_device"])[len(rates["on_device"]) // 2] >= sorted(rates[best])[len(rates[best]) // 2] - spread}),
          flush=True)


if __name__ == "__main__":
    main()
