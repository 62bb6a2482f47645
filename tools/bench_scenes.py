"""What making the pre-training scenes on the GPU costs and buys (dataset.on_device, ocrl_amd/utils/device_scenes.py).

1. Time per ocrl_scenes_batch call at B = 128, H = 64 and 128, with and without masks: device events around `--calls` back-to-back calls
   into preallocated outputs after a warm-up, repeated `--repeats` times (the spread is printed), and the store rate the time amounts to.
2. The images/s train_ocr.py logs for ocr=slate dataset=random-N5C4S4S2 dataset.obs_size=128 batch_size=128 after a warm-up, with
   dataset.on_device=True and with the host loader at num_workers=1 and num_workers=8, each as a fresh child process, the three
   alternating, `--repeats` times each.  train_ocr.py logs a cumulative rate; the rate after the warm-up is taken from two of its log
   lines: images between them over the time between them.

    python tools/bench_scenes.py [--calls 200] [--repeats 3] [--steps 200] [--warmup 50] [--skip-train]

Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ocrl_amd import _bridge, _lib  # noqa: E402

B, K = 128, 5


def call_time(H, with_masks, calls, warmup=20):
    """-> seconds per ocrl_scenes_batch call (obs, and masks when asked for)"""
    dev = torch.device("cuda:0")
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    obs = torch.empty(B, 3, H, H, device=dev)
    masks = torch.empty(B, K + 1, H, H, device=dev) if with_masks else None
    desc = _lib.ScenesDesc(H=H, K=K)
    run = lambda: _bridge.launch(dev, _lib.lib().ocrl_scenes_batch, desc, 1, _lib.ptr(idx), B, _lib.ptr(obs), None, _lib.ptr(masks), None)
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


def train_rate(extra, steps, warmup, log_every=10):
    """images/s of one train_ocr.py child between its log lines at steps `warmup` and the last one"""
    with tempfile.TemporaryDirectory() as run_dir:
        cmd = [sys.executable, os.path.join(ROOT, "train_ocr.py"), "ocr=slate", "dataset=random-N5C4S4S2", "dataset.obs_size=128", f"batch_size={B}",
               f"max_steps={steps}", f"log_interval={log_every}", "eval_interval=1000000", f"run_dir={run_dir}"] + extra
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        lines = [json.loads(l) for l in open(os.path.join(run_dir, "metrics.jsonl"))]
    at = {l["step"]: (l["step"] + 1) * B / l["train/images_per_sec"] for l in lines if "train/images_per_sec" in l}      # step -> seconds since the start
    last = max(at)
    return (last - warmup) * B / (at[last] - at[warmup])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50, help="a multiple of 10: the log line the timed window starts at")
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scenes.py measures on the GPU; there is none")
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
