"""The ground-truth-state path (ocr=gt): the fused per-object MLP (ocrl_gt_mlp_fwd / _bwd) and the environment step in state mode.

mlp: dims [64, 64, 128], acts [relu, relu, none] on M = 5 E rows of width 5 (E environments of 4 objects and the agent), E = 16, 64, 256:
the forward alone (no_grad) and forward + backward (parameter gradients, no input gradient: what the RL loss asks of an encoder fed
observations), through ``ocrl_amd.ocrs.gt.gt_mlp`` and through the same layers as a chain of ``_HipLinear`` (the library's GEMM with the
ReLU fused, one launch per layer and direction plus the pad-to-4 copies of the 5-wide input).  Both sides pay the same torch autograd
bookkeeping.  env: ``step_device`` of target-N4C4S3S1 in render_mode state against image at the same E.

ms per call = the median over ``--calls`` (>= 200) individually timed calls after warm-up, each between two events on the stream; run
it twice and compare the spread before reading a difference.  ``--only mlp | env`` selects one half.

    python tools/bench_gt.py --calls 300
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ocrl_amd import envs  # noqa: E402
from ocrl_amd.ocrs.gt import gt_mlp  # noqa: E402
from ocrl_amd.poolings.transformer import _HipLinear  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402

DIMS, ACTS = (64, 64, 128), ("relu", "relu", "none")
SIZES = (16, 64, 256)


def median_ms(f, calls, warm=30):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 5)


def bench_mlp(calls):
    out = {}
    chain = nn.Sequential(*[_HipLinear(i, o, relu=a == "relu") for i, o, a in zip((5,) + DIMS[:-1], DIMS, ACTS)]).cuda()
    params = [p for m in chain for p in (m.weight, m.bias)]
    for E in SIZES:
        x = torch.rand(E, 5, 5, device="cuda")
        cot = torch.randn(E, 5, DIMS[-1], device="cuda")
        rows = x.reshape(E * 5, 5)                             # the GEMM takes rows; the fused kernel takes any leading shape

        def fwd(f, inp):
            with torch.no_grad():
                f(inp)

        def both(f, inp, c):
            for p in params:
                p.grad = None
            f(inp).backward(c)

        fused = lambda t: gt_mlp(t, params, ACTS)
        out[f"E{E}"] = dict(rows=E * 5,
                            fused_fwd_ms=median_ms(lambda: fwd(fused, x), calls), chain_fwd_ms=median_ms(lambda: fwd(chain, rows), calls),
                            fused_fwd_bwd_ms=median_ms(lambda: both(fused, x, cot), calls),
                            chain_fwd_bwd_ms=median_ms(lambda: both(chain, rows, cot.reshape(E * 5, -1)), calls))
    return out


def bench_env(calls):
    out = {}
    for E in SIZES:
        row = {}
        for mode in ("state", "image"):
            c = compose(os.path.join(ROOT, "configs"), "train_sb3", ["ocr=gt", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", "env=target-N4C4S3S1",
                                                                      f"env.render_mode={mode}"])
            env = envs.make_env(c, num_envs=E, seed=0, device="cuda:0")
            env.reset()
            actions = torch.randint(0, 4, (E,), generator=torch.Generator().manual_seed(E)).cuda()
            row[f"{mode}_step_ms"] = median_ms(lambda: env.step_device(actions), calls)
        out[f"E{E}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--only", default="", help="mlp | env")
    a = ap.parse_args()
    res = {}
    if a.only in ("", "mlp"):
        res["mlp"] = bench_mlp(a.calls)
    if a.only in ("", "env"):
        res["env"] = bench_env(a.calls)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
