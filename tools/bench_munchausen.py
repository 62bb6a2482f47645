"""What DQN's Munchausen targets cost (include/ocrl_hip_munchausen.h), in one run, at the configs' own shapes: batch 32, 4 actions, and
for the quantile heads 8 (iqn.yaml's N') and 50 (qrdqn.yaml's) quantile values per action.

    launch        us per ``ocrl_munchausen_targets`` (one launch, no workspace) without quantile values, with 8 and with 50
    train_step    ms per ``DQN.train_step()`` with and without ``munchausen`` on the same head behind the ground-truth encoder (ocr=gt,
                  pooling=mlp), batch 32, alternating: the scalar head (configs/sb3/mdqn.yaml beside dqn.yaml) and the implicit quantile
                  head (miqn.yaml beside iqn.yaml with ``double_q: False``, which ``munchausen`` requires, so that the two differ in the
                  Munchausen targets alone)

us / ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream
(tools/bench_acnet.py's method), timed from Python through ctypes as the loop calls them.  There is no threshold.  What the switch adds
to an update: the target network's pass takes 2 x 32 rows in place of 32, one concatenation of the two observation batches, one
launch, and on the implicit quantile head one more draw of fractions."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_sb3  # noqa: E402
from ocrl_amd import _lib  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from tools.bench_acnet import median_ms  # noqa: E402

B, A = 32, 4
SAMPLES = (0, 8, 50)
ALPHA, TAU, CLIP = 0.9, 0.03, -1.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"dqn": ("dqn", ()), "mdqn": ("mdqn", ()), "iqn": ("iqn", ("sb3.algo_kwargs.double_q=False",)), "miqn": ("miqn", ())}


def bench_launch(calls, out):
    L, p = _lib.lib(), _lib.ptr
    st = _lib.stream()
    g = torch.Generator().manual_seed(1)
    cur, nxt = torch.randn(B, A, generator=g).cuda(), torch.randn(B, A, generator=g).cuda()
    actions, rewards = torch.randint(0, A, (B,), generator=g).cuda(), torch.rand(B, generator=g).cuda()
    dones = (torch.arange(B) % 5 == 0).to(torch.uint8).cuda()
    ro, nv = torch.empty(B, device="cuda"), torch.empty(B, A, device="cuda")
    res = {}
    for Np in SAMPLES:
        quant = torch.randn(B, A, Np, generator=g).cuda() if Np else None
        nm = torch.empty(B, A, Np, device="cuda") if Np else None
        ms = median_ms(lambda: _lib.check(L.ocrl_munchausen_targets(p(cur), p(nxt), p(quant), Np, p(actions), p(rewards), p(dones), B, A, ALPHA, TAU, CLIP,
                                                                    p(ro), p(nv), p(nm), st)), calls)
        res[f"Np{Np}_us"] = round(ms * 1e3, 2)
    out["launch"] = dict(res, batch=B, actions=A)


def bench_loop(calls, out):
    models = {}
    for name, (sb3, over) in CONFIGS.items():
        c = compose(os.path.join(ROOT, "configs"), "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4",
                                                                 "device=cuda:0", "sb3.algo_kwargs.buffer_size=4096", f"sb3.algo_kwargs.batch_size={B}", *over])
        _, _, model = train_sb3.build(c)
        model._total_timesteps = 1 << 20
        for _ in range(64):
            model.collect_step()
        models[name] = model
    ms = {k: [] for k in models}
    for _ in range(3):                                  # alternating: drift of the machine lands on all
        for k, m in models.items():
            ms[k].append(median_ms(m.train_step, calls))
    res = {k: round(sorted(v)[1], 5) for k, v in ms.items()}
    out["train_step_gt"] = dict(res, mdqn_over_dqn=round(res["mdqn"] / res["dqn"], 3), miqn_over_iqn=round(res["miqn"] / res["iqn"], 3), batch=B,
                                rounds={k: [round(t, 5) for t in v] for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_munchausen: no GPU: the times are taken on the device or not at all")
    out = {}
    bench_launch(a.calls, out)
    bench_loop(a.calls, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
