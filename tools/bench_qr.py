"""What DQN's quantile head costs beside the categorical one (include/ocrl_hip_qr.h beside include/ocrl_hip_c51.h), in the same run, at
the configs' own shapes: the default head (net_arch (64, 64), ReLU) on F = 128 features, 4 actions, batch 32, 50 quantiles against 51
atoms on [0, 2], both with the dueling stream.

    td            ms per ``ocrl_qr_td_fwd_bwd`` beside ``ocrl_c51_td_fwd_bwd`` (three launches each)
    act           ms per ``ocrl_qr_act`` beside ``ocrl_c51_act`` (one launch each)
    target        ms per target forward without a workspace: ``ocrl_qr_fwd`` writing quantiles and q beside ``ocrl_c51_fwd`` writing probs and q
    train_step    ms per ``DQN.train_step()`` (the update step) of configs/sb3/qrdqn.yaml beside configs/sb3/dqn_c51.yaml and
                  configs/sb3/rainbow.yaml behind the ground-truth encoder (ocr=gt, pooling=mlp), batch 32, the three alternating.
                  qrdqn.yaml is rainbow.yaml with the other head, so qrdqn / rainbow is the heads' difference and qrdqn / dqn_c51 adds
                  the noisy layers' launches
    collect_step  ms per ``DQN.collect_step()`` (the collection step: four on-device environments, one act launch) of the same three

ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream (tools/bench_acnet.py's
method), timed from Python through ctypes as the loop calls them.  A call of this size is a few launches of one or two workgroups: the
figures are launch and latency costs, not throughput.  There is no threshold: the pair work is N^2 = 2 500 terms per row against the
projection's Z^2 = 2 601, so the same order is expected."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_sb3  # noqa: E402
from ocrl_amd import _lib  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from tools.bench_acnet import median_ms  # noqa: E402
from tools.bench_c51 import ACTS, DIMS, A, B, F, GAMMA, V_MAX, V_MIN, Z, params  # noqa: E402

N, KAPPA = 50, 1.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("dqn_c51", "rainbow", "qrdqn")


def bench_heads(calls, out):
    L, p, ps_ = _lib.lib(), _lib.ptr, _lib.ptrs
    st = _lib.stream()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, F, generator=g).cuda()
    actions, rewards = torch.randint(0, A, (B,), generator=g).cuda(), torch.rand(B, generator=g).cuda()
    dones = (torch.arange(B) % 5 == 0).to(torch.uint8).cuda()
    next_probs = torch.softmax(torch.randn(B, A, Z, generator=g), dim=-1).cuda()
    next_quantiles = torch.randn(B, A, N, generator=g).cuda()
    next_q = torch.randn(B, A, generator=g).cuda()
    scal, row_loss, dx = torch.empty(3, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, F, device="cuda")
    acts_out, q = torch.empty(B, device="cuda", dtype=torch.int64), torch.empty(B, A, device="cuda")
    probs, theta = torch.empty(B, A, Z, device="cuda"), torch.empty(B, A, N, device="cuda")
    res = {}
    d = _lib.c51_desc(B, F, A, Z, DIMS, ACTS, True)
    w = params((A * Z, Z))
    dw = [torch.empty_like(t) for t in w]
    n = L.ocrl_c51_ws_floats(ctypes.byref(d))
    ws = torch.empty(n, device="cuda")
    res["c51_dueling"] = dict(
        td_ms=median_ms(lambda: _lib.check(L.ocrl_c51_td_fwd_bwd(ctypes.byref(d), p(x), ps_(w), V_MIN, V_MAX, p(next_probs), p(next_q), p(actions), p(rewards),
                                                               p(dones), None, None, GAMMA, p(scal), p(row_loss), p(dx), ps_(dw), p(ws), n, st)), calls),
        act_ms=median_ms(lambda: _lib.check(L.ocrl_c51_act(ctypes.byref(d), p(x), ps_(w), V_MIN, V_MAX, 1, 0, 0.1, None, p(acts_out), p(q), st)), calls),
        target_ms=median_ms(lambda: _lib.check(L.ocrl_c51_fwd(ctypes.byref(d), p(x), ps_(w), V_MIN, V_MAX, None, p(probs), p(q), 0, None, 0, st)), calls),
        n_floats=sum(t.numel() for t in w))
    d = _lib.qr_desc(B, F, A, N, DIMS, ACTS, True)
    w = params((A * N, N))
    dw = [torch.empty_like(t) for t in w]
    n = L.ocrl_qr_ws_floats(ctypes.byref(d))
    ws = torch.empty(n, device="cuda")
    res["qr_dueling"] = dict(
        td_ms=median_ms(lambda: _lib.check(L.ocrl_qr_td_fwd_bwd(ctypes.byref(d), p(x), ps_(w), p(next_quantiles), p(next_q), p(actions), p(rewards), p(dones),
                                                              None, None, GAMMA, KAPPA, p(scal), p(row_loss), p(dx), ps_(dw), p(ws), n, st)), calls),
        act_ms=median_ms(lambda: _lib.check(L.ocrl_qr_act(ctypes.byref(d), p(x), ps_(w), 1, 0, 0.1, None, p(acts_out), p(q), st)), calls),
        target_ms=median_ms(lambda: _lib.check(L.ocrl_qr_fwd(ctypes.byref(d), p(x), ps_(w), p(theta), p(q), 0, None, 0, st)), calls),
        n_floats=sum(t.numel() for t in w))
    for k in ("td_ms", "act_ms", "target_ms"):
        res["qr_dueling"][k.replace("_ms", "_ratio")] = round(res["qr_dueling"][k] / res["c51_dueling"][k], 3)
    for r in res.values():
        for k in ("td_ms", "act_ms", "target_ms"):
            r[k] = round(r[k], 5)
    out["heads"] = dict(res, batch=B, features=F, actions=A, atoms=Z, quantiles=N)


def bench_loop(calls, out):
    models = {}
    for sb3 in CONFIGS:
        c = compose(os.path.join(ROOT, "configs"), "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4",
                                                                 "device=cuda:0", "sb3.algo_kwargs.buffer_size=4096", f"sb3.algo_kwargs.batch_size={B}"])
        _, _, model = train_sb3.build(c)
        model._total_timesteps = 1 << 20
        for _ in range(64):
            model.collect_step()
        models[sb3] = model
    for what, step in (("train_step", lambda m: m.train_step), ("collect_step", lambda m: m.collect_step)):
        ms = {k: [] for k in models}
        for _ in range(3):                                  # the three alternating: drift of the machine lands on all
            for k, m in models.items():
                ms[k].append(median_ms(step(m), calls))
        res = {k: round(sorted(v)[1], 5) for k, v in ms.items()}
        out[f"{what}_gt"] = dict(res, qrdqn_over_dqn_c51=round(res["qrdqn"] / res["dqn_c51"], 3), qrdqn_over_rainbow=round(res["qrdqn"] / res["rainbow"], 3),
                                 batch=B, rounds={k: [round(t, 5) for t in v] for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qr: no GPU: the times are taken on the device or not at all")
    out = {}
    bench_heads(a.calls, out)
    bench_loop(a.calls, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
