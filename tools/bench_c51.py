"""What DQN's categorical head costs beside the scalar one (include/ocrl_hip_c51.h beside include/ocrl_hip_dqn.h), in the same run: the
default head (net_arch (64, 64), ReLU) on F = 128 features, 4 actions, batch 32, with 51 atoms on [0, 2].

    td            ms per ``ocrl_c51_td_fwd_bwd`` (three launches) with and without dueling, beside ``ocrl_dqn_td_fwd_bwd``
    act           ms per ``ocrl_c51_act`` (one launch), beside ``ocrl_dqn_act``
    target        ms per target forward: ``ocrl_c51_fwd`` writing probs and q without a workspace, beside ``ocrl_qnet_fwd``
    train_step    ms per ``DQN.train_step()`` of configs/sb3/dqn_c51.yaml against configs/sb3/dqn_per.yaml behind the ground-truth
                  encoder (ocr=gt, pooling=mlp), batch 32, the two alternating

ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream (tools/bench_acnet.py's
method), timed from Python through ctypes as the loop calls them.  A call of this size is a few launches of one or two workgroups: the
figures are launch and latency costs, not throughput."""
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

B, F, A, Z = 32, 128, 4, 51
DIMS, ACTS = (64, 64), (1, 1)
V_MIN, V_MAX, GAMMA = 0.0, 2.0, 0.99
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(outs):
    """a chain's parameters on the device: DIMS, then one Linear per entry of `outs` on the last width"""
    g = torch.Generator().manual_seed(0)
    ps, k = [], F
    for n in DIMS:
        ps += [(torch.rand(n, k, generator=g) * 2 - 1) / k ** 0.5, torch.zeros(n)]
        k = n
    for n in outs:
        ps += [(torch.rand(n, k, generator=g) * 2 - 1) / k ** 0.5, torch.zeros(n)]
    return [p.cuda() for p in ps]


def bench_heads(calls, out):
    L, p, ps_ = _lib.lib(), _lib.ptr, _lib.ptrs
    st = _lib.stream()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, F, generator=g).cuda()
    actions, rewards = torch.randint(0, A, (B,), generator=g).cuda(), torch.rand(B, generator=g).cuda()
    dones = (torch.arange(B) % 5 == 0).to(torch.uint8).cuda()
    next_probs = torch.softmax(torch.randn(B, A, Z, generator=g), dim=-1).cuda()
    next_q = torch.randn(B, A, generator=g).cuda()
    scal, row_loss, dx = torch.empty(3, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, F, device="cuda")
    acts_out, q, probs = torch.empty(B, device="cuda", dtype=torch.int64), torch.empty(B, A, device="cuda"), torch.empty(B, A, Z, device="cuda")
    res = {}
    # the scalar head
    d = _lib.qnet_desc(B, F, A, DIMS, ACTS)
    w = params((A,))
    dw = [torch.empty_like(t) for t in w]
    n = L.ocrl_qnet_ws_floats(ctypes.byref(d))
    ws = torch.empty(n, device="cuda")
    res["scalar"] = dict(
        td_ms=median_ms(lambda: _lib.check(L.ocrl_dqn_td_fwd_bwd(ctypes.byref(d), p(x), ps_(w), p(next_q), p(actions), p(rewards), p(dones), GAMMA, p(scal),
                                                               p(dx), ps_(dw), p(ws), n, st)), calls),
        act_ms=median_ms(lambda: _lib.check(L.ocrl_dqn_act(ctypes.byref(d), p(x), ps_(w), 1, 0, 0.1, None, p(acts_out), p(q), st)), calls),
        target_ms=median_ms(lambda: _lib.check(L.ocrl_qnet_fwd(ctypes.byref(d), p(x), ps_(w), p(q), 0, None, 0, st)), calls))
    # the categorical head
    for name, dueling in (("c51", False), ("c51_dueling", True)):
        d = _lib.c51_desc(B, F, A, Z, DIMS, ACTS, dueling)
        w = params((A * Z, Z) if dueling else (A * Z,))
        dw = [torch.empty_like(t) for t in w]
        n = L.ocrl_c51_ws_floats(ctypes.byref(d))
        ws = torch.empty(n, device="cuda")
        res[name] = dict(
            td_ms=median_ms(lambda: _lib.check(L.ocrl_c51_td_fwd_bwd(ctypes.byref(d), p(x), ps_(w), V_MIN, V_MAX, p(next_probs), p(next_q), p(actions),
                                                                   p(rewards), p(dones), None, None, GAMMA, p(scal), p(row_loss), p(dx), ps_(dw), p(ws), n,
                                                                   st)), calls),
            act_ms=median_ms(lambda: _lib.check(L.ocrl_c51_act(ctypes.byref(d), p(x), ps_(w), V_MIN, V_MAX, 1, 0, 0.1, None, p(acts_out), p(q), st)), calls),
            target_ms=median_ms(lambda: _lib.check(L.ocrl_c51_fwd(ctypes.byref(d), p(x), ps_(w), V_MIN, V_MAX, None, p(probs), p(q), 0, None, 0, st)), calls),
            n_floats=sum(t.numel() for t in w))
        for k in ("td_ms", "act_ms", "target_ms"):
            res[name][k.replace("_ms", "_ratio")] = round(res[name][k] / res["scalar"][k], 3)
    for r in res.values():
        for k in ("td_ms", "act_ms", "target_ms"):
            r[k] = round(r[k], 5)
    out["heads"] = dict(res, batch=B, features=F, actions=A, atoms=Z)


def bench_train_step(calls, out):
    models = {}
    for sb3 in ("dqn_per", "dqn_c51"):
        c = compose(os.path.join(ROOT, "configs"), "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4",
                                                                 "device=cuda:0", "sb3.algo_kwargs.buffer_size=4096", f"sb3.algo_kwargs.batch_size={B}"])
        _, _, model = train_sb3.build(c)
        model._total_timesteps = 1 << 20
        for _ in range(64):
            model.collect_step()
        models[sb3] = model
    ms = {k: [] for k in models}
    for _ in range(3):                                      # the two alternating: drift of the machine lands on both
        for k, m in models.items():
            ms[k].append(median_ms(m.train_step, calls))
    res = {k: round(sorted(v)[1], 5) for k, v in ms.items()}
    out["train_step_gt"] = dict(res, ratio=round(res["dqn_c51"] / res["dqn_per"], 3), batch=B, rounds={k: [round(t, 5) for t in v] for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_c51: no GPU: the times are taken on the device or not at all")
    out = {}
    bench_heads(a.calls, out)
    bench_train_step(a.calls, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
