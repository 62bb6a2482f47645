"""What DQN's implicit quantile head costs beside the quantile one (include/ocrl_hip_iqn.h beside include/ocrl_hip_qr.h), in the same
run, at the configs' own shapes: the default head (net_arch (64, 64), ReLU) on F = 128 features, 4 actions, batch 32; IQN at iqn.yaml's
N = N' = 8 fractions per row (K = 32 for acting) and 64 cosines, and again at N = N' = K = 32, against QR-DQN's 50 quantiles with the
dueling stream.

    td            ms per ``ocrl_iqn_td_fwd_bwd`` (four launches) beside ``ocrl_qr_td_fwd_bwd`` (three)
    act           ms per ``ocrl_iqn_act`` at K fractions drawn in the kernel beside ``ocrl_qr_act`` (one launch each)
    target        ms per target forward without a workspace: ``ocrl_iqn_fwd`` writing quantiles and q (two launches) beside ``ocrl_qr_fwd``
    taus          ms per ``ocrl_iqn_taus`` [32, N] (one launch; an update makes two, three under double Q)
    train_step    ms per ``DQN.train_step()`` of configs/sb3/iqn.yaml beside configs/sb3/qrdqn.yaml behind the ground-truth encoder
                  (ocr=gt, pooling=mlp), batch 32, alternating; and of iqn.yaml at N = N' = K = 32
    collect_step  ms per ``DQN.collect_step()`` (four on-device environments, one act launch) of the same three

ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream (tools/bench_acnet.py's
method), timed from Python through ctypes as the loop calls them.  There is no threshold.  The expectation to confirm or refute: the
head's cost follows the B * N expanded rows, 16 row tiles at batch 32 and N = 8 (64 at N = 32) against QR-DQN's 2; the tiles run on
workgroups of their own, so the time grows with the tiles only once they outnumber what the device runs side by side."""
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
from tools.bench_c51 import ACTS, DIMS, A, B, F, GAMMA, params  # noqa: E402
from tools.bench_qr import KAPPA  # noqa: E402
from tools.bench_qr import N as NQ  # noqa: E402

C = 64
SAMPLES = ((8, 8, 32), (32, 32, 32))            # (N, N', K): iqn.yaml's, then all 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"qrdqn": ("qrdqn", ()), "iqn": ("iqn", ()),
           "iqn_32": ("iqn", ("sb3.algo_kwargs.n_tau_samples=32", "sb3.algo_kwargs.n_tau_prime_samples=32", "sb3.algo_kwargs.n_act_samples=32"))}


def bench_heads(calls, out):
    L, p, ps_ = _lib.lib(), _lib.ptr, _lib.ptrs
    st = _lib.stream()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, F, generator=g).cuda()
    actions, rewards = torch.randint(0, A, (B,), generator=g).cuda(), torch.rand(B, generator=g).cuda()
    dones = (torch.arange(B) % 5 == 0).to(torch.uint8).cuda()
    next_q = torch.randn(B, A, generator=g).cuda()
    scal, row_loss, dx = torch.empty(3, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, F, device="cuda")
    acts_out, q = torch.empty(B, device="cuda", dtype=torch.int64), torch.empty(B, A, device="cuda")
    res = {}
    d = _lib.qr_desc(B, F, A, NQ, DIMS, ACTS, True)
    w = params((A * NQ, NQ))
    dw = [torch.empty_like(t) for t in w]
    n = L.ocrl_qr_ws_floats(ctypes.byref(d))
    ws = torch.empty(n, device="cuda")
    next_quantiles, theta = torch.randn(B, A, NQ, generator=g).cuda(), torch.empty(B, A, NQ, device="cuda")
    res["qr_dueling"] = dict(
        td_ms=median_ms(lambda: _lib.check(L.ocrl_qr_td_fwd_bwd(ctypes.byref(d), p(x), ps_(w), p(next_quantiles), p(next_q), p(actions), p(rewards), p(dones),
                                                              None, None, GAMMA, KAPPA, p(scal), p(row_loss), p(dx), ps_(dw), p(ws), n, st)), calls),
        act_ms=median_ms(lambda: _lib.check(L.ocrl_qr_act(ctypes.byref(d), p(x), ps_(w), 1, 0, 0.1, None, p(acts_out), p(q), st)), calls),
        target_ms=median_ms(lambda: _lib.check(L.ocrl_qr_fwd(ctypes.byref(d), p(x), ps_(w), p(theta), p(q), 0, None, 0, st)), calls),
        n_floats=sum(t.numel() for t in w), row_tiles=(B + 15) // 16)
    emb = [((torch.rand(F, C, generator=g) * 2 - 1) / C ** 0.5).cuda(), torch.zeros(F).cuda()]
    w = emb + params((A,))
    dw = [torch.empty_like(t) for t in w]
    for N, Np, K in SAMPLES:
        d, dp, dk = (_lib.iqn_desc(B, F, A, m, C, DIMS, ACTS) for m in (N, Np, K))
        n = L.ocrl_iqn_ws_floats(ctypes.byref(d))
        ws = torch.empty(n, device="cuda")
        taus, taus_p = torch.rand(B, N, generator=g).cuda(), torch.rand(B, Np, generator=g).cuda()
        next_quantiles, theta = torch.randn(B, A, Np, generator=g).cuda(), torch.empty(B, A, Np, device="cuda")
        r = dict(
            td_ms=median_ms(lambda: _lib.check(L.ocrl_iqn_td_fwd_bwd(ctypes.byref(d), p(x), p(taus), ps_(w), p(next_quantiles), Np, p(next_q), p(actions),
                                                                   p(rewards), p(dones), None, None, GAMMA, KAPPA, p(scal), p(row_loss), p(dx), ps_(dw), p(ws),
                                                                   n, st)), calls),
            act_ms=median_ms(lambda: _lib.check(L.ocrl_iqn_act(ctypes.byref(dk), p(x), ps_(w), 1, 0, 0.1, None, None, p(acts_out), p(q), st)), calls),
            target_ms=median_ms(lambda: _lib.check(L.ocrl_iqn_fwd(ctypes.byref(dp), p(x), p(taus_p), ps_(w), p(theta), p(q), 0, None, 0, st)), calls),
            taus_ms=median_ms(lambda: _lib.check(L.ocrl_iqn_taus(1, 0, B, N, p(taus), st)), calls),
            n_floats=sum(t.numel() for t in w), row_tiles=(B * N + 15) // 16)
        for k in ("td_ms", "act_ms", "target_ms"):
            r[k.replace("_ms", "_over_qr")] = round(r[k] / res["qr_dueling"][k], 3)
        res[f"iqn_N{N}_K{K}"] = r
    for r in res.values():
        for k in ("td_ms", "act_ms", "target_ms", "taus_ms"):
            if k in r:
                r[k] = round(r[k], 5)
    out["heads"] = dict(res, batch=B, features=F, actions=A, quantiles=NQ, cosines=C)


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
    for what, step in (("train_step", lambda m: m.train_step), ("collect_step", lambda m: m.collect_step)):
        ms = {k: [] for k in models}
        for _ in range(3):                                  # alternating: drift of the machine lands on all
            for k, m in models.items():
                ms[k].append(median_ms(step(m), calls))
        res = {k: round(sorted(v)[1], 5) for k, v in ms.items()}
        out[f"{what}_gt"] = dict(res, iqn_over_qrdqn=round(res["iqn"] / res["qrdqn"], 3), iqn_32_over_iqn=round(res["iqn_32"] / res["iqn"], 3), batch=B,
                                 rounds={k: [round(t, 5) for t in v] for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iqn: no GPU: the times are taken on the device or not at all")
    out = {}
    bench_heads(a.calls, out)
    bench_loop(a.calls, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
