"""What the noisy linear layers cost (include/ocrl_hip_noisy.h): ``sb3=rainbow`` against ``sb3=dqn_c51`` in the same run, at the configs' own
shapes (the default head, net_arch (64, 64), 51 atoms, dueling, behind ocr=gt and pooling=mlp, 4 environments, batch 32).

    entries       ms per ``ocrl_noisy_factors``, ``ocrl_noisy_perturb`` and ``ocrl_noisy_grad`` (one launch each) on the head's four layers
    act           ms per ``policy.act`` on the features of a vec step: rainbow regenerates the effective weights of a draw first (two more
                  launches), dqn_c51 flips its coin
    train_step    ms per ``DQN.train_step()``: rainbow makes the effective weights three times (the online network's for the loss and for
                  double Q-learning, the target network's) and forms the sigmas' gradient once: seven more launches

ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream (tools/bench_acnet.py's
method); the two configs alternate in three rounds and the middle round's median counts, so drift of the machine lands on both.  Calls of
this size are a handful of launches of a few workgroups: the figures are launch and latency costs, not throughput."""
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

B = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("dqn_c51", "rainbow")


def bench_entries(calls, model, out):
    L, st = _lib.lib(), _lib.stream()
    net = model.policy.q_net
    mods = [m for m in net.q_net if isinstance(m, torch.nn.Linear)] + [net.value_net]
    mu = [p.detach() for m in mods for p in (m.weight, m.bias)]
    sigma = [p.detach() for m in mods for p in (m.weight_sigma, m.bias_sigma)]
    layers = [(m.in_features, m.out_features) for m in mods]
    d = _lib.noisy_desc(layers)
    fac = torch.empty(L.ocrl_noisy_factor_floats(ctypes.byref(d)), device="cuda")
    w_eff, dsigma = [torch.empty_like(p) for p in mu], [torch.empty_like(p) for p in mu]
    dw = [torch.randn_like(p) for p in mu]
    out["entries"] = dict(
        factors_ms=round(median_ms(lambda: _lib.check(L.ocrl_noisy_factors(ctypes.byref(d), 1, 2, None, _lib.ptr(fac), st)), calls), 5),
        perturb_ms=round(median_ms(lambda: _lib.check(L.ocrl_noisy_perturb(ctypes.byref(d), _lib.ptrs(mu), _lib.ptrs(sigma), _lib.ptr(fac),
                                                                          _lib.ptrs(w_eff), st)), calls), 5),
        grad_ms=round(median_ms(lambda: _lib.check(L.ocrl_noisy_grad(ctypes.byref(d), _lib.ptrs(dw), _lib.ptr(fac), _lib.ptrs(dsigma), st)), calls), 5),
        layers=layers, n_floats=sum(p.numel() for p in mu), factor_floats=fac.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noisy: no GPU: the times are taken on the device or not at all")
    models = {}
    for sb3 in CONFIGS:
        c = compose(os.path.join(ROOT, "configs"), "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", "num_envs=4",
                                                                 "device=cuda:0", "sb3.algo_kwargs.buffer_size=4096", f"sb3.algo_kwargs.batch_size={B}"])
        _, _, model = train_sb3.build(c)
        model._total_timesteps = 1 << 20
        for _ in range(64):
            model.collect_step()
        models[sb3] = model
    out = {}
    bench_entries(a.calls, models["rainbow"], out)
    feats = {}
    with torch.no_grad():
        for k, m in models.items():
            m.policy.eval()
            m.policy.set_noise(m.noise_draws)
            feats[k] = m.policy.extract_features(m._obs(m._last_obs))

    def act(k):
        with torch.no_grad():
            models[k].policy.act(feats[k], epsilon=models[k].epsilon())

    for name, fn in (("act", act), ("train_step", lambda k: models[k].train_step())):
        ms = {k: [] for k in models}
        for _ in range(3):
            for k in models:
                ms[k].append(median_ms(lambda: fn(k), a.calls))
        res = {k: round(sorted(v)[1], 5) for k, v in ms.items()}
        out[name] = dict(res, ratio=round(res["rainbow"] / res["dqn_c51"], 3), extra_ms=round(res["rainbow"] - res["dqn_c51"], 5),
                         rounds={k: [round(t, 5) for t in v] for k, v in ms.items()})
    out["shapes"] = dict(envs=4, batch=B)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
