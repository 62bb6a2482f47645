"""What FQF costs (include/ocrl_hip_fqf.h), in one run, behind the ground-truth encoder (ocr=gt, pooling=mlp): batch 32 for an update, 16
environments for acting, 32 fractions per row.

    act           us per acting step on 16 rows of features: FQF's two launches (``ocrl_fqf_fractions``, then ``ocrl_fqf_act``), each of
                  the two alone, and ``ocrl_iqn_act`` at the same N on given fractions
    train_step    ms per ``DQN.train_step()`` with ``fqf=True, n_tau_samples=32`` (configs/sb3/fqf.yaml) beside the implicit quantile
                  head's at ``n_tau_samples = n_tau_prime_samples = 32`` (iqn.yaml otherwise), batch 32, alternating.  The FQF step is the
                  IQN step without its three draws of fractions, plus the proposal's launch, two weighted folds (one under double Q
                  alone), one head forward at 63 fractions, the fraction loss's two launches and one RMSprop call

us / ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream
(tools/bench_acnet.py's method), timed from Python through ctypes as the loop calls them.  There is no threshold."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_sb3  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from tools.bench_acnet import median_ms  # noqa: E402

B, ENVS, N = 32, 16, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"iqn": ("iqn", (f"sb3.algo_kwargs.n_tau_samples={N}", f"sb3.algo_kwargs.n_tau_prime_samples={N}")), "fqf": ("fqf", ())}


def build(sb3, over):
    c = compose(os.path.join(ROOT, "configs"), "train_sb3", ["ocr=gt", "pooling=mlp", f"sb3={sb3}", "sb3_acnet=mlp", "env=target-N4C4S3S1", f"num_envs={ENVS}",
                                                             "device=cuda:0", "sb3.algo_kwargs.buffer_size=4096", f"sb3.algo_kwargs.batch_size={B}", *over])
    _, _, model = train_sb3.build(c)
    model._total_timesteps = 1 << 20
    for _ in range(16):
        model.collect_step()
    return model


def bench_act(models, calls, out):
    iqn, fqf = models["iqn"].policy, models["fqf"].policy
    with torch.no_grad():
        obs = models["fqf"]._obs(models["fqf"]._last_obs)
        xf, xi = fqf.extract_features(obs).contiguous(), iqn.extract_features(obs).contiguous()
        taus = fqf.q_net.fractions(xf).taus
        given = torch.rand(ENVS, N, device=xf.device)
        us = lambda fn: round(median_ms(fn, calls) * 1e3, 2)
        res = dict(fqf_two_launches_us=us(lambda: fqf.q_net.act(xf, 1, 0, 0.05, None)), fqf_fractions_us=us(lambda: fqf.q_net.fractions(xf)),
                   fqf_act_us=us(lambda: fqf.q_net.act(xf, 1, 0, 0.05, None, taus=taus)),
                   iqn_act_us=us(lambda: iqn.q_net.act(xi, 1, 0, 0.05, None, taus=given)))
    out["act"] = dict(res, fqf_over_iqn=round(res["fqf_two_launches_us"] / res["iqn_act_us"], 3), rows=ENVS, fractions=N)


def bench_loop(models, calls, out):
    ms = {k: [] for k in models}
    for _ in range(3):                                  # alternating: drift of the machine lands on both
        for k, m in models.items():
            ms[k].append(median_ms(m.train_step, calls))
    res = {k: round(sorted(v)[1], 5) for k, v in ms.items()}
    out["train_step_gt"] = dict(res, fqf_over_iqn=round(res["fqf"] / res["iqn"], 3), batch=B, fractions=N,
                                rounds={k: [round(t, 5) for t in v] for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fqf: no GPU: the times are taken on the device or not at all")
    models = {k: build(*v) for k, v in CONFIGS.items()}
    out = {}
    bench_act(models, a.calls, out)
    bench_loop(models, a.calls, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
