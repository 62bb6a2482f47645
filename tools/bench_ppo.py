"""What the PPO loop (ocrl_amd.sb3s.ppo) pays per environment step and per minibatch update, against the torch chain it replaces:
configs/sb3_acnet/mlp.yaml on F = 128 features, 4 actions.

    act4 / act32   ms per ``policy.forward`` on E = 4 and E = 32 rows with the sampler inside the head's launch (``set_sampling``:
                   ocrl_acnet_act) and with the eager tail (ocrl_acnet_fwd, then log_softmax, exp, multinomial, gather)
    step           ms per optimiser step on the policy's parameters: ocrl_flat_clip_adam_l2 on the flat buffers against
                   clip_grad_norm_ + torch.optim.Adam(eps=1e-5) over the parameter list

ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream (tools/bench_acnet.py's
method); both sides are timed from Python, as the loop calls them."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd import _lib  # noqa: E402
from ocrl_amd.sb3s import CustomActorCriticPolicy  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from tools.bench_acnet import median_ms  # noqa: E402

F, A = 128, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = types.SimpleNamespace(sb3_acnet=compose(os.path.join(root, "configs", "sb3_acnet"), "mlp"))
    torch.manual_seed(0)
    pol = CustomActorCriticPolicy(types.SimpleNamespace(shape=(F,)), types.SimpleNamespace(n=A), config=cfg).cuda()
    out = {}
    with torch.no_grad():
        for E in (4, 32):
            x = torch.randn(E, F, device="cuda")
            pol.set_sampling(0)
            fused = median_ms(lambda: pol(x), a.calls)
            pol.set_sampling(None)
            eager = median_ms(lambda: pol(x), a.calls)
            out[f"act{E}"] = dict(fused_ms=round(fused, 5), eager_tail_ms=round(eager, 5))
    params = list(pol.parameters())
    n = sum((p.numel() + 3) & ~3 for p in params)
    L, p = _lib.lib(), _lib.ptr
    fp, fg, fm, fv = (torch.zeros(n, device="cuda") for _ in range(4))
    fg.normal_()
    nws = L.ocrl_flat_clip_adam_ws_floats()
    ws, norm, st = torch.empty(nws, device="cuda"), torch.empty(1, device="cuda"), _lib.stream()
    step = [0]

    def hip_step():
        step[0] += 1
        _lib.check(L.ocrl_flat_clip_adam_l2(p(fp), p(fg), p(fm), p(fv), n, 0.5, 3e-4, 0.9, 0.999, 1e-5, step[0], p(norm), p(ws), nws, st))

    for q in params:
        q.grad = torch.randn_like(q)
    opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()

    out["step"] = dict(n_tensors=len(params), n_floats=n, hip_ms=round(median_ms(hip_step, a.calls), 5), torch_ms=round(median_ms(torch_step, a.calls), 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
