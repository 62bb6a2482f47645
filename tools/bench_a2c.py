"""What one A2C update (ocrl_amd.sb3s.A2C.train: a2c_loss, backward, ocrl_flat_clip_rmsprop_l2, one device read) costs, against the eager
torch chain with the same arithmetic: configs/sb3_acnet/mlp.yaml on F = 128 features behind an identity extractor, 4 actions.

    train16 / train80   ms per ``A2C.train()`` on a filled rollout buffer of B = T * E = 16 (4 x 4) and 80 (5 x 16) rows; the eager side
                        is the network of tests/acnet_ref.py under autograd (what ``evaluate_actions`` computes), the loss of
                        tests/a2c_ref.a2c, ``backward``, ``clip_grad_norm_`` and the fp32 RMSpropTFLike update written out on the
                        parameter list (``_foreach`` calls), with the same read of the four scalars and the norm at the end

ms per call = the median over `--calls` individually timed calls after warm-up, each between two events on the stream (tools/bench_acnet.py's
method); both sides are timed from Python, as the loop calls them, and both end in one device read."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ocrl_amd.sb3s import A2C, CustomActorCriticPolicy, RolloutBuffer  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from tests import a2c_ref  # noqa: E402
from tests import acnet_ref as R  # noqa: E402
from tools.bench_acnet import ACTS, DIMS, median_ms  # noqa: E402

F, A = 128, 4
LR, ALPHA, EPS, MAX_NORM = 7e-4, 0.99, 1e-5, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = types.SimpleNamespace(sb3_acnet=compose(os.path.join(root, "configs", "sb3_acnet"), "mlp"))
    out = {}
    for T, E in ((4, 4), (5, 16)):
        B = T * E
        torch.manual_seed(0)
        pol = CustomActorCriticPolicy(types.SimpleNamespace(shape=(F,)), types.SimpleNamespace(n=A), config=cfg)
        env = types.SimpleNamespace(num_envs=E, observation_space=types.SimpleNamespace(shape=(F,)), action_space=types.SimpleNamespace(n=A))
        algo = A2C(pol, env, n_steps=T, learning_rate=LR, ent_coef=0.01)
        gen = torch.Generator().manual_seed(1)
        buf = RolloutBuffer(T, E, (F,), algo.device, 0.99, 1.0)
        for t in range(T):
            buf.add(torch.randn(E, F, generator=gen), torch.randint(0, A, (E,), generator=gen), torch.rand(E, generator=gen), torch.zeros(E),
                    torch.randn(E, generator=gen), -1.4 * torch.ones(E))
        buf.advantages.normal_()
        buf.returns.normal_()
        algo.rollout_buffer = buf
        flat = buf.flat()

        ps = [torch.nn.Parameter(p.detach().clone()) for p in pol._head_args()[3]]
        sq = [torch.ones_like(p) for p in ps]
        x, act, adv, ret = flat.observations.clone(), flat.actions.clone(), flat.advantages.clone(), flat.returns.clone()

        def torch_train():
            for p in ps:
                p.grad = None
            _, _, lg, vl = R.forward(x, ps, DIMS, ACTS)
            s = a2c_ref.a2c(lg, vl, act, adv, ret, 0.5, 0.01, False)
            s["loss"].backward()
            norm = torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
            gs = [p.grad for p in ps]
            with torch.no_grad():
                torch._foreach_mul_(sq, ALPHA)
                torch._foreach_addcmul_(sq, gs, gs, value=1 - ALPHA)
                avg = torch._foreach_sqrt(torch._foreach_add(sq, EPS))
                torch._foreach_addcdiv_(ps, gs, avg, value=-LR)
            return torch.stack([s[k].detach() for k in a2c_ref.SCALARS] + [norm]).tolist()

        out[f"train{B}"] = dict(hip_ms=round(median_ms(algo.train, a.calls), 5), torch_ms=round(median_ms(torch_train, a.calls), 5), n_floats=algo.flat_p.numel())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
