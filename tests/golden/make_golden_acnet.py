"""Generate tests/golden/acnet.npz from the reference's own CustomNetwork (sb3s/custom_acnets.py:8-96).

Runs ONLY in the build container (needs /root/reference).  Import recipe: the reference on sys.path; empty stub modules for wandb, h5py,
omegaconf and gym (gym.spaces with Space and Box); stubs for stable_baselines3(.common(.policies)) whose ActorCriticPolicy is a bare
nn.Module subclass; a namespace package ``sb3s`` whose __path__ is the reference's folder; then
``from sb3s.custom_acnets import CustomNetwork``.  stable-baselines3 itself is not available, so the heads (action_net, value_net) and the
PPO loss are built here with plain torch on top of the reference's CustomNetwork, from the published algorithm.

Per case: closed-form weights, seeded features, the reference's latent_pi / latent_vf, logits, values, the six PPO scalars and every
gradient of loss.backward(); plus the identity configuration's behaviour and the state_dict key lists.
The helpers below need neither the reference nor a GPU: the tests import them to rebuild the same inputs.

    python tests/golden/make_golden_acnet.py
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
FIXTURE = os.path.join(HERE, "acnet.npz")
SCALARS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")
CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01

# tag: (feature_dim, batch, actions, config)
CASES = {
    "mlp": (128, 32, 4, dict(shared_net=dict(dims=[64, 64], acts=["relu", "relu"]), policy_net=dict(dims=[64], acts=["tanh"]),
                             value_net=dict(dims=[64], acts=["tanh"]))),
    "value2": (67, 32, 18, dict(shared_net=dict(dims=[], acts=[]), policy_net=dict(dims=[], acts=[]),
                                value_net=dict(dims=[64, 32], acts=["tanh", "relu"]))),
}
IDENTITY = dict(shared_net=dict(dims=[], acts=[]), policy_net=dict(dims=[], acts=[]), value_net=dict(dims=[], acts=[]))


def _ns(d):
    return types.SimpleNamespace(**{k: _ns(v) if isinstance(v, dict) else v for k, v in d.items()})


def case_config(tag):
    return _ns(dict(ortho_init=False, **(IDENTITY if tag == "identity" else CASES[tag][3])))


def closed_form(shape, t):
    """tensor t of a network: a smooth pseudo-random pattern, weights scaled by 1/sqrt(fan_in)"""
    n = int(np.prod(shape))
    k = torch.arange(n, dtype=torch.float64)
    v = torch.sin(k * 0.7548776662 + 1.37 * t + 0.3) + 0.35 * torch.cos(k * 0.5698402910 + 0.71 * t)
    v = v * (1.6 / math.sqrt(shape[1])) if len(shape) == 2 else v * 0.05
    return v.float().reshape(shape)


def inputs(tag):
    """features, actions, old_log_prob shifts, advantages, returns of a case (seeded)"""
    F, B, A, _ = CASES[tag]
    gen = torch.Generator().manual_seed(300 + list(CASES).index(tag))
    return dict(features=torch.randn(B, F, generator=gen), actions=torch.randint(0, A, (B,), generator=gen),
                shift=(torch.arange(B) % 3 - 1).float() * 0.35, advantages=torch.randn(B, generator=gen), returns=torch.randn(B, generator=gen))


def import_reference():
    for name in ("wandb", "h5py", "omegaconf", "gym", "gym.spaces", "stable_baselines3", "stable_baselines3.common",
                 "stable_baselines3.common.policies"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["gym"].spaces = sys.modules["gym.spaces"]
    sys.modules["gym.spaces"].Space = type("Space", (), {})
    sys.modules["gym.spaces"].Box = type("Box", (), {})
    sys.modules["stable_baselines3.common.policies"].ActorCriticPolicy = type("ActorCriticPolicy", (torch.nn.Module,), {})
    pkg = types.ModuleType("sb3s")
    pkg.__path__ = [os.path.join(REF, "sb3s")]
    sys.modules["sb3s"] = pkg
    sys.path.insert(0, REF)
    from sb3s.custom_acnets import CustomNetwork
    return CustomNetwork


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import acnet_ref as R
    CustomNetwork = import_reference()
    out = {}
    for tag, (F, B, A, _) in CASES.items():
        net = CustomNetwork(F, case_config(tag))
        sd = net.state_dict()
        net.load_state_dict({k: closed_form(tuple(v.shape), i) for i, (k, v) in enumerate(sd.items())})
        action_net, value_net = torch.nn.Linear(net.latent_dim_pi, A), torch.nn.Linear(net.latent_dim_vf, 1)
        with torch.no_grad():
            for i, p in enumerate((action_net.weight, action_net.bias, value_net.weight, value_net.bias)):
                p.copy_(closed_form(tuple(p.shape), len(sd) + i))
        inp = inputs(tag)
        x = inp["features"].clone().requires_grad_(True)
        lp, lv = net(x)
        logits, values = action_net(lp), value_net(lv)[:, 0]
        logp = torch.log_softmax(logits.detach(), -1).gather(1, inp["actions"][:, None])[:, 0]
        old = logp - inp["shift"]
        s = R.ppo(logits, values, inp["actions"], old, inp["advantages"], inp["returns"], CLIP, VF_COEF, ENT_COEF, True)
        s["loss"].backward()
        out[f"{tag}.keys"] = np.array(list(sd))
        out[f"{tag}.latent_dims"] = np.array([net.latent_dim_pi, net.latent_dim_vf])
        for k, v in net.state_dict().items():
            out[f"{tag}.w.{k}"] = v.numpy()
            out[f"{tag}.shape.{k}"] = np.array(v.shape)
        for h, m in (("action_net", action_net), ("value_net", value_net)):
            for k, p in m.named_parameters():
                out[f"{tag}.{h}.{k}"] = p.detach().numpy()
                out[f"{tag}.grad.{h}.{k}"] = p.grad.numpy()
        for k, p in net.named_parameters():
            out[f"{tag}.grad.w.{k}"] = p.grad.numpy()
        out[f"{tag}.grad.features"] = x.grad.numpy()
        for k, v in (("features", inp["features"]), ("actions", inp["actions"]), ("old_log_prob", old), ("advantages", inp["advantages"]),
                     ("returns", inp["returns"]), ("latent_pi", lp), ("latent_vf", lv), ("logits", logits), ("values", values)):
            out[f"{tag}.{k}"] = v.detach().numpy()
        out[f"{tag}.scalars"] = np.array([s[k].item() for k in SCALARS], dtype=np.float64)
    ident = CustomNetwork(24, case_config("identity"))
    x = torch.randn(3, 24)
    a, b = ident(x)
    out["identity.keys"] = np.array(list(ident.state_dict()), dtype="U1")
    out["identity.returns_input"] = np.array([a is x, b is x])
    out["identity.latent_dims"] = np.array([ident.latent_dim_pi, ident.latent_dim_vf])
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {FIXTURE}: {os.path.getsize(FIXTURE)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
