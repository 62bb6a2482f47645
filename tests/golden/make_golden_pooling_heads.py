"""Generate the golden vectors of the RN, MLP and Identity pooling heads from the reference's own modules.

Runs ONLY in the build container (needs /root/reference; import recipe = SURVEY.md Appendix C, as make_golden_pooling.py): imports
``poolings.rn.rn_module.RN_Module``, ``poolings.mlp.mlp_module.MLP_Module`` and ``poolings.identity.identity_module.Identity_Module``,
loads closed-form weights (``closed_form``), runs seeded slots (``slots``) forward and ``(out * cotangent).sum()`` backward, and writes
one fixture per head, tests/golden/pooling_{rn,mlp,identity}.npz (``fixture_path``).  Every head records its state_dict names and
shapes and its rep_dim.  Small cases keep full gradients; the default RN (6 x 192 slots, configs/pooling/rn.yaml) and the default MLP
keep per-tensor moments and a fixed strided sample.
The helpers below need neither the reference nor a GPU: the tests import them to rebuild the same inputs.

    python tests/golden/make_golden_pooling_heads.py
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# tag: (head, rep_dim, num_slots, batch, config, full gradients)
CASES = {
    "rn_small": ("RN", 32, 5, 3, dict(g_dims=[64, 64], f_dims=[64, 32]), True),
    "rn_default": ("RN", 192, 6, 2, dict(g_dims=[256, 256, 256, 256], f_dims=[256, 128, 64, 64]), False),
    "mlp_default": ("MLP", 192, 6, 3, dict(dims=[128, 128], acts=["relu", "relu"]), False),
    "mlp_linear": ("MLP", 30, 3, 4, dict(dims=[64, 32, 16], acts=["relu", "none", "relu"]), True),
    "identity": ("Identity", 192, 6, 2, dict(), True),
}
NSAMPLE = 509


def fixture_path(tag):
    return os.path.join(HERE, f"pooling_{CASES[tag][0].lower()}.npz")


def config(tag):
    return types.SimpleNamespace(name=CASES[tag][0], **CASES[tag][4])


def closed_form(shape, t):
    """tensor t of a head: a smooth pseudo-random pattern, weights scaled by 1/sqrt(fan_in) so that ReLUs stay half open"""
    n = int(np.prod(shape))
    k = torch.arange(n, dtype=torch.float64)
    v = torch.sin(k * 0.7548776662 + 1.37 * t + 0.3) + 0.35 * torch.cos(k * 0.5698402910 + 0.71 * t)
    if len(shape) == 2:
        v = v * (1.6 / math.sqrt(shape[1]))
    else:
        v = v * 0.05
    return v.float().reshape(shape)


def load_closed_form(module):
    """every parameter of `module` set to closed_form(shape, position in the state_dict)"""
    sd = module.state_dict()
    module.load_state_dict({k: closed_form(tuple(v.shape), i) for i, (k, v) in enumerate(sd.items())})


def slots(tag):
    _, D, K, B, _, _ = CASES[tag]
    return torch.randn(B, K, D, generator=torch.Generator().manual_seed(100 + list(CASES).index(tag)))


def cotangent(tag, rep_dim):
    B = CASES[tag][3]
    return torch.randn(B, rep_dim, generator=torch.Generator().manual_seed(200 + list(CASES).index(tag)))


def sample(t):
    """per-tensor moments (sum, sum |.|, sum of squares) and a fixed strided sample of at most NSAMPLE entries"""
    t = t.detach().double().flatten().cpu()
    return np.concatenate([np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()]),
                           t[:: max(1, t.numel() // NSAMPLE)][:NSAMPLE].numpy()])


def import_reference():
    sys.path.insert(0, REF)
    for n in ("wandb", "h5py", "omegaconf"):
        sys.modules.setdefault(n, types.ModuleType(n))
    pkg = types.ModuleType("poolings")
    pkg.__path__ = [os.path.join(REF, "poolings")]
    sys.modules["poolings"] = pkg
    from poolings.identity.identity_module import Identity_Module  # noqa
    from poolings.mlp.mlp_module import MLP_Module  # noqa
    from poolings.rn.rn_module import RN_Module  # noqa
    return dict(RN=RN_Module, MLP=MLP_Module, Identity=Identity_Module)


def build(mods, tag):
    head, D, K, _, _, _ = CASES[tag]
    if head == "RN":
        return mods["RN"](D, K, 1, config(tag))
    return mods[head](D, K, config(tag))


def main():
    mods = import_reference()
    torch.manual_seed(0)
    fx, inventory = {}, {}                      # keyed by fixture file
    for tag, (head, D, K, B, _, full) in CASES.items():
        m = build(mods, tag)
        load_closed_form(m)
        sd = m.state_dict()
        path = fixture_path(tag)
        fx.setdefault(path, {})
        inventory.setdefault(path, {})[tag] = dict(rep_dim=int(m.rep_dim), params=[[k, list(v.shape)] for k, v in sd.items()])
        s = slots(tag).requires_grad_(True)
        out = m(s)
        cot = cotangent(tag, out.shape[1])
        (out * cot).sum().backward()
        f = fx[path]
        f[tag + ":out"] = out.detach().numpy()
        f[tag + ":dslots"] = s.grad.numpy() if full else sample(s.grad)
        for k, p in m.named_parameters():
            f[tag + ":g:" + k] = p.grad.numpy() if full else sample(p.grad)
        print(f"[{tag}] out {tuple(out.shape)} |out| {out.abs().max().item():.3e} open ReLUs "
              f"{', '.join(f'{(a > 0).float().mean().item():.2f}' for a in _relu_outputs(m, s))}")
    for path, f in fx.items():
        f["inventory"] = np.array(json.dumps(inventory[path]))
        np.savez_compressed(path, **f)
        print(path, os.path.getsize(path), "bytes")


def _relu_outputs(m, s):
    """fraction of open ReLUs per layer, a sanity print for the closed-form weights"""
    acts = []
    hooks = [mod.register_forward_hook(lambda _m, _i, o: acts.append(o.detach())) for mod in m.modules() if isinstance(mod, torch.nn.ReLU)]
    with torch.no_grad():
        m(s.detach())
    for h in hooks:
        h.remove()
    return acts


if __name__ == "__main__":
    main()
