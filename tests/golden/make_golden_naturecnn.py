"""Generate the golden vectors of the NatureCNN and MultipleCNN encoders from the reference's own modules.

Runs ONLY in the build container (needs /root/reference): imports ``ocrs.naturecnn.naturecnn_module.NatureCNN_Module`` and
``ocrs.multiple_cnns.multiple_cnn_module.MultipleCNN_Module`` with their heavy imports stubbed (``utils.tools``, ``ocrs.base``, omegaconf's
``open_dict``), loads closed-form weights (``closed_form``), runs seeded observations (``observations``) forward and
``(out * cotangent).sum()`` backward, and writes tests/golden/naturecnn.npz and multiple_cnn.npz (``fixture_path``).  Every case records
its state_dict names and shapes, rep_dim and num_slots, and its output.  Gradients of at most FULL_MAX entries (the biases) are kept
whole; the weight gradients keep per-tensor moments and a fixed strided sample.
The helpers below need neither the reference nor a GPU: the tests import them to rebuild the same inputs.

    python tests/golden/make_golden_naturecnn.py
"""
import contextlib
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# tag: (encoder, obs_size, batch, config)
CASES = {
    "default": ("NatureCNN", 64, 2, dict(rep_dim=512, use_cnn_feat=False, cnn_feat_size=4)),
    "feat4": ("NatureCNN", 64, 2, dict(rep_dim=512, use_cnn_feat=True, cnn_feat_size=4)),
    "feat2": ("NatureCNN", 64, 2, dict(rep_dim=512, use_cnn_feat=True, cnn_feat_size=2)),
    "size2_flat": ("NatureCNN", 64, 2, dict(rep_dim=64, use_cnn_feat=False, cnn_feat_size=2)),
    "obs84": ("NatureCNN", 84, 2, dict(rep_dim=512, use_cnn_feat=False, cnn_feat_size=4)),
    "multi2": ("MultipleCNN", 64, 3, dict(rep_dim=16, num_modules=2)),
}
OBS_CHANNELS = 3
NSAMPLE = 509
FULL_MAX = 4096


def fixture_path(tag):
    return os.path.join(HERE, "multiple_cnn.npz" if CASES[tag][0] == "MultipleCNN" else "naturecnn.npz")


def config(tag):
    return types.SimpleNamespace(name=CASES[tag][0], **CASES[tag][3])


def env_config(tag):
    return types.SimpleNamespace(obs_size=CASES[tag][1], obs_channels=OBS_CHANNELS)


def closed_form(shape, t):
    """tensor t of the encoder: a smooth pseudo-random pattern, weights scaled by 1/sqrt(fan_in) so that ReLUs stay half open"""
    n = int(np.prod(shape))
    k = torch.arange(n, dtype=torch.float64)
    v = torch.sin(k * 0.7548776662 + 1.37 * t + 0.3) + 0.35 * torch.cos(k * 0.5698402910 + 0.71 * t)
    if len(shape) >= 2:
        v = v * (1.6 / math.sqrt(int(np.prod(shape[1:]))))
    else:
        v = v * 0.05
    return v.float().reshape(shape)


def load_closed_form(module):
    """every parameter of `module` set to closed_form(shape, position in the state_dict)"""
    sd = module.state_dict()
    module.load_state_dict({k: closed_form(tuple(v.shape), i) for i, (k, v) in enumerate(sd.items())})


def observations(tag):
    _, S, B, _ = CASES[tag]
    return torch.rand(B, OBS_CHANNELS, S, S, generator=torch.Generator().manual_seed(300 + list(CASES).index(tag)))


def cotangent(tag, shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(400 + list(CASES).index(tag)))


def sample(t):
    """per-tensor moments (sum, sum |.|, sum of squares) and a fixed strided sample of at most NSAMPLE entries"""
    t = t.detach().double().flatten().cpu()
    return np.concatenate([np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()]),
                           t[:: max(1, t.numel() // NSAMPLE)][:NSAMPLE].numpy()])


def import_reference():
    sys.path.insert(0, REF)
    for n in ("wandb", "h5py"):
        sys.modules.setdefault(n, types.ModuleType(n))
    oc = types.ModuleType("omegaconf")
    oc.OmegaConf = object
    oc.open_dict = lambda cfg: contextlib.nullcontext(cfg)
    sys.modules["omegaconf"] = oc
    utils = types.ModuleType("utils")
    utils.__path__ = []
    tools = types.ModuleType("utils.tools")
    tools.Tensor = torch.Tensor
    sys.modules["utils"], sys.modules["utils.tools"] = utils, tools
    pkg = types.ModuleType("ocrs")
    pkg.__path__ = [os.path.join(REF, "ocrs")]
    sys.modules["ocrs"] = pkg
    base = types.ModuleType("ocrs.base")
    base.Base = object
    sys.modules["ocrs.base"] = base
    from ocrs.multiple_cnns.multiple_cnn_module import MultipleCNN_Module  # noqa
    from ocrs.naturecnn.naturecnn_module import NatureCNN_Module  # noqa
    return dict(NatureCNN=NatureCNN_Module, MultipleCNN=MultipleCNN_Module)


def main():
    mods = import_reference()
    torch.manual_seed(0)
    fx, inventory = {}, {}                      # keyed by fixture file
    for tag, (enc, S, B, _) in CASES.items():
        m = mods[enc](config(tag), env_config(tag))
        load_closed_form(m)
        sd = m.state_dict()
        path = fixture_path(tag)
        fx.setdefault(path, {})
        inventory.setdefault(path, {})[tag] = dict(rep_dim=int(m.rep_dim), num_slots=int(m.num_slots),
                                                   params=[[k, list(v.shape)] for k, v in sd.items()])
        out = m(observations(tag))
        cot = cotangent(tag, out.shape)
        (out * cot).sum().backward()
        f = fx[path]
        f[tag + ":out"] = out.detach().numpy()
        for k, p in m.named_parameters():
            f[tag + ":g:" + k] = p.grad.numpy() if p.numel() <= FULL_MAX else sample(p.grad)
        print(f"[{tag}] out {tuple(out.shape)} |out| {out.abs().max().item():.3e} open {(out > 0).float().mean().item():.2f}")
    for path, f in fx.items():
        f["inventory"] = np.array(json.dumps(inventory[path]))
        np.savez_compressed(path, **f)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
