"""Generate the golden vectors of the NatureCNN pooling heads from the reference's own modules.

Runs ONLY in the build container (needs /root/reference): imports ``poolings.cnn_linear.cnn_linear_module.CNN_Linear_Module`` and
``poolings.cnn_transformer.cnn_transformer_module.CNN_Transformer_Module`` with their heavy imports stubbed (``utils.tools`` is replaced
by a stub that carries ``Tensor`` and a ``slot_to_img`` of our own), loads closed-form weights (``load_weights``), runs seeded
tokens (``tokens``) forward and ``(out * cotangent).sum()`` backward, and writes tests/golden/pooling_cnn.npz.  Every case records its
state_dict names and shapes and rep_dim (``inventory``), and its output.  Gradients of at most FULL_MAX entries are kept whole; the
others, the token gradient among them, keep per-tensor moments and a fixed strided sample (``sample``).
The helpers below need neither the reference nor a GPU: the tests import them to rebuild the same inputs.

    python tests/golden/make_golden_pooling_cnn.py
"""
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pooling_oracle as PO  # noqa: E402
from tests.golden.make_golden_naturecnn import closed_form, sample  # noqa: E402,F401

# tag: (head, map side, token width, batch, pooling config)
CASES = {
    "linear64": ("CNN_Linear", 64, 67, 2, dict(rep_dim=512)),
    "trans64": ("CNN_Transformer", 64, 67, 2, dict(d_model=128, rep_dim=128, nhead=8, num_layers=1, pos_emb="ape")),
    "trans128": ("CNN_Transformer", 128, 67, 2, dict(d_model=128, rep_dim=128, nhead=8, num_layers=1, pos_emb="ape")),
}
FULL_MAX = 4096
FIXTURE = os.path.join(HERE, "pooling_cnn.npz")


def config(tag):
    return types.SimpleNamespace(name=CASES[tag][0], **CASES[tag][4])


def tokens(tag):
    """seeded feature-map tokens [B, side^2, D] in [-1, 1)"""
    _, S, D, B, _ = CASES[tag]
    return torch.rand(B, S * S, D, generator=torch.Generator().manual_seed(500 + list(CASES).index(tag))) * 2 - 1


def cotangent(tag, shape):
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.29 + 0.1 + list(CASES).index(tag)).reshape(shape).float()


def weights(module, tag):
    """closed-form state_dict of `module`: the convolutions and the Linear as closed_form(shape, position), the transformer as the
    pooling oracle's formula_params; the `pe` buffer stays the module's own"""
    sd = module.state_dict()
    out = {}
    if CASES[tag][0] == "CNN_Transformer":
        c = config(tag)
        out.update(PO.formula_params(PO.default_cfg(rep_dim=64, d_model=c.d_model, nhead=c.nhead, num_layers=c.num_layers)))
    for i, (k, v) in enumerate(sd.items()):
        if k.endswith(".pe"):
            out[k] = v
        elif k not in out:
            out[k] = closed_form(tuple(v.shape), i)
    assert set(out) == set(sd)
    return out


def import_reference():
    sys.path.insert(0, REF)
    for n in ("wandb", "h5py", "omegaconf"):
        sys.modules.setdefault(n, types.ModuleType(n))
    utils = types.ModuleType("utils")
    utils.__path__ = []
    tools = types.ModuleType("utils.tools")
    tools.Tensor = torch.Tensor
    tools.math = math                       # the reference's modules get `math` through `from utils.tools import *`

    def slot_to_img(slot):
        B, N, D = slot.shape
        s = math.isqrt(N)
        return slot.reshape(B, s, s, D).permute(0, 3, 1, 2)

    tools.slot_to_img = slot_to_img
    sys.modules["utils"], sys.modules["utils.tools"] = utils, tools
    pkg = types.ModuleType("poolings")
    pkg.__path__ = [os.path.join(REF, "poolings")]
    sys.modules["poolings"] = pkg
    from poolings.cnn_linear.cnn_linear_module import CNN_Linear_Module  # noqa
    from poolings.cnn_transformer.cnn_transformer_module import CNN_Transformer_Module  # noqa
    return dict(CNN_Linear=CNN_Linear_Module, CNN_Transformer=CNN_Transformer_Module)


def main():
    mods = import_reference()
    fx, inventory = {}, {}
    for tag, (head, S, D, B, _) in CASES.items():
        m = mods[head](D, S * S, config(tag))
        m.load_state_dict(weights(m, tag))
        m.eval()
        sd = m.state_dict()
        inventory[tag] = dict(rep_dim=int(m.rep_dim), params=[[k, list(v.shape)] for k, v in sd.items()])
        x = tokens(tag).requires_grad_(True)
        out = m(x)
        (out * cotangent(tag, out.shape)).sum().backward()
        fx[tag + ":out"] = out.detach().numpy()
        fx[tag + ":dtokens"] = sample(x.grad)
        for k, p in m.named_parameters():
            fx[tag + ":g:" + k] = p.grad.numpy() if p.numel() <= FULL_MAX else sample(p.grad)
        print(f"[{tag}] out {tuple(out.shape)} |out| {out.abs().max().item():.3e} |dtokens| {x.grad.abs().max().item():.3e}")
    fx["inventory"] = np.array(json.dumps(inventory))
    np.savez_compressed(FIXTURE, **fx)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
