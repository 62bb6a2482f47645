"""Generate tests/golden/gt.npz from the reference's own GT_Module (ocrs/gt/gt_module.py).

Runs ONLY where the reference checkout is present (import recipe as make_golden_naturecnn.py: wandb, h5py, omegaconf and utils.tools
stubbed).  Per case: num_slots, rep_dim and the state_dict keys (``inventory``), closed-form weights, a seeded state [3, K, 5], EVERY
layer's output (forward hooks on the container's members, so a ReLU's output is recorded where there is one) and the autograd gradients
of ``(out * cotangent).sum()``.  The helpers need neither the reference nor a GPU: the tests import them to rebuild the same inputs.

    python tests/golden/make_golden_gt.py
"""
import contextlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_pooling_heads import REF, closed_form, load_closed_form  # noqa: E402

# tag: (dims, acts, env name, num_objects_range)
CASES = {
    "identity": ([], [], "TargetN4C4S3S1Env", [4, 4]),
    "small": ([8, 12], ["relu", "relu"], "TargetN4C4S3S1Env", [2, 4]),
    "wide": ([64, 64, 128], ["relu", "relu", "none"], "TargetN4C4S3S1Env", [4, 4]),
    "wide_push": ([64, 64, 128], ["relu", "relu", "none"], "PushN3C4S1S1Env", [3, 3]),
    "short_acts": ([8, 12, 16], ["none", "relu"], "OddOneOutN4C2S2S1Env", [4, 4]),      # zip: the shorter list wins; rep_dim stays dims[-1]
}
FIXTURE = os.path.join(HERE, "gt.npz")


def configs(tag):
    dims, acts, name, rng = CASES[tag]
    return (types.SimpleNamespace(name="GT", dims=list(dims), acts=list(acts)),
            types.SimpleNamespace(name=name, num_objects_range=list(rng), state_size=5, obs_size=64, obs_channels=3))


def state(tag, num_slots):
    """[3, K, 5]: ids in the first two columns, a scale index in the third, positions in the last two, as a state observation has them"""
    g = torch.Generator().manual_seed(320 + list(CASES).index(tag))      # seeds at which every ReLU pre-activation is >= 1e-4 of its layer's largest
    ids = torch.stack([torch.randint(0, 7, (3, num_slots), generator=g), torch.randint(0, 4, (3, num_slots), generator=g),
                       torch.randint(0, 2, (3, num_slots), generator=g)], -1).float()
    return torch.cat([ids, torch.rand(3, num_slots, 2, generator=g)], -1)


def cotangent(tag, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(400 + list(CASES).index(tag)))


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
    from ocrs.gt.gt_module import GT_Module  # noqa
    return GT_Module


def main():
    GT_Module = import_reference()
    fx, inventory = {}, {}
    for tag in CASES:
        m = GT_Module(*configs(tag))
        load_closed_form(m)
        sd = m.state_dict()
        inventory[tag] = dict(num_slots=int(m.num_slots), rep_dim=int(m.rep_dim), params=[[k, list(v.shape)] for k, v in sd.items()],
                              members=[type(x).__name__ for x in m._net])
        for k, v in sd.items():
            fx[f"{tag}:w:{k}"] = v.numpy()
        s = state(tag, m.num_slots).requires_grad_(True)
        outs = []
        hooks = [x.register_forward_hook(lambda _m, _i, o: outs.append(o.detach())) for x in m._net]
        out = m(s)
        for h in hooks:
            h.remove()
        fx[f"{tag}:state"] = s.detach().numpy()
        fx[f"{tag}:out"] = out.detach().numpy()
        for i, o in enumerate(outs):                           # one per member of _net, in order
            fx[f"{tag}:member:{i}"] = o.numpy()
        if sd:
            cot = cotangent(tag, out.shape)
            (out * cot).sum().backward()
            fx[f"{tag}:dstate"] = s.grad.numpy()
            for k, p in m.named_parameters():
                fx[f"{tag}:g:{k}"] = p.grad.numpy()
        print(f"[{tag}] slots {m.num_slots} rep_dim {m.rep_dim} keys {list(sd)} out {tuple(out.shape)}")
    fx["inventory"] = np.array(json.dumps(inventory))
    np.savez_compressed(FIXTURE, **fx)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
