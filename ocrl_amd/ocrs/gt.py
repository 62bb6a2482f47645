"""Ground-truth-state "encoder" (ocrs/gt/gt.py:11-14, gt_module.py:6-37): the environment's state rows [B, hi + 1, 5] stand in for the
slots, optionally through a per-object MLP.  It is the upper bound the object-centric encoders are read against.

``GT_Module`` holds the parameters in the reference's container (``_net``: nn.Sequential of nn.Linear, with an ``nn.Identity`` in each
ReLU's place so that the ``_net.{i}`` state_dict keys are the reference's); the container's ``forward`` is never called.  With
``dims: []`` the module is the identity and launches nothing.  Otherwise the arithmetic is ``ocrl_gt_mlp_fwd/_bwd`` (HIP: one launch
forward with the ReLUs fused, at most two backward), wrapped in a ``torch.autograd.Function``.  No CPU fallback: a CPU tensor raises."""
import torch
from torch import nn

from .. import _bridge, _lib
from .base import Base

_WHO = "ocrl_amd.ocrs.GT"


class _GTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dims, acts, *params):
        shapes = [sh for l, d in enumerate(dims) for sh in ((d, dims[l - 1] if l else x.shape[-1]), (d,))]
        x, ps = _bridge.inputs(_WHO, x, params, shapes)
        L, dev = _lib.lib(), x.device
        D = x.shape[-1]
        M = x.numel() // D if D else 0
        geom = (len(dims), _bridge.ints(dims))
        ws = _bridge.workspace(_WHO, L.ocrl_gt_mlp_ws_floats(M, D, *geom), dev, f"{M} rows of width {D}, dims {list(dims)}")
        out = torch.empty(*x.shape[:-1], dims[-1], device=dev, dtype=torch.float32)
        args = (M, D, *geom, _bridge.ints(acts), _lib.ptr(ws), ws.numel())
        _bridge.launch(dev, L.ocrl_gt_mlp_fwd, _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(out), *args)
        ctx.save_for_backward(x, *ps)
        ctx.args, ctx.ws = args, ws
        return out

    @staticmethod
    def backward(ctx, dout):
        x, *ps = ctx.saved_tensors
        dout = _bridge.cotangent(dout)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(x.device, _lib.lib().ocrl_gt_mlp_bwd, _lib.ptr(x), _lib.ptr(dout), _lib.ptrs(ps), _lib.ptr(dx), _lib.ptrs(gs), *ctx.args)
        return (dx, None, None, *gs)


def gt_mlp(x, params, acts):
    """x [..., D] through the layers params = [W_0, b_0, W_1, b_1, ..] (torch Linear layout), a ReLU after layer l when acts[l] is
    "relu" (or a non-zero int)"""
    dims = tuple(int(w.shape[0]) for w in params[0::2])
    return _GTFn.apply(x, dims, tuple(int(a == "relu" if isinstance(a, str) else bool(a)) for a in acts), *params)


class GT_Module(nn.Module):
    trains_through_autograd = True                             # OCRExtractor: the RL loss reaches the parameters through torch autograd

    def __init__(self, ocr_config, env_config) -> None:
        super().__init__()
        extra = 2 if ("Push" in env_config.name) or ("Maze" in env_config.name) else 1
        self.num_slots = env_config.num_objects_range[1] + extra
        self.rep_dim = env_config.state_size
        net, acts, in_dim = [], [], self.rep_dim
        for dim, act in zip(ocr_config.dims, ocr_config.acts):
            net.append(nn.Linear(in_dim, dim))
            if act == "relu":
                net.append(nn.Identity())                      # the ReLU's index; the activation itself is fused into the kernel
            acts.append(act)
            in_dim = dim
        self._net = nn.Sequential(*net)
        self._acts = tuple(acts)
        if len(ocr_config.dims) > 0:
            self.rep_dim = ocr_config.dims[-1]

    def _param_list(self):
        return [p for m in self._net if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]

    def forward(self, obs):
        ps = self._param_list()
        return gt_mlp(obs, ps, self._acts) if ps else obs

    def get_loss(self, obs, with_rep=False):
        return ({}, self(obs)) if with_rep else {}

    def get_samples(self, obs) -> dict:
        return {}


class GT(Base):
    def __init__(self, ocr_config, env_config) -> None:
        self._module = GT_Module(ocr_config, env_config)
        super().__init__(ocr_config, env_config)
