"""Relation Network pooling (poolings/rn/rn.py:6-9, rn_module.py:8-59): an MLP g on every ordered pair of slots, summed over the pairs,
then an MLP f.

``RN_Module`` holds the parameters in the reference's containers (``_g`` / ``_f``: nn.Sequential of [nn.Linear, nn.ReLU] pairs), so
``state_dict()`` keys, shapes and initialisation are the reference's and its checkpoints load unchanged; the containers' ``forward`` is
never called.  The arithmetic is ``ocrl_pool_rn_fwd/_bwd`` (HIP: the first g layer factored over the slots, the pairs expanded by an
addition), wrapped in a ``torch.autograd.Function``.  No CPU fallback: a CPU tensor raises."""
import torch
from torch import nn

from .. import _bridge, _lib
from .base import Base

_WHO = "ocrl_amd.poolings.RN"


class _RNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, slots, g_dims, f_dims, *params):
        slots, ps = _bridge.inputs(_WHO, slots, params)
        L, dev = _lib.lib(), slots.device
        B, K, D = slots.shape
        dims = (len(g_dims), _bridge.ints(g_dims), len(f_dims), _bridge.ints(f_dims))
        ws = _bridge.workspace(_WHO, L.ocrl_pool_rn_ws_floats(B, K, D, *dims), dev,
                               f"batch {B}, {K} slots of width {D}, g_dims {list(g_dims)}, f_dims {list(f_dims)}")
        out = torch.empty(B, f_dims[-1], device=dev, dtype=torch.float32)
        _bridge.launch(dev, L.ocrl_pool_rn_fwd, _lib.ptr(slots), _lib.ptrs(ps), _lib.ptr(out), B, K, D, *dims, _lib.ptr(ws), ws.numel())
        ctx.save_for_backward(slots, *ps)
        ctx.dims, ctx.ws = dims, ws
        return out

    @staticmethod
    def backward(ctx, dout):
        slots, *ps = ctx.saved_tensors
        B, K, D = slots.shape
        dout = _bridge.cotangent(dout)
        gs = [torch.empty_like(p) for p in ps]
        ds = torch.empty_like(slots) if ctx.needs_input_grad[0] else None
        _bridge.launch(slots.device, _lib.lib().ocrl_pool_rn_bwd, _lib.ptr(slots), _lib.ptr(dout), _lib.ptrs(ps), _lib.ptr(ds), _lib.ptrs(gs),
                       B, K, D, *ctx.dims, _lib.ptr(ctx.ws), ctx.ws.numel())
        return (ds, None, None, *gs)


def _linear_relu(in_dim, dims):
    """nn.Sequential([nn.Linear, nn.ReLU] x len(dims)) with the reference's indices (rn_module.py:17-31)"""
    layers = []
    for d in dims:
        layers += [nn.Linear(in_dim, d), nn.ReLU()]
        in_dim = d
    return nn.Sequential(*layers)


class RN_Module(nn.Module):
    def __init__(self, ocr_rep_dim: int, ocr_num_slots: int, num_stacked_obss: int, config) -> None:
        super().__init__()
        if num_stacked_obss != 1:                            # rn_module.py:11
            raise NotImplementedError(f"RN pooling takes one observation (num_stacked_obss = 1, got {num_stacked_obss})")
        if ocr_num_slots < 2:                                # no pairs (the reference fails on K = 1 with an AttributeError)
            raise ValueError(f"RN pooling needs at least 2 slots (got {ocr_num_slots})")
        self.rep_dim = config.f_dims[-1]
        self._g_dims = tuple(int(d) for d in config.g_dims)
        self._f_dims = tuple(int(d) for d in config.f_dims)
        self._g = _linear_relu(ocr_rep_dim * 2, self._g_dims)
        self._f = _linear_relu(self._g_dims[-1], self._f_dims)

    def _param_list(self):
        return [p for seq in (self._g, self._f) for m in seq if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]

    def forward(self, state):
        return _RNFn.apply(state, self._g_dims, self._f_dims, *self._param_list())


class RN(Base):
    """the reference's argument order (poolings/rn/rn.py:6): (ocr, num_stacked_obss, config)"""

    def __init__(self, ocr, num_stacked_obss: int, config) -> None:
        self._module = RN_Module(ocr.rep_dim, ocr.num_slots, num_stacked_obss, config)
        super().__init__(ocr, config)
