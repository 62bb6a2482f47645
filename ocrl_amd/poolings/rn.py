"""Relation Network pooling (poolings/rn/rn.py:6-9, rn_module.py:8-59): an MLP g on every ordered pair of slots, summed over the pairs,
then an MLP f.

``RN_Module`` holds the parameters in the reference's containers (``_g`` / ``_f``: nn.Sequential of [nn.Linear, nn.ReLU] pairs), so
``state_dict()`` keys, shapes and initialisation are the reference's and its checkpoints load unchanged; the containers' ``forward`` is
never called.  The arithmetic is ``ocrl_pool_rn_fwd/_bwd`` (HIP: the first g layer factored over the slots, the pairs expanded by an
addition), wrapped in a ``torch.autograd.Function``.  No CPU fallback: a CPU tensor raises."""
import ctypes

import torch
from torch import nn

from .. import _lib
from .base import Base


def _int_array(v):
    return (ctypes.c_int * len(v))(*v)


class _RNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, slots, g_dims, f_dims, *params):
        if not slots.is_cuda:
            raise RuntimeError("ocrl_amd.poolings: tensors must live on the GPU (there is no CPU fallback)")
        L = _lib.lib()
        B, K, D = slots.shape
        slots = slots.contiguous().float()
        ps = [p.detach().contiguous() for p in params]
        gd, fd = _int_array(g_dims), _int_array(f_dims)
        n = L.ocrl_pool_rn_ws_floats(B, K, D, len(g_dims), gd, len(f_dims), fd)
        if n == 0:
            raise ValueError(f"ocrl_amd.poolings.RN: shape not supported: batch {B}, {K} slots of width {D}, g_dims {list(g_dims)}, "
                             f"f_dims {list(f_dims)} (needs >= 2 slots, widths that are multiples of 4, and batch * K * (K - 1) pair rows "
                             f"times the widest g layer below 2^31)")
        ws = torch.empty(n, device=slots.device, dtype=torch.float32)
        out = torch.empty(B, f_dims[-1], device=slots.device, dtype=torch.float32)
        arr = _lib.ptrs(ps)
        st = _lib.stream()
        _lib.check(L.ocrl_pool_rn_fwd(_lib.ptr(slots), arr, _lib.ptr(out), B, K, D, len(g_dims), gd, len(f_dims), fd, _lib.ptr(ws), n, st))
        ctx.dims, ctx.ws, ctx.ps, ctx.slots = (g_dims, f_dims), ws, ps, slots
        ctx.need_dslots = ctx.needs_input_grad[0]      # read from the autograd node: the converted copy above carries no requires_grad
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _lib.lib()
        g_dims, f_dims = ctx.dims
        B, K, D = ctx.slots.shape
        dout = dout.contiguous().float()
        gs = [torch.empty_like(p) for p in ctx.ps]
        ds = torch.empty_like(ctx.slots) if ctx.need_dslots else None
        arr = _lib.ptrs(ctx.ps)
        garr = _lib.ptrs(gs)
        st = _lib.stream()
        _lib.check(L.ocrl_pool_rn_bwd(_lib.ptr(ctx.slots), _lib.ptr(dout), arr, _lib.ptr(ds), garr, B, K, D, len(g_dims), _int_array(g_dims),
                                      len(f_dims), _int_array(f_dims), _lib.ptr(ctx.ws), ctx.ws.numel(), st))
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
        if state.shape[1] < 2:
            raise ValueError(f"RN pooling needs at least 2 slots (got {state.shape[1]})")
        return _RNFn.apply(state, self._g_dims, self._f_dims, *self._param_list())


class RN(Base):
    """the reference's argument order (poolings/rn/rn.py:6): (ocr, num_stacked_obss, config)"""

    def __init__(self, ocr, num_stacked_obss: int, config) -> None:
        self._module = RN_Module(ocr.rep_dim, ocr.num_slots, num_stacked_obss, config)
        super().__init__(ocr, config)
