"""CNN_Linear pooling (poolings/cnn_linear/cnn_linear.py, cnn_linear_module.py:7-14, poolings/common/naturecnn.py:10-29): NatureCNN over
``slot_to_img(rep)`` (utils/tools.py:33-36), the head behind SLATE with ``use_cnn_feat`` ("SLATE-CNN").

``_NatureCNN`` holds real ``nn.Conv2d`` / ``nn.Linear`` layers at the reference's ``Sequential`` indices (the ReLU slots are
``nn.Identity``, as in ocrs/naturecnn.py), so ``state_dict()`` keys, shapes and default initialisation are the reference's, reference
checkpoints load unchanged, and SB3's ``ortho_init`` finds the layers.  The containers' ``forward`` is never called: the arithmetic is
``ocrl_pool_cnn_fwd/_bwd`` wrapped in one ``torch.autograd.Function``.  ``slot_to_img`` is a view here: the ``[B, N, D]`` token map
already is the channels-last image the first convolution reads, so nothing is permuted or copied.  The tokens get a gradient when they
require one.  No CPU fallback: a CPU tensor raises."""
import math

import torch
from torch import nn

from .. import _bridge, _lib
from .._bridge import NATURE_CONVS, conv_map_size, conv_shapes
from .base import Base

_WHO = "ocrl_amd.poolings.CNN"
_FLAT = 1024                                                     # the reference's Linear(1024, rep_dim): a 64 x 64 map


class _NatureCNN(nn.Module):
    """parameter container of poolings/common/naturecnn.py:10-29 (its own class: the Linear sits inside ``_net`` at index 7)"""

    def __init__(self, in_dim, rep_dim, use_cnn_feat):
        super().__init__()
        net, c = [], in_dim
        for cout, k, s in NATURE_CONVS[:3]:            # _net.0 / .2 / .4
            net += [nn.Conv2d(c, cout, kernel_size=k, stride=s, padding=0), nn.Identity()]
            c = cout
        if not use_cnn_feat:
            net += [nn.Flatten(), nn.Linear(_FLAT, rep_dim), nn.Identity()]
        self._net = nn.Sequential(*net)
        self.in_dim = in_dim
        self.rep_dim = 0 if use_cnn_feat else int(rep_dim)

    def param_list(self):
        return [p for m in self._net if isinstance(m, (nn.Conv2d, nn.Linear)) for p in (m.weight, m.bias)]


def _check_inputs(tokens, params, in_dim, rep):
    """what the C entry points cannot check: they get no parameter sizes and derive the Linear's input width from the map's side.
    Returns (tokens, parameters) as the kernels read them, and the map's side"""
    if tokens.dim() != 3 or tokens.shape[2] != in_dim:
        raise ValueError(f"{_WHO}: expected tokens [B, N, {in_dim}], got {list(tokens.shape)}")
    side = math.isqrt(tokens.shape[1])
    if side * side != tokens.shape[1]:
        raise ValueError(f"{_WHO}: slot_to_img needs a square token map, got N = {tokens.shape[1]}")
    o = conv_map_size(side)
    if rep and 64 * o * o != _FLAT:
        raise ValueError(f"ocrl_amd.poolings.CNN_Linear: a {side} x {side} token map flattens to 64 x {o} x {o} = {64 * o * o} features, "
                         f"but the Linear takes {_FLAT} (a 64 x 64 map)")
    return (*_bridge.inputs(_WHO, tokens, params, conv_shapes(in_dim) + ([(rep, _FLAT), (rep,)] if rep else [])), side)


def _run(tokens, side, rep, params, save):
    """one ocrl_pool_cnn_fwd call; returns (out, ws)"""
    L, dev = _lib.lib(), tokens.device
    B, _, D = tokens.shape
    ws = _bridge.workspace(_WHO, L.ocrl_pool_cnn_ws_floats(B, side, side, D, rep), dev,
                           f"batch {B} of {side} x {side} x {D} token maps, rep_dim {rep}")
    o = conv_map_size(side)
    out = torch.empty((B, rep) if rep else (B, o * o, 64), device=dev, dtype=torch.float32)
    _bridge.launch(dev, L.ocrl_pool_cnn_fwd, _lib.ptr(tokens), _lib.ptrs(params), _lib.ptr(out), B, side, side, D, rep, int(save), _lib.ptr(ws),
                   ws.numel())
    return out, ws


class _PoolCnnFn(torch.autograd.Function):
    """over the tokens and the parameters `ps` as _check_inputs returned them; `params` are their attached originals, which get the
    gradients"""

    @staticmethod
    def forward(ctx, tokens, side, rep, ps, *params):
        out, ws = _run(tokens, side, rep, ps, save=True)
        ctx.save_for_backward(tokens, *ps)
        ctx.side, ctx.rep, ctx.ws = side, rep, ws
        return out

    @staticmethod
    def backward(ctx, dout):
        tokens, *ps = ctx.saved_tensors
        B, _, D = tokens.shape
        dout = _bridge.cotangent(dout)
        gs = [torch.empty_like(p) for p in ps]
        dt = torch.empty_like(tokens) if ctx.needs_input_grad[0] else None
        _bridge.launch(tokens.device, _lib.lib().ocrl_pool_cnn_bwd, _lib.ptr(tokens), _lib.ptr(dout), _lib.ptrs(ps), _lib.ptr(dt), _lib.ptrs(gs),
                       B, ctx.side, ctx.side, D, ctx.rep, _lib.ptr(ctx.ws), ctx.ws.numel())
        return (dt, None, None, None, *gs)


def run_pool_cnn(tokens, net):
    """NatureCNN over slot_to_img(tokens): an autograd node that keeps the activations when anything needs a gradient, a bare call
    otherwise (a no_grad rollout keeps nothing)"""
    params = net.param_list()
    x, ps, side = _check_inputs(tokens, params, net.in_dim, net.rep_dim)
    if torch.is_grad_enabled() and (tokens.requires_grad or any(p.requires_grad for p in params)):
        return _PoolCnnFn.apply(x, side, net.rep_dim, ps, *params)
    return _run(x, side, net.rep_dim, ps, save=False)[0]


class CNN_Linear_Module(nn.Module):
    def __init__(self, ocr_rep_dim: int, ocr_num_slots: int, config, num_stacked_obss: int = 1) -> None:
        super().__init__()
        self.rep_dim = rep_dim = config.rep_dim
        self._net = _NatureCNN(ocr_rep_dim * num_stacked_obss, rep_dim, use_cnn_feat=False)

    def forward(self, state):
        return run_pool_cnn(state, self._net)


class CNN_Linear(Base):
    def __init__(self, ocr, config, num_stacked_obss: int = 1) -> None:
        self._module = CNN_Linear_Module(ocr.rep_dim, ocr.num_slots, config, num_stacked_obss)
        super().__init__(ocr, config)
