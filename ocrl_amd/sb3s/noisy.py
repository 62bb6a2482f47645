"""DQN's noisy linear layers (NoisyNet, Fortunato et al. 2018, with factorised Gaussian noise): the sixth component of Rainbow (Hessel et
al. 2018), where learned parameter noise replaces the epsilon-greedy coin.  Restated from the published algorithm; the GPU work is the
library's (include/ocrl_hip_noisy.h, which states every formula).  A ``NoisyLinear`` holds ``weight`` / ``bias`` (the means) and
``weight_sigma`` / ``bias_sigma`` (the noise scales); the heads of dqn.py and c51.py never call it: ``effective_params`` writes the
perturbed tensors of one draw (``ocrl_noisy_factors`` + ``ocrl_noisy_perturb``) and the unchanged head kernels receive them in place of the
parameters.  ``DQN(noisy=True)`` uses them (dqn.py; ``sb3=rainbow``)."""
import ctypes
import math

import torch
from torch import nn

from .. import _bridge, _lib

_WHO = "ocrl_amd.sb3s"


class NoisyLinear(nn.Linear):
    """nn.Linear whose effective parameters of a draw are weight + weight_sigma * (f_out f_in^T) and bias + bias_sigma * f_out.
    ``weight`` and ``bias`` keep nn.Linear's initialisation, U(-1/sqrt(in), 1/sqrt(in)), which is the paper's for factorised noise; every
    sigma starts at ``sigma0 / sqrt(in)``.  state_dict order: weight, bias, weight_sigma, bias_sigma.  ``forward`` is nn.Linear's on the
    means: the noise lives in the head that owns the layer (``effective_params``)."""

    def __init__(self, in_features, out_features, sigma0=0.5):
        super().__init__(in_features, out_features)
        self.sigma0 = float(sigma0)
        s = self.sigma0 / math.sqrt(in_features)
        self.weight_sigma = nn.Parameter(torch.full((out_features, in_features), s))
        self.bias_sigma = nn.Parameter(torch.full((out_features,), s))

    def extra_repr(self):
        return f"{super().extra_repr()}, sigma0={self.sigma0}"


def linear(in_features, out_features, noisy=False, sigma0=0.5):
    """the Linear of a head: a NoisyLinear with ``noisy``"""
    return NoisyLinear(in_features, out_features, sigma0) if noisy else nn.Linear(in_features, out_features)


def draw_factors(layers, seed, draw, dev, eps=None):
    """(descriptor, factors) of draw ``draw`` of stream ``seed`` for ``layers`` = (in, out) per layer: one ``ocrl_noisy_factors`` launch.
    ``eps`` (the layout of ``factors``) replaces the Gaussians."""
    d = _lib.noisy_desc(layers)
    n = _lib.lib().ocrl_noisy_factor_floats(ctypes.byref(d))
    if n == 0:
        raise ValueError(f"{_WHO}: noisy layers {list(layers)} not supported: " + _lib.lib().ocrl_last_error().decode())
    factors = torch.empty(n, device=dev, dtype=torch.float32)
    if eps is not None:
        eps = eps.to(device=dev, dtype=torch.float32).contiguous()
        if eps.numel() != n:
            raise ValueError(f"{_WHO}: eps has {eps.numel()} entries, the factors of layers {list(layers)} {n}")
    _bridge.launch(dev, _lib.lib().ocrl_noisy_factors, ctypes.byref(d), int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1), _lib.ptr(eps),
                   _lib.ptr(factors))
    return d, factors


class _NoisyFn(torch.autograd.Function):
    """(weight, bias per layer) of one draw from the means and the noise scales, in fresh tensors.  backward: the gradient of a mean is
    the incoming gradient itself, the gradient of a sigma ``ocrl_noisy_grad`` of it."""

    @staticmethod
    def forward(ctx, seed, draw, *params):
        n = len(params) // 2
        mu, sigma = list(params[:n]), list(params[n:])
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or p.device != params[0].device:
                raise RuntimeError(f"{_WHO}: noisy layers run on the GPU in float32 (there is no CPU fallback; got {p.dtype} on {p.device})")
        dev = params[0].device
        mu, sigma = [p.detach().contiguous() for p in mu], [p.detach().contiguous() for p in sigma]
        layers = [(w.shape[1], w.shape[0]) for w in mu[0::2]]
        d, factors = draw_factors(layers, seed, draw, dev)
        w_eff = [torch.empty_like(p) for p in mu]
        _bridge.launch(dev, _lib.lib().ocrl_noisy_perturb, ctypes.byref(d), _lib.ptrs(mu), _lib.ptrs(sigma), _lib.ptr(factors), _lib.ptrs(w_eff))
        ctx.d, ctx.factors = d, factors                       # private to the node: nothing else holds them
        ctx.shapes = [tuple(p.shape) for p in mu]
        return tuple(w_eff)

    @staticmethod
    def backward(ctx, *gs):
        dev = ctx.factors.device
        dsigma = None
        if any(ctx.needs_input_grad[2 + len(gs):]):
            gs = tuple(_bridge.cotangent(g) for g in gs)
            dw = [g if g is not None else torch.zeros(s, device=dev) for g, s in zip(gs, ctx.shapes)]
            dsigma = [torch.empty_like(g) for g in dw]
            _bridge.launch(dev, _lib.lib().ocrl_noisy_grad, ctypes.byref(ctx.d), _lib.ptrs(dw), _lib.ptr(ctx.factors), _lib.ptrs(dsigma))
        return (None, None, *gs, *(dsigma or (None,) * len(gs)))


def effective_params(mods, noise):
    """The parameter list a head hands to its kernels: (weight, bias) per Linear of ``mods``.  ``noise`` None: the means themselves,
    nothing is launched.  ``noise`` = (seed, draw): the perturbed tensors of that draw, attached to autograd; every call regenerates them."""
    mu = [p for m in mods for p in (m.weight, m.bias)]
    if noise is None:
        return mu
    sigma = [p for m in mods for p in (m.weight_sigma, m.bias_sigma)]
    return list(_NoisyFn.apply(int(noise[0]), int(noise[1]), *mu, *sigma))


__all__ = ["NoisyLinear"]
