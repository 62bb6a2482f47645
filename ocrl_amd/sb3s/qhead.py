"""What DQN's five heads (dqn.py's QNetwork, c51.py's CategoricalQNetwork, qr.py's QuantileQNetwork, iqn.py's ImplicitQuantileQNetwork and
fqf.py's FullyParameterizedQuantileQNetwork) and their fused loss steps share: the stack of hidden layers under ``q_net``, the launch
every head's ``act`` ends on, the coercion of a step's per-row inputs and the backward of a step whose forward already wrote the
gradients."""
import ctypes

import torch
from torch import nn

from .. import _bridge, _lib
from .noisy import effective_params, linear

_WHO = "ocrl_amd.sb3s"
_ACT = {"relu": (nn.ReLU, 1), "tanh": (nn.Tanh, 2)}
DQN_SCALARS = ("loss", "mean_q", "mean_target")


class QHead(nn.Module):
    """len(net_arch) x [Linear, activation] -> Linear(last, n_out) in ``q_net``, an nn.Sequential whose ``state_dict()`` keys are
    ``q_net.{2i}.weight|bias``; the container's ``forward`` is never called.  ``noisy``: every Linear is a NoisyLinear (sigmas start at
    ``noisy_sigma0 / sqrt(in)``) and the kernels receive the effective parameters of the draw ``_noise`` = (seed, draw) names
    (DQNPolicy.set_noise; None: the means).  ``latent_dim`` is the width the output Linear reads."""
    _noise = None

    def __init__(self, features_dim, n_out, net_arch, activation, noisy, noisy_sigma0):
        super().__init__()
        if activation not in _ACT:
            raise ValueError(f"{_WHO}.{type(self).__name__}: activation {activation!r} is not one of {', '.join(_ACT)}")
        self._dims, self._act = tuple(int(w) for w in net_arch), _ACT[activation][1]
        self.noisy, self.noisy_sigma0 = bool(noisy), float(noisy_sigma0)
        layers, in_dim = [], int(features_dim)
        for w in self._dims:
            layers += [self._linear(in_dim, w), _ACT[activation][0]()]
            in_dim = w
        self.latent_dim = in_dim
        self.q_net = nn.Sequential(*layers, self._linear(in_dim, n_out))

    def _linear(self, in_dim, out_dim):
        return linear(in_dim, out_dim, self.noisy, self.noisy_sigma0)

    def _layout(self):
        """(hidden widths, activation codes), as the C ABI takes them"""
        return self._dims, (self._act,) * len(self._dims)

    def _param_list(self, *more):
        """(weight, bias) per Linear of ``q_net``, then of ``more``, as the kernels take them; with ``noisy`` the effective tensors of
        the current draw"""
        return effective_params([m for m in self.q_net if isinstance(m, nn.Linear)] + list(more), self._noise if self.noisy else None)

    def _launch_act(self, fn, d, x, ps, seed, row_offset, epsilon, uniforms, before=(), after=()):
        """what every head's ``act`` ends on: (actions int64 [B], q [B, n_actions]) of the launch fn(desc, x, params, *before, seed,
        row_offset, epsilon, uniforms, *after, actions, q).  ``before`` is what an entry takes ahead of the stream (C51's support, FQF's
        boundaries), ``after`` behind it (IQN's fractions)"""
        actions = torch.empty(x.shape[0], device=x.device, dtype=torch.int64)
        q = torch.empty(x.shape[0], self.n_actions, device=x.device)
        _bridge.launch(x.device, fn, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), *before, int(seed), int(row_offset), float(epsilon),
                       _lib.ptr(uniforms), *after, _lib.ptr(actions), _lib.ptr(q))
        return actions, q


def coerce(who, dev, what, *named):
    """the per-row inputs of a fused step.  named = (name, tensor or None, dtype, entries) each: a given tensor comes back detached, on
    ``dev``, of that dtype, flat and contiguous; one whose count is not ``entries`` raises a ValueError that names it and ``what``"""
    out = []
    for name, t, dt, n in named:
        if t is not None:
            t = (t.detach() if t.requires_grad else t).to(device=dev, dtype=dt).reshape(-1).contiguous()
            if t.numel() != n:
                raise ValueError(f"{who}: {name} has {t.numel()} entries for {what}")
        out.append(t)
    return out


def scaled_grads(ctx, gloss, n_other):
    """the backward of a fused step whose forward left the loss's gradients in ``ctx.dx`` (features) and ``ctx.gs`` (parameters):
    they are scaled by the loss's cotangent; the ``n_other`` inputs between the features and the parameters get none"""
    dx = None if ctx.dx is None else ctx.dx * gloss
    return (dx,) + (None,) * n_other + tuple(g * gloss for g in ctx.gs)
