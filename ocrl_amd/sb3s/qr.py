"""DQN's quantile head: the return distribution of QR-DQN (Dabney, Rowland, Bellemare and Munos 2018) as ``n_quantiles`` quantile values
per action at the fixed fractions tau_i = (i + 0.5) / N, with no support to set, optionally with the dueling aggregation (Wang et al.
2016) applied per quantile.  Restated from the published algorithm; the GPU work is the library's (include/ocrl_hip_qr.h, which states
every formula): ``QuantileQNetwork.quantile_values`` is ``ocrl_qr_fwd`` / ``ocrl_qr_bwd`` under a ``torch.autograd.Function``,
``quantiles`` one ``ocrl_qr_fwd`` launch, acting ``ocrl_qr_act`` and the loss ``qr_loss`` (``ocrl_qr_td_fwd_bwd``: the quantile Huber loss
against the Bellman-shifted quantiles of the bootstrap action and the head's gradient, fused).  ``DQN(n_quantiles=50)`` uses them
(dqn.py; ``sb3=qrdqn``)."""
import ctypes

import torch

from .. import _bridge, _lib
from .qhead import DQN_SCALARS, QHead, coerce, scaled_grads

_WHO = "ocrl_amd.sb3s"
MAX_QUANTILES, MAX_QUANTILE_COLS = 64, 256   # quantiles per action, n_actions * n_quantiles (include/ocrl_hip_qr.h)


def _desc(B, F, A, N, dims, acts, dueling, dev, keep=True):
    """(descriptor, workspace) of a call"""
    d = _lib.qr_desc(B, F, A, N, dims, acts, dueling)
    return d, _bridge.workspace(_WHO, _lib.lib().ocrl_qr_ws_floats(ctypes.byref(d)), dev,
                                f"batch {B}, feature_dim {F}, {A} actions of {N} quantiles, hidden widths {list(dims)}", keep)


class _QrFn(torch.autograd.Function):
    """quantile values [B, A, N] of a feature batch"""

    @staticmethod
    def forward(ctx, features, head, *params):
        A, N, dims, acts, dueling = head
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        need_grad = any(ctx.needs_input_grad)
        d, ws = _desc(B, F, A, N, dims, acts, dueling, dev, need_grad)
        theta = torch.empty(B, A, N, device=dev)
        _bridge.launch(dev, _lib.lib().ocrl_qr_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(theta), None, int(need_grad),
                       _lib.ptr(ws) if need_grad else None, ws.numel())
        ctx.save_for_backward(x, *ps)
        ctx.d, ctx.ws = d, ws
        return theta

    @staticmethod
    def backward(ctx, dtheta):
        x, *ps = ctx.saved_tensors
        dtheta = _bridge.cotangent(dtheta)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(x.device, _lib.lib().ocrl_qr_bwd, ctypes.byref(ctx.d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(dtheta), _lib.ptr(dx),
                       _lib.ptrs(gs), _lib.ptr(ctx.ws), ctx.ws.numel())
        return (dx, None, *gs)


class _QrTdFn(torch.autograd.Function):
    """the fused TD step: (loss, scalars [3], row_loss [B]); the gradients are the forward's own outputs"""

    @staticmethod
    def forward(ctx, features, next_quantiles, next_q, actions, rewards, dones, discounts, weights, gamma, kappa, head, *params):
        A, N, dims, acts, dueling = head
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        f32 = torch.float32
        actions, rewards, dones, next_quantiles, next_q, discounts, weights = coerce(
            f"{_WHO}.qr_loss", dev, f"a batch of {B}, {A} actions and {N} quantiles", ("actions", actions, torch.int64, B),
            ("rewards", rewards, f32, B), ("dones", dones, torch.uint8, B), ("next_quantiles", next_quantiles, f32, B * A * N),
            ("next_q", next_q, f32, B * A), ("discounts", discounts, f32, B), ("weights", weights, f32, B))
        d, ws = _desc(B, F, A, N, dims, acts, dueling, dev)
        scal = torch.empty(3, device=dev, dtype=torch.float32)
        row_loss = torch.empty(B, device=dev, dtype=torch.float32)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(dev, _lib.lib().ocrl_qr_td_fwd_bwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(next_quantiles), _lib.ptr(next_q),
                       _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones), _lib.ptr(discounts), _lib.ptr(weights), float(gamma), float(kappa),
                       _lib.ptr(scal), _lib.ptr(row_loss), _lib.ptr(dx), _lib.ptrs(gs), _lib.ptr(ws), ws.numel())
        ctx.gs, ctx.dx = gs, dx
        ctx.mark_non_differentiable(scal, row_loss)
        return scal[0].clone(), scal, row_loss

    @staticmethod
    def backward(ctx, gloss, _gscal, _grow):
        return scaled_grads(ctx, gloss, 10)


class QuantileQNetwork(QHead):
    """features [B, F] -> len(net_arch) x [Linear, activation] -> Linear(last, n_actions * n_quantiles), quantile i of action a in
    column a * n_quantiles + i; with ``dueling`` a second Linear(last, n_quantiles), ``value_net``, on the same latent:
    theta[a, i] = V[i] + Adv[a, i] - mean_a' Adv[a', i].  The parameters sit in ``q_net``, an nn.Sequential with QNetwork's keys
    (``q_net.{2i}.weight|bias``; QHead), and in ``value_net``; neither container's ``forward`` is called.  ``n_actions`` and
    ``n_quantiles`` are attributes; ``taus`` [n_quantiles] = (i + 0.5) / n_quantiles.  ``noisy``: every Linear, the advantage and the
    value layer included, is a NoisyLinear, as CategoricalQNetwork's.  No CPU fallback: a CPU tensor raises."""

    def __init__(self, features_dim, n_actions, n_quantiles, net_arch=(64, 64), activation="relu", dueling=False, noisy=False,
                 noisy_sigma0=0.5):
        super().__init__(features_dim, int(n_actions) * int(n_quantiles), net_arch, activation, noisy, noisy_sigma0)
        self.n_actions, self.n_quantiles, self.dueling = int(n_actions), int(n_quantiles), bool(dueling)
        if self.n_quantiles < 1:
            raise ValueError(f"{_WHO}.QuantileQNetwork: n_quantiles >= 1 (got {n_quantiles})")
        if self.dueling:
            self.value_net = self._linear(self.latent_dim, self.n_quantiles)
        self.register_buffer("taus", (torch.arange(self.n_quantiles, dtype=torch.float32) + 0.5) / self.n_quantiles, persistent=False)

    def _head(self):
        """what the autograd functions need of the head besides its parameters"""
        return (self.n_actions, self.n_quantiles, *self._layout(), self.dueling)

    def _param_list(self):
        """QHead's list with the value Linear's pair at its end"""
        return super()._param_list(*([self.value_net] if self.dueling else []))

    def quantile_values(self, features):
        """theta [B, n_actions, n_quantiles], attached to autograd"""
        return _QrFn.apply(features, self._head(), *self._param_list())

    def forward(self, features):
        """q [B, n_actions]: the mean of ``quantile_values`` over the quantiles, attached to autograd; under ``torch.no_grad()`` the
        kernel's own q (``quantiles``)"""
        if not torch.is_grad_enabled():
            return self.quantiles(features)[1]
        return self.quantile_values(features).mean(-1)

    def quantiles(self, features):
        """(theta [B, n_actions, n_quantiles], q [B, n_actions]) in one launch, detached: what a target network is asked for"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        B, F = x.shape
        d, _ = _desc(B, F, self.n_actions, self.n_quantiles, *self._layout(), self.dueling, x.device, keep=False)
        theta = torch.empty(B, self.n_actions, self.n_quantiles, device=x.device)
        q = torch.empty(B, self.n_actions, device=x.device)
        _bridge.launch(x.device, _lib.lib().ocrl_qr_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(theta), _lib.ptr(q), 0, None, 0)
        return theta, q

    def act(self, features, seed, row_offset, epsilon, uniforms):
        """(actions int64 [B], q [B, n_actions]) of ``ocrl_qr_act``: DQNPolicy.act's launch for this head"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        B, F = x.shape
        d, _ = _desc(B, F, self.n_actions, self.n_quantiles, *self._layout(), self.dueling, x.device, keep=False)
        return self._launch_act(_lib.lib().ocrl_qr_act, d, x, ps, seed, row_offset, epsilon, uniforms)


def qr_loss(policy, features, next_quantiles, next_q, actions, rewards, dones, gamma, kappa=1.0, discounts=None, weights=None):
    """The quantile Huber loss of ``policy`` (a DQNPolicy with a QuantileQNetwork) on a feature batch [B, F] against the quantiles of the
    next observations: (loss, metrics, row_loss).  ``next_quantiles`` [B, n, N] is the target network's, ``next_q`` [B, n] names the
    bootstrap action (the target network's, or the online network's for double Q-learning); ``kappa`` is the Huber threshold,
    ``discounts`` [B] replaces ``gamma`` per row, ``weights`` [B] scales each row's loss and gradient.  ``loss`` is the mean over the rows
    of the quantile Huber loss between the quantiles of the action taken and the shifted quantiles of the bootstrap action (summed over
    the head's quantiles, averaged over the target's: sb3_contrib's ``quantile_huber_loss``), attached to autograd: ``backward()`` puts
    the gradients on the head's parameters and on ``features``.  ``metrics`` maps DQN_SCALARS to detached 0-d tensors (loss, the mean q
    of the action taken, the mean of the target quantiles); ``row_loss`` [B], detached, is each row's loss, unweighted: the priority of
    prioritized replay."""
    net = policy.q_net
    if not isinstance(net, QuantileQNetwork):
        raise TypeError(f"{_WHO}.qr_loss: the policy's head is a {type(net).__name__}, not a QuantileQNetwork (build it with n_quantiles >= 1)")
    loss, scal, row_loss = _QrTdFn.apply(features, next_quantiles, next_q, actions, rewards, dones, discounts, weights, gamma, kappa, net._head(),
                                         *net._param_list())
    return loss, {k: scal[i] for i, k in enumerate(DQN_SCALARS)}, row_loss


__all__ = ["QuantileQNetwork", "qr_loss"]
