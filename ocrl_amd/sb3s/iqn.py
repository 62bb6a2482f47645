"""DQN's implicit quantile head: the return distribution of IQN (Dabney, Ostrovski, Silver and Munos 2018) as a function of a sampled
fraction tau.  A cosine embedding of tau (``n_cos`` cosines, a Linear and a ReLU) gates the features, the chain of hidden layers and an
output Linear map the gated features to one quantile value per action, and each row is evaluated at as many fractions as the caller
passes.  Restated from the published algorithm; the GPU work is the library's (include/ocrl_hip_iqn.h, which states every formula):
``ImplicitQuantileQNetwork.quantile_values`` is ``ocrl_iqn_fwd`` / ``ocrl_iqn_bwd`` under a ``torch.autograd.Function``, ``quantiles`` one
``ocrl_iqn_fwd`` call, acting ``ocrl_iqn_act``, the draws ``ocrl_iqn_taus`` and the loss ``iqn_loss`` (``ocrl_iqn_td_fwd_bwd``: the
quantile Huber loss at the sampled fractions against the Bellman-shifted quantile values of the bootstrap action and the head's
gradient, fused).  ``DQN(n_tau_samples=8)`` uses them (dqn.py; ``sb3=iqn``)."""
import ctypes

import torch
from torch import nn

from .. import _bridge, _lib
from .qhead import DQN_SCALARS, QHead, coerce, scaled_grads

_WHO = "ocrl_amd.sb3s"
MAX_TAU_SAMPLES, MAX_COS = 64, 64            # fractions per row of a call, cosines (include/ocrl_hip_iqn.h)
TRAIN_SEED_SALT = 0x9E3779B97F4A7C15         # DQN's training draws: stream (seed + this) mod 2^64, apart from the acting rows' stream


def _desc(B, F, A, N, C, dims, acts, dev, keep=True):
    """(descriptor, workspace) of a call"""
    d = _lib.iqn_desc(B, F, A, N, C, dims, acts)
    return d, _bridge.workspace(_WHO, _lib.lib().ocrl_iqn_ws_floats(ctypes.byref(d)), dev,
                                f"batch {B}, feature_dim {F}, {A} actions, {N} fractions per row, {C} cosines, hidden widths {list(dims)}", keep)


def _taus(taus, B, dev, who):
    """the fractions [B, N] of a call as the kernels take them: (tensor, N)"""
    t = (taus.detach() if taus.requires_grad else taus).to(device=dev, dtype=torch.float32)
    if t.dim() != 2 or t.shape[0] != B or t.shape[1] < 1:
        raise ValueError(f"{_WHO}.{who}: taus is [batch, n] with n >= 1 (got {tuple(taus.shape)} for a batch of {B})")
    return t.contiguous(), int(t.shape[1])


def draw_taus(seed, row_offset, B, N, dev):
    """[B, N] fractions k / 2^24 of rows row_offset .. row_offset + B of stream ``seed``: one ``ocrl_iqn_taus`` launch"""
    out = torch.empty(int(B), int(N), device=dev, dtype=torch.float32)
    _bridge.launch(out.device, _lib.lib().ocrl_iqn_taus, int(seed) & (2 ** 64 - 1), int(row_offset) & (2 ** 64 - 1), int(B), int(N), _lib.ptr(out))
    return out


class _IqnFn(torch.autograd.Function):
    """quantile values [B, A, N] of a feature batch at the fractions taus [B, N]"""

    @staticmethod
    def forward(ctx, features, taus, head, *params):
        A, C, dims, acts = head
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        taus, N = _taus(taus, B, dev, "ImplicitQuantileQNetwork.quantile_values")
        need_grad = any(ctx.needs_input_grad)
        d, ws = _desc(B, F, A, N, C, dims, acts, dev, need_grad)
        theta = torch.empty(B, A, N, device=dev)
        _bridge.launch(dev, _lib.lib().ocrl_iqn_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptr(taus), _lib.ptrs(ps), _lib.ptr(theta), None,
                       int(need_grad), _lib.ptr(ws) if need_grad else None, ws.numel())
        ctx.save_for_backward(x, taus, *ps)
        ctx.d, ctx.ws = d, ws
        return theta

    @staticmethod
    def backward(ctx, dtheta):
        x, taus, *ps = ctx.saved_tensors
        dtheta = _bridge.cotangent(dtheta)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(x.device, _lib.lib().ocrl_iqn_bwd, ctypes.byref(ctx.d), _lib.ptr(x), _lib.ptr(taus), _lib.ptrs(ps), _lib.ptr(dtheta),
                       _lib.ptr(dx), _lib.ptrs(gs), _lib.ptr(ctx.ws), ctx.ws.numel())
        return (dx, None, None, *gs)


class _IqnTdFn(torch.autograd.Function):
    """the fused TD step: (loss, scalars [3], row_loss [B]); the gradients are the forward's own outputs"""

    @staticmethod
    def forward(ctx, features, taus, next_quantiles, next_q, actions, rewards, dones, discounts, weights, gamma, kappa, head, *params):
        A, C, dims, acts = head
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        f32 = torch.float32
        taus, N = _taus(taus, B, dev, "iqn_loss")
        if next_quantiles.dim() != 3 or tuple(next_quantiles.shape[:2]) != (B, A):
            raise ValueError(f"{_WHO}.iqn_loss: next_quantiles is [batch, n_actions, n'] (got {tuple(next_quantiles.shape)} for a batch of {B} and "
                             f"{A} actions)")
        Np = int(next_quantiles.shape[2])
        actions, rewards, dones, next_quantiles, next_q, discounts, weights = coerce(
            f"{_WHO}.iqn_loss", dev, f"a batch of {B}, {A} actions and {Np} target fractions", ("actions", actions, torch.int64, B),
            ("rewards", rewards, f32, B), ("dones", dones, torch.uint8, B), ("next_quantiles", next_quantiles, f32, B * A * Np),
            ("next_q", next_q, f32, B * A), ("discounts", discounts, f32, B), ("weights", weights, f32, B))
        d, ws = _desc(B, F, A, N, C, dims, acts, dev)
        scal = torch.empty(3, device=dev, dtype=torch.float32)
        row_loss = torch.empty(B, device=dev, dtype=torch.float32)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(dev, _lib.lib().ocrl_iqn_td_fwd_bwd, ctypes.byref(d), _lib.ptr(x), _lib.ptr(taus), _lib.ptrs(ps), _lib.ptr(next_quantiles), Np,
                       _lib.ptr(next_q), _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones), _lib.ptr(discounts), _lib.ptr(weights), float(gamma),
                       float(kappa), _lib.ptr(scal), _lib.ptr(row_loss), _lib.ptr(dx), _lib.ptrs(gs), _lib.ptr(ws), ws.numel())
        ctx.gs, ctx.dx = gs, dx
        ctx.mark_non_differentiable(scal, row_loss)
        return scal[0].clone(), scal, row_loss

    @staticmethod
    def backward(ctx, gloss, _gscal, _grow):
        return scaled_grads(ctx, gloss, 11)


class ImplicitQuantileQNetwork(QHead):
    """(features [B, F], taus [B, N]) -> theta [B, n_actions, N]: phi = relu(tau_embedding(cos(pi k tau), k < n_cos)) [F] gates the
    features, then len(net_arch) x [Linear, activation] -> Linear(last, n_actions) on features * phi.  The chain's parameters sit in
    ``q_net``, an nn.Sequential with QNetwork's keys (``q_net.{2i}.weight|bias``; QHead), the embedding's in ``tau_embedding``, always a
    plain Linear(n_cos, F); neither container's ``forward`` is called.  ``noisy``: the chain's Linears, the output layer included, are
    NoisyLinears; the embedding is not.  ``n_act_samples`` (K) is the number of fractions acting and ``forward`` use.  ``forward`` and
    deterministic acting take the midpoints (s + 0.5) / K, a fixed quadrature, so evaluation needs no stream; exploring acting draws K
    fractions per row.  No CPU fallback: a CPU tensor raises."""

    def __init__(self, features_dim, n_actions, n_cos=64, n_act_samples=32, net_arch=(64, 64), activation="relu", noisy=False, noisy_sigma0=0.5):
        super().__init__(features_dim, int(n_actions), net_arch, activation, noisy, noisy_sigma0)
        self.n_actions, self.n_cos, self.n_act_samples = int(n_actions), int(n_cos), int(n_act_samples)
        if not (4 <= self.n_cos <= MAX_COS and self.n_cos % 4 == 0):
            raise ValueError(f"{_WHO}.ImplicitQuantileQNetwork: n_cos is a multiple of 4 in 4 .. {MAX_COS} (got {n_cos})")
        if not 1 <= self.n_act_samples <= MAX_TAU_SAMPLES:
            raise ValueError(f"{_WHO}.ImplicitQuantileQNetwork: n_act_samples lies in 1 .. {MAX_TAU_SAMPLES} (got {n_act_samples})")
        self.features_dim = int(features_dim)
        self.tau_embedding = nn.Linear(self.n_cos, self.features_dim)
        self.register_buffer("midpoints", (torch.arange(self.n_act_samples, dtype=torch.float32) + 0.5) / self.n_act_samples, persistent=False)

    def _head(self):
        """what the autograd functions need of the head besides its parameters"""
        return (self.n_actions, self.n_cos, *self._layout())

    def _param_list(self):
        """the embedding's (weight, bias), then QHead's list: the order the kernels take"""
        return [self.tau_embedding.weight, self.tau_embedding.bias] + super()._param_list()

    def _midpoints(self, B):
        return self.midpoints.unsqueeze(0).expand(B, -1).contiguous()

    def quantile_values(self, features, taus):
        """theta [B, n_actions, N] at taus [B, N], attached to autograd (the fractions get no gradient)"""
        return _IqnFn.apply(features, taus, self._head(), *self._param_list())

    def forward(self, features):
        """q [B, n_actions] at the midpoints (s + 0.5) / n_act_samples: the mean of ``quantile_values`` over them, attached to autograd;
        under ``torch.no_grad()`` the kernel's own q (``quantiles``)"""
        taus = self._midpoints(features.shape[0])
        if not torch.is_grad_enabled():
            return self.quantiles(features, taus)[1]
        return self.quantile_values(features, taus).mean(-1)

    def quantiles(self, features, taus):
        """(theta [B, n_actions, N], q [B, n_actions]) at taus [B, N] in one call, detached: what a target network is asked for"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        B, F = x.shape
        taus, N = _taus(taus, B, x.device, "ImplicitQuantileQNetwork.quantiles")
        d = _lib.iqn_desc(B, F, self.n_actions, N, self.n_cos, *self._layout())
        theta = torch.empty(B, self.n_actions, N, device=x.device)
        q = torch.empty(B, self.n_actions, device=x.device)
        _bridge.launch(x.device, _lib.lib().ocrl_iqn_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptr(taus), _lib.ptrs(ps), _lib.ptr(theta), _lib.ptr(q), 0,
                       None, 0)
        return theta, q

    def act(self, features, seed, row_offset, epsilon, uniforms, taus=None, deterministic=False):
        """(actions int64 [B], q [B, n_actions]) of ``ocrl_iqn_act``: DQNPolicy.act's launch for this head.  ``taus`` [B, n_act_samples]
        replaces the fractions; without them ``deterministic`` takes the midpoints, else row r draws its n_act_samples fractions from
        (seed, row_offset + r) (``ocrl_iqn_taus``' rule)"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        B, F = x.shape
        if taus is None and deterministic:
            taus = self._midpoints(B)
        N = self.n_act_samples
        if taus is not None:
            taus, N = _taus(taus, B, x.device, "ImplicitQuantileQNetwork.act")
        d = _lib.iqn_desc(B, F, self.n_actions, N, self.n_cos, *self._layout())
        return self._launch_act(_lib.lib().ocrl_iqn_act, d, x, ps, seed, row_offset, epsilon, uniforms, after=(_lib.ptr(taus),))


def iqn_loss(policy, features, taus, next_quantiles, next_q, actions, rewards, dones, gamma, kappa=1.0, discounts=None, weights=None):
    """The quantile Huber loss of ``policy`` (a DQNPolicy with an ImplicitQuantileQNetwork) on a feature batch [B, F] at the fractions
    ``taus`` [B, N] against the quantile values of the next observations: (loss, metrics, row_loss).  ``next_quantiles`` [B, n, N'] is the
    target network's at N' fractions of its own, ``next_q`` [B, n] names the bootstrap action (the target network's, or the online
    network's for double Q-learning); ``kappa`` is the Huber threshold, ``discounts`` [B] replaces ``gamma`` per row, ``weights`` [B]
    scales each row's loss and gradient.  ``loss`` is the mean over the rows of the quantile Huber loss between the N quantile values of
    the action taken and the N' shifted ones of the bootstrap action (summed over N, averaged over N'), attached to autograd:
    ``backward()`` puts the gradients on the head's parameters and on ``features``.  ``metrics`` maps DQN_SCALARS to detached 0-d tensors
    (loss, the mean q of the action taken, the mean of the targets); ``row_loss`` [B], detached, is each row's loss, unweighted: the
    priority of prioritized replay."""
    net = policy.q_net
    if not isinstance(net, ImplicitQuantileQNetwork):
        raise TypeError(f"{_WHO}.iqn_loss: the policy's head is a {type(net).__name__}, not an ImplicitQuantileQNetwork (build it with "
                        "n_tau_samples >= 1)")
    loss, scal, row_loss = _IqnTdFn.apply(features, taus, next_quantiles, next_q, actions, rewards, dones, discounts, weights, gamma, kappa,
                                          net._head(), *net._param_list())
    return loss, {k: scal[i] for i, k in enumerate(DQN_SCALARS)}, row_loss


__all__ = ["ImplicitQuantileQNetwork", "iqn_loss"]
