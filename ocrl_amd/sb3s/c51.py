"""DQN's categorical head: the return distribution of C51 (Bellemare, Dabney and Munos 2017) over ``n_atoms`` fixed atoms between
``v_min`` and ``v_max``, optionally with the dueling aggregation (Wang et al. 2016) applied per atom, as Rainbow (Hessel et al. 2018)
combines them.  Restated from the published algorithms; the GPU work is the library's (include/ocrl_hip_c51.h, which states every
formula): ``CategoricalQNetwork.logits`` is ``ocrl_c51_fwd`` / ``ocrl_c51_bwd`` under a ``torch.autograd.Function``, ``distribution`` one
``ocrl_c51_fwd`` launch, acting ``ocrl_c51_act`` and the loss ``c51_loss`` (``ocrl_c51_td_fwd_bwd``: the projection of the target
distribution onto the support, the cross-entropy and the head's gradient, fused).  ``DQN(n_atoms=51, dueling=True)`` uses them
(dqn.py; ``sb3=dqn_c51``)."""
import ctypes

import torch

from .. import _bridge, _lib
from .qhead import DQN_SCALARS, QHead, coerce, scaled_grads

_WHO = "ocrl_amd.sb3s"


def _desc(B, F, A, Z, dims, acts, dueling, dev, keep=True):
    """(descriptor, workspace) of a call"""
    d = _lib.c51_desc(B, F, A, Z, dims, acts, dueling)
    return d, _bridge.workspace(_WHO, _lib.lib().ocrl_c51_ws_floats(ctypes.byref(d)), dev,
                                f"batch {B}, feature_dim {F}, {A} actions of {Z} atoms, hidden widths {list(dims)}", keep)


class _C51Fn(torch.autograd.Function):
    """logits [B, A, Z] of a feature batch"""

    @staticmethod
    def forward(ctx, features, head, *params):
        A, Z, dims, acts, dueling, v_min, v_max = head
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        need_grad = any(ctx.needs_input_grad)
        d, ws = _desc(B, F, A, Z, dims, acts, dueling, dev, need_grad)
        logits = torch.empty(B, A, Z, device=dev)
        _bridge.launch(dev, _lib.lib().ocrl_c51_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), v_min, v_max, _lib.ptr(logits), None, None,
                       int(need_grad), _lib.ptr(ws) if need_grad else None, ws.numel())
        ctx.save_for_backward(x, *ps)
        ctx.d, ctx.ws = d, ws
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        x, *ps = ctx.saved_tensors
        dlogits = _bridge.cotangent(dlogits)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(x.device, _lib.lib().ocrl_c51_bwd, ctypes.byref(ctx.d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(dlogits), _lib.ptr(dx),
                       _lib.ptrs(gs), _lib.ptr(ctx.ws), ctx.ws.numel())
        return (dx, None, *gs)


class _C51TdFn(torch.autograd.Function):
    """the fused TD step: (loss, scalars [3], row_loss [B]); the gradients are the forward's own outputs"""

    @staticmethod
    def forward(ctx, features, next_probs, next_q, actions, rewards, dones, discounts, weights, gamma, head, *params):
        A, Z, dims, acts, dueling, v_min, v_max = head
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        f32 = torch.float32
        actions, rewards, dones, next_probs, next_q, discounts, weights = coerce(
            f"{_WHO}.c51_loss", dev, f"a batch of {B}, {A} actions and {Z} atoms", ("actions", actions, torch.int64, B),
            ("rewards", rewards, f32, B), ("dones", dones, torch.uint8, B), ("next_probs", next_probs, f32, B * A * Z),
            ("next_q", next_q, f32, B * A), ("discounts", discounts, f32, B), ("weights", weights, f32, B))
        d, ws = _desc(B, F, A, Z, dims, acts, dueling, dev)
        scal = torch.empty(3, device=dev, dtype=torch.float32)
        row_loss = torch.empty(B, device=dev, dtype=torch.float32)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(dev, _lib.lib().ocrl_c51_td_fwd_bwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), v_min, v_max, _lib.ptr(next_probs),
                       _lib.ptr(next_q), _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones), _lib.ptr(discounts), _lib.ptr(weights), float(gamma),
                       _lib.ptr(scal), _lib.ptr(row_loss), _lib.ptr(dx), _lib.ptrs(gs), _lib.ptr(ws), ws.numel())
        ctx.gs, ctx.dx = gs, dx
        ctx.mark_non_differentiable(scal, row_loss)
        return scal[0].clone(), scal, row_loss

    @staticmethod
    def backward(ctx, gloss, _gscal, _grow):
        return scaled_grads(ctx, gloss, 9)


class CategoricalQNetwork(QHead):
    """features [B, F] -> len(net_arch) x [Linear, activation] -> Linear(last, n_actions * n_atoms), atom j of action a in column
    a * n_atoms + j; with ``dueling`` a second Linear(last, n_atoms), ``value_net``, on the same latent:
    logit[a, j] = V[j] + Adv[a, j] - mean_a' Adv[a', j].  The parameters sit in ``q_net``, an nn.Sequential with QNetwork's keys
    (``q_net.{2i}.weight|bias``; QHead), and in ``value_net``; neither container's ``forward`` is called.  ``n_actions``, ``n_atoms`` and the
    support ``atoms`` [n_atoms] = v_min + j (v_max - v_min) / (n_atoms - 1) are attributes.  ``noisy``: every Linear, the advantage and
    the value layer included, is a NoisyLinear, as QNetwork's.  No CPU fallback: a CPU tensor raises."""

    def __init__(self, features_dim, n_actions, n_atoms, v_min, v_max, net_arch=(64, 64), activation="relu", dueling=False, noisy=False,
                 noisy_sigma0=0.5):
        super().__init__(features_dim, int(n_actions) * int(n_atoms), net_arch, activation, noisy, noisy_sigma0)
        self.n_actions, self.n_atoms, self.dueling = int(n_actions), int(n_atoms), bool(dueling)
        self.v_min, self.v_max = float(v_min), float(v_max)
        if self.n_atoms < 2 or not self.v_min < self.v_max:
            raise ValueError(f"{_WHO}.CategoricalQNetwork: n_atoms >= 2 and v_min < v_max (got {n_atoms}, {v_min}, {v_max})")
        if self.dueling:
            self.value_net = self._linear(self.latent_dim, self.n_atoms)
        self.register_buffer("atoms", torch.linspace(self.v_min, self.v_max, self.n_atoms), persistent=False)

    def _head(self):
        """what the autograd functions need of the head besides its parameters"""
        return (self.n_actions, self.n_atoms, *self._layout(), self.dueling, self.v_min, self.v_max)

    def _param_list(self):
        """QHead's list with the value Linear's pair at its end"""
        return super()._param_list(*([self.value_net] if self.dueling else []))

    def logits(self, features):
        """[B, n_actions, n_atoms], attached to autograd"""
        return _C51Fn.apply(features, self._head(), *self._param_list())

    def forward(self, features):
        """the expected q [B, n_actions], formed from ``logits`` with torch operations (attached to autograd)"""
        return (torch.softmax(self.logits(features), dim=-1) * self.atoms).sum(-1)

    def distribution(self, features):
        """(probs [B, n_actions, n_atoms], q [B, n_actions]) in one launch, detached: what a target network is asked for"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        B, F = x.shape
        d, _ = _desc(B, F, self.n_actions, self.n_atoms, *self._layout(), self.dueling, x.device, keep=False)
        probs = torch.empty(B, self.n_actions, self.n_atoms, device=x.device)
        q = torch.empty(B, self.n_actions, device=x.device)
        _bridge.launch(x.device, _lib.lib().ocrl_c51_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), self.v_min, self.v_max, None, _lib.ptr(probs),
                       _lib.ptr(q), 0, None, 0)
        return probs, q

    def act(self, features, seed, row_offset, epsilon, uniforms):
        """(actions int64 [B], q [B, n_actions]) of ``ocrl_c51_act``: DQNPolicy.act's launch for this head"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        B, F = x.shape
        d, _ = _desc(B, F, self.n_actions, self.n_atoms, *self._layout(), self.dueling, x.device, keep=False)
        return self._launch_act(_lib.lib().ocrl_c51_act, d, x, ps, seed, row_offset, epsilon, uniforms, before=(self.v_min, self.v_max))


def c51_loss(policy, features, next_probs, next_q, actions, rewards, dones, gamma, discounts=None, weights=None):
    """The categorical loss of ``policy`` (a DQNPolicy with a CategoricalQNetwork) on a feature batch [B, F] against the distribution of
    the next observations: (loss, metrics, row_loss).  ``next_probs`` [B, n, Z] is the target network's, ``next_q`` [B, n] names the
    bootstrap action (the target network's, or the online network's for double Q-learning); ``discounts`` [B] replaces ``gamma`` per row,
    ``weights`` [B] scales each row's loss and gradient.  ``loss`` is the mean cross-entropy between the projected target distribution and
    the head's distribution of the action taken, attached to autograd: ``backward()`` puts the gradients on the head's parameters and on
    ``features``.  ``metrics`` maps DQN_SCALARS to detached 0-d tensors (loss, the mean expected q of the action taken, the mean of the
    projected target); ``row_loss`` [B], detached, is each row's cross-entropy, unweighted: the priority of prioritized replay."""
    net = policy.q_net
    if not isinstance(net, CategoricalQNetwork):
        raise TypeError(f"{_WHO}.c51_loss: the policy's head is a {type(net).__name__}, not a CategoricalQNetwork (build it with n_atoms >= 2)")
    loss, scal, row_loss = _C51TdFn.apply(features, next_probs, next_q, actions, rewards, dones, discounts, weights, gamma, net._head(),
                                          *net._param_list())
    return loss, {k: scal[i] for i, k in enumerate(DQN_SCALARS)}, row_loss


__all__ = ["CategoricalQNetwork", "c51_loss"]
