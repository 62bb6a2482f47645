"""DQN's fully parameterized quantile function: FQF (Yang, Zhao, Lin, Qin, Bian and Liu 2019).  The fractions at which the implicit
quantile head (iqn.py) is evaluated are neither fixed nor drawn: ``fraction_net``, a Linear on the features followed by a soft-max,
proposes N intervals per row, the head is evaluated at their midpoints tau_hat, q is the interval-weighted sum of the quantile values,
and the proposal is trained on the gradient of the 1-Wasserstein error of the staircase with respect to the interval boundaries.
Restated from the published algorithm; the GPU work is the library's (include/ocrl_hip_fqf.h, which states every formula):
``FullyParameterizedQuantileQNetwork.fractions`` is one ``ocrl_fqf_fractions`` launch, ``quantiles`` the unchanged ``ocrl_iqn_fwd`` at
tau_hat and ``ocrl_fqf_q``, acting ``ocrl_fqf_fractions`` + ``ocrl_fqf_act``, and ``fqf_fraction_loss`` one head forward at the 2 N - 1
fractions of ``eval_taus`` followed by ``ocrl_fqf_fraction_bwd``.  The head's own loss is ``iqn_loss`` at tau_hat, unchanged.
``DQN(fqf=True, n_tau_samples=32)`` uses them (dqn.py; ``sb3=fqf``)."""
import collections
import ctypes

import torch
from torch import nn

from .. import _bridge, _lib
from .iqn import ImplicitQuantileQNetwork, _taus
from .qhead import coerce

_WHO = "ocrl_amd.sb3s"
MAX_FRACTIONS = 32                           # proposed intervals per row: 2 N - 1 <= 63 fractions of one head forward (include/ocrl_hip_fqf.h)
FQF_SCALARS = ("fraction_loss", "fraction_entropy")
Fractions = collections.namedtuple("Fractions", "taus tau_hats eval_taus logp entropy")


class FullyParameterizedQuantileQNetwork(ImplicitQuantileQNetwork):
    """An ImplicitQuantileQNetwork whose fractions come from ``fraction_net`` = Linear(features_dim, n_fractions) (Xavier-uniform at
    gain 0.01, zero bias: a near-uniform start; never noisy): ``fractions(features)`` gives the boundaries taus [B, N + 1] (0 first, 1
    last, non-decreasing), the midpoints tau_hats [B, N], both in one block eval_taus [B, 2 N - 1], and the proposal's log-probabilities
    and entropy.  ``forward``, ``quantiles`` and ``act`` evaluate the head at the proposed tau_hats, in training and in evaluation alike,
    and weight the quantile values by the intervals.  The proposal reads the features detached and takes its gradient from
    ``fqf_fraction_loss`` alone.  No CPU fallback: a CPU tensor raises."""

    def __init__(self, features_dim, n_actions, n_fractions=32, n_cos=64, net_arch=(64, 64), activation="relu", noisy=False, noisy_sigma0=0.5):
        if not 2 <= int(n_fractions) <= MAX_FRACTIONS:
            raise ValueError(f"{_WHO}.FullyParameterizedQuantileQNetwork: n_fractions lies in 2 .. {MAX_FRACTIONS} (got {n_fractions})")
        super().__init__(features_dim, n_actions, n_cos, int(n_fractions), net_arch, activation, noisy, noisy_sigma0)
        self.n_fractions = int(n_fractions)
        self.fraction_net = nn.Linear(self.features_dim, self.n_fractions)
        nn.init.xavier_uniform_(self.fraction_net.weight, gain=0.01)
        nn.init.zeros_(self.fraction_net.bias)

    def fractions(self, features):
        """Fractions(taus [B, N + 1], tau_hats [B, N], eval_taus [B, 2 N - 1], logp [B, N], entropy [B]) of a feature batch, detached:
        one ``ocrl_fqf_fractions`` launch"""
        x, (W, b) = _bridge.inputs(_WHO, features.detach(), [self.fraction_net.weight, self.fraction_net.bias])
        B, F = x.shape
        N, dev = self.n_fractions, x.device
        out = Fractions(*(torch.empty(B, n, device=dev) for n in (N + 1, N, 2 * N - 1, N)), torch.empty(B, device=dev))
        _bridge.launch(dev, _lib.lib().ocrl_fqf_fractions, _lib.ptr(x), _lib.ptr(W), _lib.ptr(b), B, F, N, *(_lib.ptr(t) for t in out))
        return out

    def _bounds(self, taus, B, dev, who):
        """the boundaries [B, N + 1] of a call as the kernels take them"""
        t, n = _taus(taus, B, dev, who)
        if n != self.n_fractions + 1:
            raise ValueError(f"{_WHO}.{who}: taus is [batch, n_fractions + 1] = [{B}, {self.n_fractions + 1}] (got {tuple(taus.shape)})")
        return t

    def weighted_q(self, theta, taus):
        """q [B, n_actions] = sum_i (tau_{i+1} - tau_i) theta[:, :, i] of quantile values [B, n_actions, N] at tau_hats: ``ocrl_fqf_q``"""
        theta = _bridge.gpu_input(_WHO, theta.detach())
        B, A, N = theta.shape
        taus = self._bounds(taus, B, theta.device, "FullyParameterizedQuantileQNetwork.weighted_q")
        q = torch.empty(B, A, device=theta.device)
        _bridge.launch(theta.device, _lib.lib().ocrl_fqf_q, _lib.ptr(theta), _lib.ptr(taus), B, A, N, _lib.ptr(q))
        return q

    def theta(self, features, fractions):
        """quantile values [B, n_actions, M] at fractions [B, M], detached: one ``ocrl_iqn_fwd`` launch, no workspace"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        B, F = x.shape
        fr, M = _taus(fractions, B, x.device, "FullyParameterizedQuantileQNetwork.theta")
        d = _lib.iqn_desc(B, F, self.n_actions, M, self.n_cos, *self._layout())
        theta = torch.empty(B, self.n_actions, M, device=x.device)
        _bridge.launch(x.device, _lib.lib().ocrl_iqn_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptr(fr), _lib.ptrs(ps), _lib.ptr(theta), None, 0, None, 0)
        return theta

    def quantiles(self, features, taus=None):
        """(theta [B, n_actions, N] at the midpoints of the boundaries ``taus`` [B, N + 1], q [B, n_actions] weighted by the intervals),
        detached: what a target network is asked for.  Without ``taus`` this network's own proposal on ``features``."""
        if taus is None:
            taus = self.fractions(features).taus
        taus = self._bounds(taus, features.shape[0], features.device, "FullyParameterizedQuantileQNetwork.quantiles")
        theta = self.theta(features, 0.5 * (taus[:, :-1] + taus[:, 1:]))            # ocrl_fqf_fractions' tau_hats, bit for bit
        return theta, self.weighted_q(theta, taus)

    def forward(self, features):
        """q [B, n_actions] at the proposed fractions; attached to autograd through the head (the fractions get no gradient), and under
        ``torch.no_grad()`` the kernels' own q (``quantiles``)"""
        if not torch.is_grad_enabled():
            return self.quantiles(features)[1]
        fr = self.fractions(features)
        return (self.quantile_values(features, fr.tau_hats) * (fr.taus[:, 1:] - fr.taus[:, :-1]).unsqueeze(1)).sum(-1)

    def act(self, features, seed, row_offset, epsilon, uniforms, taus=None, deterministic=False):
        """(actions int64 [B], q [B, n_actions]): DQNPolicy.act's two launches for this head, ``ocrl_fqf_fractions`` (skipped when the
        boundaries ``taus`` [B, N + 1] are given) and ``ocrl_fqf_act``.  ``deterministic`` changes nothing here: the proposed fractions
        are a function of the features"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        B, F = x.shape
        taus = self.fractions(x).taus if taus is None else self._bounds(taus, B, x.device, "FullyParameterizedQuantileQNetwork.act")
        d = _lib.fqf_desc(B, F, self.n_actions, self.n_fractions, self.n_cos, *self._layout())
        return self._launch_act(_lib.lib().ocrl_fqf_act, d, x, ps, seed, row_offset, epsilon, uniforms, before=(_lib.ptr(taus),))


def fqf_fraction_loss(policy, features, actions, weights=None, ent_coef=0.0, fractions=None):
    """The fraction loss of ``policy`` (a DQNPolicy with a FullyParameterizedQuantileQNetwork) on a feature batch [B, F], without
    autograd: fills ``.grad`` of ``fraction_net``'s weight and bias (overwritten, not accumulated) with the gradient of
    mean_b w_b W1(b) - ent_coef * mean_b H_b, where dW1 / dtau_i = 2 theta(tau_i) - theta(tau_hat_i) - theta(tau_hat_{i-1}) on the quantile
    values of the action taken (the paper's Proposition 1), and returns {fraction_loss, fraction_entropy} as detached 0-d tensors.
    ``weights`` [B] scales each row's W1 term; ``fractions``: what ``policy.q_net.fractions(features)`` gave, when the caller has it.
    One head forward at eval_taus (no gradient: the head learns from ``iqn_loss``), then ``ocrl_fqf_fraction_bwd``."""
    net = policy.q_net
    if not isinstance(net, FullyParameterizedQuantileQNetwork):
        raise TypeError(f"{_WHO}.fqf_fraction_loss: the policy's head is a {type(net).__name__}, not a FullyParameterizedQuantileQNetwork "
                        "(build it with fqf=True)")
    x = _bridge.gpu_input(_WHO, features.detach())
    dev = x.device
    B, F = x.shape
    A, N = net.n_actions, net.n_fractions
    fr = net.fractions(x) if fractions is None else fractions
    theta = net.theta(x, fr.eval_taus)
    actions, weights, logp, entropy = coerce(f"{_WHO}.fqf_fraction_loss", dev, f"a batch of {B} and {N} fractions", ("actions", actions, torch.int64, B),
                                             ("weights", weights, torch.float32, B), ("logp", fr.logp, torch.float32, B * N),
                                             ("entropy", fr.entropy, torch.float32, B))
    W, b = net.fraction_net.weight, net.fraction_net.bias
    for p in (W, b):
        if p.grad is None or not p.grad.is_contiguous():
            p.grad = torch.empty_like(p, memory_format=torch.contiguous_format)
    ws = _bridge.workspace(_WHO, _lib.lib().ocrl_fqf_ws_floats(B, F, N), dev, f"batch {B}, feature_dim {F}, {N} fractions")
    scal = torch.empty(2, device=dev, dtype=torch.float32)
    _bridge.launch(dev, _lib.lib().ocrl_fqf_fraction_bwd, _lib.ptr(x), _lib.ptr(logp), _lib.ptr(entropy), _lib.ptr(theta), _lib.ptr(actions),
                   _lib.ptr(weights), float(ent_coef), B, F, A, N, _lib.ptr(W.grad), _lib.ptr(b.grad), _lib.ptr(scal), _lib.ptr(ws), ws.numel())
    return {k: scal[i] for i, k in enumerate(FQF_SCALARS)}


__all__ = ["FullyParameterizedQuantileQNetwork", "fqf_fraction_loss"]
