"""DQN on the GPU: what the reference would select with ``sb3=dqn`` (configs/sb3/dqn.yaml), the value-based baseline on the same
Discrete sprite tasks and the same ``OCRExtractor``.

``DQNPolicy`` and ``DQN`` restate stable-baselines3 1.5's classes of the same names from the published algorithm (Mnih et al. 2015) with
that package's hyper-parameter names and defaults: none of its text is copied.  The GPU work is the library's (include/ocrl_hip_dqn.h):
acting is ``ocrl_dqn_act`` (the Q head's forward and the epsilon-greedy choice in one launch after the extractor), the replay buffer
(replay.py) samples and reads a batch in two launches, the loss is ``dqn_loss`` (``ocrl_dqn_td_fwd_bwd``: the TD target, the Huber loss
and the head's gradient, fused) and the update ``ocrl_flat_clip_adam_l2`` on one flat parameter buffer.  Double Q-learning (van Hasselt et al. 2016),
n-step returns and proportional prioritized replay (Schaul et al. 2016) are keyword arguments of ``DQN``, off by default
(include/ocrl_hip_replay.h; ``sb3=dqn_per``).  ``n_atoms >= 2`` replaces the scalar head by the categorical one (C51, Bellemare et al.
2017) and ``dueling`` adds its value stream (c51.py, include/ocrl_hip_c51.h; ``sb3=dqn_c51``); both are off by default.  ``noisy`` makes
every Linear of the head a noisy layer (Fortunato et al. 2018) whose learned parameter noise replaces the epsilon-greedy coin (noisy.py,
include/ocrl_hip_noisy.h; ``sb3=rainbow``, the six components of Hessel et al. 2018 together); off by default.  ``n_quantiles >= 1``
replaces the scalar head by the quantile one (QR-DQN, Dabney et al. 2018: the return distribution without a support; qr.py,
include/ocrl_hip_qr.h; ``sb3=qrdqn``), with ``dueling`` and ``noisy`` as for the categorical head; off by default.  ``n_tau_samples >= 1``
replaces it by the implicit quantile one (IQN, Dabney et al. 2018: the quantile values as a function of sampled fractions; iqn.py,
include/ocrl_hip_iqn.h; ``sb3=iqn``), with ``noisy`` but without ``dueling``; off by default.  ``munchausen`` rewrites the rewards
and the target network's values at the next observation in front of the scalar, quantile and implicit quantile heads' unchanged TD steps
(Munchausen RL, Vieillard et al. 2020: the clipped log-policy bonus and the soft value of a soft-max policy; munchausen.py,
include/ocrl_hip_munchausen.h; ``sb3=mdqn``, ``sb3=miqn``); off by default.  ``fqf`` lets a small network
propose the implicit quantile head's fractions per state and trains it on the 1-Wasserstein error of the staircase they make (FQF, Yang
et al. 2019; fqf.py, include/ocrl_hip_fqf.h; ``sb3=fqf``); off by default.  Where this departs
from stable-baselines3 and from those papers is listed in DESIGN.md §7."""
import collections
import copy
import ctypes
import math

import numpy as np
import torch
from torch import nn

from .. import _bridge, _lib
from ..ocrs.flat_module import FlatParamModule
from .c51 import CategoricalQNetwork, c51_loss
from .fqf import FQF_SCALARS, MAX_FRACTIONS, FullyParameterizedQuantileQNetwork, fqf_fraction_loss
from .iqn import MAX_COS, MAX_TAU_SAMPLES, TRAIN_SEED_SALT, ImplicitQuantileQNetwork, draw_taus, iqn_loss
from .munchausen import check_munchausen, munchausen_targets
from .custom_acnets import _n_actions
from .on_policy import OnPolicyAlgorithm, _check_constant, _tensor
from .qhead import DQN_SCALARS, QHead, coerce, scaled_grads
from .qr import MAX_QUANTILE_COLS, MAX_QUANTILES, QuantileQNetwork, qr_loss
from .replay import MAX_N_STEP, ReplayBuffer

_WHO = "ocrl_amd.sb3s"
MAX_ATOMS, MAX_LOGITS = 64, 256   # of the categorical head: atoms per action, n_actions * n_atoms (include/ocrl_hip_c51.h)
FQF_RMS_ALPHA, FQF_RMS_EPS = 0.95, 1e-5   # the fraction proposal's RMSprop (the FQF paper's setting)
ADAM_EPS = 1e-8                 # stable-baselines3's DQNPolicy builds torch's default Adam (the actor-critic policy: 1e-5)


def _desc(B, F, A, dims, acts, dev, keep=True):
    """(descriptor, workspace) of a call"""
    d = _lib.qnet_desc(B, F, A, dims, acts)
    return d, _bridge.workspace(_WHO, _lib.lib().ocrl_qnet_ws_floats(ctypes.byref(d)), dev,
                                f"batch {B}, feature_dim {F}, {A} actions, hidden widths {list(dims)}", keep)


class _QnetFn(torch.autograd.Function):
    """q [B, A] of a feature batch"""

    @staticmethod
    def forward(ctx, features, dims, acts, A, *params):
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        need_grad = any(ctx.needs_input_grad)
        d, ws = _desc(B, F, A, dims, acts, dev, need_grad)
        q = torch.empty(B, A, device=dev)
        _bridge.launch(dev, _lib.lib().ocrl_qnet_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(q), int(need_grad),
                       _lib.ptr(ws) if need_grad else None, ws.numel())
        ctx.save_for_backward(x, *ps)
        ctx.d, ctx.ws = d, ws
        return q

    @staticmethod
    def backward(ctx, dq):
        x, *ps = ctx.saved_tensors
        dq = _bridge.cotangent(dq)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(x.device, _lib.lib().ocrl_qnet_bwd, ctypes.byref(ctx.d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(dq), _lib.ptr(dx), _lib.ptrs(gs),
                       _lib.ptr(ctx.ws), ctx.ws.numel())
        return (dx, None, None, None, *gs)


class _DqnTdFn(torch.autograd.Function):
    """the fused TD step: (loss, scalars [3], |delta| per row or None); the gradients are the forward's own outputs.  With none of
    the optional inputs of ocrl_dqn_td_fwd_bwd_ext (include/ocrl_hip_replay.h) given and no ``want_abs_td`` the call is
    ocrl_dqn_td_fwd_bwd's"""

    @staticmethod
    def forward(ctx, features, next_q, next_q_online, actions, rewards, dones, discounts, weights, gamma, want_abs_td, dims, acts, A, *params):
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        f32 = torch.float32
        actions, rewards, dones, next_q, next_q_online, discounts, weights = coerce(
            f"{_WHO}.dqn_loss", dev, f"a batch of {B} and {A} actions", ("actions", actions, torch.int64, B), ("rewards", rewards, f32, B),
            ("dones", dones, torch.uint8, B), ("next_q", next_q, f32, B * A), ("next_q_online", next_q_online, f32, B * A),
            ("discounts", discounts, f32, B), ("weights", weights, f32, B))
        d, ws = _desc(B, F, A, dims, acts, dev)
        scal = torch.empty(3, device=dev, dtype=f32)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        abs_td = None
        if next_q_online is None and discounts is None and weights is None and not want_abs_td:
            _bridge.launch(dev, _lib.lib().ocrl_dqn_td_fwd_bwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(next_q), _lib.ptr(actions),
                           _lib.ptr(rewards), _lib.ptr(dones), float(gamma), _lib.ptr(scal), _lib.ptr(dx), _lib.ptrs(gs), _lib.ptr(ws), ws.numel())
        else:
            abs_td = torch.empty(B, device=dev, dtype=f32)
            _bridge.launch(dev, _lib.lib().ocrl_dqn_td_fwd_bwd_ext, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(next_q),
                           _lib.ptr(next_q_online), _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones), _lib.ptr(discounts), _lib.ptr(weights),
                           float(gamma), _lib.ptr(scal), _lib.ptr(abs_td), _lib.ptr(dx), _lib.ptrs(gs), _lib.ptr(ws), ws.numel())
        ctx.gs, ctx.dx = gs, dx              # the gradients are the forward's own outputs: the backward reads nothing else again
        ctx.mark_non_differentiable(*(t for t in (scal, abs_td) if t is not None))
        return scal[0].clone(), scal, abs_td

    @staticmethod
    def backward(ctx, gloss, _gscal, _gtd):
        return scaled_grads(ctx, gloss, 12)


class QNetwork(QHead):
    """features [B, F] -> len(net_arch) x [Linear, activation] -> Linear(last, n_actions).  The parameters sit in ``q_net`` (QHead); the
    arithmetic is ``ocrl_qnet_fwd`` / ``ocrl_qnet_bwd`` under a ``torch.autograd.Function``.  No CPU fallback: a CPU tensor raises."""

    def __init__(self, features_dim, n_actions, net_arch=(64, 64), activation="relu", noisy=False, noisy_sigma0=0.5):
        super().__init__(features_dim, int(n_actions), net_arch, activation, noisy, noisy_sigma0)
        self.n_actions = int(n_actions)

    def forward(self, features):
        return _QnetFn.apply(features, *self._layout(), self.n_actions, *self._param_list())

    def act(self, features, seed, row_offset, epsilon, uniforms):
        """(actions int64 [B], q [B, n_actions]) of ``ocrl_dqn_act``: DQNPolicy.act's launch for this head"""
        x, ps = _bridge.inputs(_WHO, features.detach(), self._param_list())
        d, _ = _desc(*x.shape, self.n_actions, *self._layout(), x.device, keep=False)
        return self._launch_act(_lib.lib().ocrl_dqn_act, d, x, ps, seed, row_offset, epsilon, uniforms)


class DQNPolicy(nn.Module):
    """features_extractor -> QNetwork.  ``features_extractor`` is a module with ``features_dim`` (an OCRExtractor), or
    ``features_extractor_class(observation_space, **features_extractor_kwargs)``; without either the observations are flattened.
    ``exploration_rate`` is the epsilon ``act`` explores with (DQN sets it before every step); the target network is a second DQNPolicy
    (DQN builds it).  ``n_atoms >= 2`` makes the head a CategoricalQNetwork on the support [v_min, v_max] (``dueling``: with its value
    stream); ``q_values`` is then the expectation of the distribution and ``act`` is ``ocrl_c51_act``.  ``n_quantiles >= 1`` (with
    ``n_atoms`` 1) makes it a QuantileQNetwork (``dueling``: with its value stream); ``q_values`` is then the mean of the quantiles
    (``ocrl_qr_fwd``) and ``act`` is ``ocrl_qr_act``.  ``n_tau_samples >= 1`` (with ``n_atoms`` 1, ``n_quantiles`` 0 and no ``dueling``)
    makes it an ImplicitQuantileQNetwork of ``n_cos`` cosines; ``q_values`` is then the mean over the ``n_act_samples`` midpoint
    fractions and ``act`` is ``ocrl_iqn_act`` on ``n_act_samples`` fractions per row, drawn from the policy's stream unless
    ``deterministic``.  ``noisy`` builds the head of noisy
    layers (``noisy_sigma0``: the sigmas' start); which draw of the noise the head uses is set explicitly with ``set_noise`` and does not
    follow ``train()`` / ``eval()``.  ``fqf`` (with ``n_tau_samples`` in 2 .. 32) makes the head a
    FullyParameterizedQuantileQNetwork of ``n_tau_samples`` proposed fractions: ``q_values`` and ``act`` evaluate it at the fractions its
    ``fraction_net`` proposes for the row (``ocrl_fqf_fractions``, then ``ocrl_fqf_act``), ``deterministic`` or not, and ``n_act_samples``
    is not read.  ``head_kind`` names the head that was built ("dqn", "c51", "qr", "iqn" or "fqf"); ``DQN.train_step`` picks its step by it."""

    def __init__(self, observation_space, action_space, lr_schedule=None, config=None, features_extractor=None, features_extractor_class=None,
                 features_extractor_kwargs=None, net_arch=(64, 64), activation="relu", n_atoms=1, v_min=0.0, v_max=2.0, dueling=False, noisy=False,
                 noisy_sigma0=0.5, n_quantiles=0, n_tau_samples=0, n_act_samples=32, n_cos=64, fqf=False, **kwargs):
        super().__init__()
        self._config = config
        self.observation_space, self.action_space = observation_space, action_space
        n = _n_actions(action_space)                          # Discrete only, with the actor-critic policy's message
        if features_extractor is None and features_extractor_class is not None:
            features_extractor = features_extractor_class(observation_space, **(features_extractor_kwargs or {}))
        if features_extractor is None:
            features_extractor = nn.Flatten()
            self.features_dim = int(math.prod(observation_space.shape))
        else:
            self.features_dim = int(features_extractor.features_dim)
        self.features_extractor = features_extractor
        self.n_atoms, self.dueling, self.n_quantiles = int(n_atoms), bool(dueling), int(n_quantiles)
        self.noisy, self.noisy_sigma0 = bool(noisy), float(noisy_sigma0)
        if not self.noisy_sigma0 >= 0.0:
            raise ValueError(f"{_WHO}.DQNPolicy: noisy_sigma0 >= 0 (got {noisy_sigma0})")
        noise = dict(noisy=True, noisy_sigma0=self.noisy_sigma0) if self.noisy else {}
        self.n_tau_samples, self.n_act_samples, self.n_cos = int(n_tau_samples), int(n_act_samples), int(n_cos)
        self.fqf = bool(fqf)
        if self.fqf:
            _check_fqf(f"{_WHO}.DQNPolicy", self.n_tau_samples, self.n_tau_samples, False, self.dueling, self.n_atoms, self.n_quantiles)
            self.head_kind = "fqf"
            self.q_net = FullyParameterizedQuantileQNetwork(self.features_dim, n, self.n_tau_samples, self.n_cos, net_arch, activation, **noise)
        elif self.n_tau_samples != 0:
            if self.n_tau_samples < 0 or self.n_atoms != 1 or self.n_quantiles != 0:
                raise ValueError(f"{_WHO}.DQNPolicy: n_tau_samples >= 1 (the implicit quantile head) goes with n_atoms = 1 and n_quantiles = 0: "
                                 f"one return distribution at a time (got n_tau_samples {n_tau_samples}, n_atoms {n_atoms}, n_quantiles "
                                 f"{n_quantiles})")
            if self.dueling:
                raise ValueError(f"{_WHO}.DQNPolicy: dueling is not built for the implicit quantile head (got dueling=True with n_tau_samples "
                                 f"{n_tau_samples})")
            self.head_kind = "iqn"
            self.q_net = ImplicitQuantileQNetwork(self.features_dim, n, self.n_cos, self.n_act_samples, net_arch, activation, **noise)
        elif self.n_quantiles != 0:
            if self.n_quantiles < 0 or self.n_atoms != 1:
                raise ValueError(f"{_WHO}.DQNPolicy: n_quantiles >= 1 (the quantile head) goes with n_atoms = 1: one return distribution at a "
                                 f"time (got n_quantiles {n_quantiles}, n_atoms {n_atoms})")
            self.head_kind = "qr"
            self.q_net = QuantileQNetwork(self.features_dim, n, self.n_quantiles, net_arch, activation, self.dueling, **noise)
        elif self.n_atoms >= 2:
            self.head_kind = "c51"
            self.q_net = CategoricalQNetwork(self.features_dim, n, self.n_atoms, v_min, v_max, net_arch, activation, self.dueling, **noise)
        elif self.n_atoms == 1 and not self.dueling:
            self.head_kind = "dqn"
            self.q_net = QNetwork(self.features_dim, n, net_arch, activation, **noise)
        else:
            raise ValueError(f"{_WHO}.DQNPolicy: n_atoms is 1 (the scalar head) or >= 2 (the categorical head), and dueling is built for the "
                             f"categorical head only (got n_atoms {n_atoms}, dueling {dueling})")
        self.exploration_rate = 0.0

    def extract_features(self, obs):
        return self.features_extractor(obs)

    def q_values(self, obs):
        """q [B, n] of an observation batch, attached to autograd"""
        return self.q_net(self.extract_features(obs))

    _sample_seed = None                                       # set_sampling(): the stream of the exploration coin and the random action
    _sample_rows = 0

    def set_sampling(self, seed):
        """give the policy its exploration stream: row r of the n-th ``act`` call draws from (seed, rows of the earlier calls + r)"""
        self._sample_seed = None if seed is None else int(seed) & (2 ** 64 - 1)
        self._sample_rows = 0

    def set_noise(self, draw):
        """choose the noisy head's parameters for the calls that follow: the integer ``draw`` names that draw of the policy's noise
        stream (seeded by ``set_sampling``), ``None`` the mean weights (nothing is launched for them).  Without ``noisy`` there is
        nothing to choose and the call changes nothing."""
        if not self.noisy:
            return
        if draw is not None and self._sample_seed is None:
            raise RuntimeError(f"{_WHO}.DQNPolicy.set_noise: no noise stream: call policy.set_sampling(seed) first")
        self.q_net._noise = None if draw is None else (self._sample_seed, int(draw))

    def act(self, features, row_offset=None, deterministic: bool = False, uniforms=None, epsilon=None):
        """(actions int64 [B], q [B, n], None) of a feature batch in one kernel launch, detached (the collection step; the rule is
        include/ocrl_hip_dqn.h's).  Each row flips its own coin: with probability ``epsilon`` (``None``: ``exploration_rate``;
        ``deterministic``: 0) a uniform random action, otherwise the lowest index of the maximum Q.  Row r draws from (the set_sampling
        seed, row_offset + r); ``row_offset=None`` takes and advances the policy's own row counter.  ``uniforms`` [B, 2] in [0, 1)
        replaces the draw.  A noisy head acts on the draw ``set_noise`` chose, and on the mean weights when ``deterministic``."""
        if deterministic and self.noisy and self.q_net._noise is not None:
            chosen, self.q_net._noise = self.q_net._noise, None
            try:
                return self.act(features, row_offset, True, uniforms, epsilon)
            finally:
                self.q_net._noise = chosen
        x = _bridge.gpu_input(_WHO, features.detach())
        B = x.shape[0]
        eps = 0.0 if deterministic else float(self.exploration_rate if epsilon is None else epsilon)
        if uniforms is not None:
            uniforms = uniforms.to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
            if uniforms.numel() != 2 * B:
                raise ValueError(f"{_WHO}.DQNPolicy.act: {uniforms.numel()} uniforms for a batch of {B} (two per row)")
        elif eps > 0 and self._sample_seed is None:
            raise RuntimeError(f"{_WHO}.DQNPolicy.act: no exploration stream: call policy.set_sampling(seed) or pass uniforms")
        if row_offset is None:
            row_offset = self._sample_rows
            self._sample_rows += B
        sampled = {}
        if self.head_kind == "iqn":                               # the one head that draws fractions of its own (fqf's are proposed)
            if not deterministic and self._sample_seed is None:
                raise RuntimeError(f"{_WHO}.DQNPolicy.act: no stream for the sampled fractions: call policy.set_sampling(seed) or act "
                                   "deterministically (the midpoint fractions)")
            sampled = dict(deterministic=deterministic)
        return (*self.q_net.act(x, self._sample_seed or 0, row_offset, eps, uniforms, **sampled), None)

    def forward(self, obs, deterministic: bool = False):
        return self.act(self.extract_features(obs), deterministic=deterministic)


def dqn_loss(policy, features, next_q, actions, rewards, dones, gamma, next_q_online=None, discounts=None, weights=None, return_abs_td=False):
    """DQN's loss of ``policy`` on a feature batch [B, F] (``policy.extract_features(obs)``) against the target network's
    ``next_q`` [B, n]: (loss, metrics).  ``loss`` is the mean Huber loss of Q[a] - (r + gamma max next_q, or r where done), attached to
    autograd: ``backward()`` puts the gradients on the head's parameters and on ``features``.  ``metrics`` maps DQN_SCALARS to detached 0-d
    tensors.

    The extensions (ocrl_dqn_td_fwd_bwd_ext; with none of them set the call is ocrl_dqn_td_fwd_bwd's, as before): ``next_q_online`` [B, n]
    chooses the action whose ``next_q`` bootstraps (double Q-learning), ``discounts`` [B] replaces ``gamma`` per row (gamma^m of an n-step
    return), ``weights`` [B] scales each row's loss and gradient (importance weights), and ``return_abs_td`` adds the rows' |Q[a] - y|
    [B], detached, as a third result."""
    dims, acts = policy.q_net._layout()
    loss, scal, abs_td = _DqnTdFn.apply(features, next_q, next_q_online, actions, rewards, dones, discounts, weights, gamma, bool(return_abs_td),
                                        dims, acts, policy.q_net.n_actions, *policy.q_net._param_list())
    metrics = {k: scal[i] for i, k in enumerate(DQN_SCALARS)}
    return (loss, metrics, abs_td) if return_abs_td else (loss, metrics)


def _check_fqf(who, n_tau_samples, n_tau_prime_samples, munchausen, dueling, n_atoms, n_quantiles):
    """what fqf=True refuses, each by the names of both arguments"""
    if n_tau_samples == 0:
        raise ValueError(f"{who}: fqf=True proposes n_tau_samples fractions per state: set n_tau_samples in 2 .. {MAX_FRACTIONS} (got fqf=True "
                         "with n_tau_samples = 0)")
    if not 2 <= n_tau_samples <= MAX_FRACTIONS:
        raise ValueError(f"{who}: fqf=True takes n_tau_samples in 2 .. {MAX_FRACTIONS}: the 2 n - 1 fractions of the fraction loss go through "
                         f"the head in one pass (got fqf=True with n_tau_samples = {n_tau_samples})")
    if n_tau_prime_samples not in (0, n_tau_samples):
        raise ValueError(f"{who}: fqf=True evaluates the target network at the online network's own fractions: n_tau_prime_samples is 0 or "
                         f"n_tau_samples (got fqf=True with n_tau_prime_samples = {n_tau_prime_samples}, n_tau_samples = {n_tau_samples})")
    if munchausen:
        raise ValueError(f"{who}: fqf with munchausen=True is not built (got fqf=True with munchausen=True)")
    if dueling:
        raise ValueError(f"{who}: fqf with dueling=True is not built: the implicit quantile head has no value stream (got fqf=True with "
                         "dueling=True)")
    if n_atoms > 1 or n_quantiles > 0:
        raise ValueError(f"{who}: fqf=True with n_atoms > 1 or n_quantiles > 0 names two return distributions: one at a time (got fqf=True "
                         f"with n_atoms = {n_atoms}, n_quantiles = {n_quantiles})")


def exploration_schedule(frac, initial_eps, final_eps, fraction):
    """epsilon at the share ``frac`` of the run: linear from ``initial_eps`` to ``final_eps`` over the first ``fraction``, then constant"""
    if frac > fraction:
        return float(final_eps)
    return float(initial_eps + frac * (final_eps - initial_eps) / fraction)


def _layout(params):
    """(offsets, length) of a flat buffer over ``params``: each starts on a multiple of 4 floats (OnPolicyAlgorithm._flatten_parameters)"""
    offs, n = [], 0
    for p in params:
        offs.append(n)
        n += (p.numel() + 3) & ~3
    return offs, max(n, 4)


class DQN:
    """Deep Q-learning with a target network and a replay buffer for Discrete actions (stable-baselines3's DQN on a VecEnv).  ``env`` as
    OnPolicyAlgorithm takes it; ``policy`` is a DQNPolicy or its class.  An iteration is ``train_freq`` vec steps, then
    ``gradient_steps`` updates once ``num_timesteps > learning_starts``.  Every environment flips its own exploration coin.

    ``noisy=True``: the head is built of noisy layers and epsilon is 0 at every step, warm-up included; the three
    ``exploration_*`` arguments are accepted and unused.  ``noise_draws`` counts the draws handed out: one per ``collect_step``, shared by
    all its rows, and two per ``train_step``, the first for the online network (its forward on the observations and, under ``double_q``,
    its evaluation of the next observations share it), the second for the target network.  The online network's noise stream is seeded
    with ``seed``, the target network's with ``seed + 1``.

    ``n_quantiles >= 1``: the head learns ``n_quantiles`` quantile values per action with the quantile Huber loss at
    ``huber_kappa`` (``_train_step_qr``); it takes ``n_atoms = 1`` and combines with every other argument here.

    ``n_tau_samples >= 1``: the implicit quantile head (IQN).  An update evaluates the online network at ``n_tau_samples``
    (N) sampled fractions per row and the target network at ``n_tau_prime_samples`` (N'; 0: N), acting takes ``n_act_samples`` (K),
    the embedding has ``n_cos`` cosines and the loss is the quantile Huber loss at ``huber_kappa`` (``_train_step_iqn``).  It takes
    ``n_atoms = 1``, ``n_quantiles = 0`` and no ``dueling`` and combines with double Q, n-step returns, prioritized replay and ``noisy``.

    ``munchausen=True``: Munchausen targets on the scalar, quantile and implicit quantile heads.  An update evaluates
    the target network on the observations as well (one pass of 2 ``batch_size`` rows), ``munchausen_targets`` adds ``munchausen_alpha``
    times the log-policy of the action taken, scaled by ``munchausen_tau`` and clipped to [``munchausen_clip``, 0], to the rewards and
    puts the soft value of the soft-max policy at temperature ``munchausen_tau`` in place of the target network's values at the next
    observations; the head's TD step then runs unchanged.  It takes ``n_atoms = 1`` and no ``double_q`` and combines with n-step
    returns (the bonus is the first action's), prioritized replay, ``noisy`` and ``dueling`` on the quantile head; acting is unchanged.

    ``fqf=True``: FQF on the implicit quantile head.  ``n_tau_samples`` (N, 2 .. 32) fractions per row are proposed by the
    online network's ``fraction_net`` from the observation's features; an update evaluates both networks at them
    (``_train_step_fqf``), q is the interval-weighted sum, and the proposal takes the fraction loss's gradient
    (``fqf_fraction_loss``, with ``fqf_ent_coef`` times the proposal's entropy) and a TF-style RMSprop step of its own at
    ``fqf_fraction_lr`` on buffers outside ``flat_p`` (``frac_p``, ``frac_g``, ``frac_sq``).  ``n_tau_prime_samples`` is 0 or N,
    ``n_act_samples`` is not read; it refuses ``munchausen``, ``dueling`` and a second distributional head and combines with double Q,
    n-step returns, prioritized replay and ``noisy``."""
    ALGO = "DQN"
    HYPER = ("learning_rate", "buffer_size", "learning_starts", "batch_size", "tau", "gamma", "train_freq", "gradient_steps",
             "target_update_interval", "exploration_fraction", "exploration_initial_eps", "exploration_final_eps", "max_grad_norm",
             "double_q", "n_step", "prioritized_replay", "prioritized_replay_alpha", "prioritized_replay_beta0", "prioritized_replay_beta_final",
             "prioritized_replay_eps", "n_atoms", "v_min", "v_max", "dueling", "noisy", "noisy_sigma0", "n_quantiles", "huber_kappa",
             "n_tau_samples", "n_tau_prime_samples", "n_act_samples", "n_cos", "munchausen", "munchausen_alpha", "munchausen_tau", "munchausen_clip",
             "fqf", "fqf_fraction_lr", "fqf_ent_coef")

    def __init__(self, policy, env, learning_rate=1e-4, buffer_size=1_000_000, learning_starts=50_000, batch_size=32, tau=1.0, gamma=0.99,
                 train_freq=4, gradient_steps=1, target_update_interval=10_000, exploration_fraction=0.1, exploration_initial_eps=1.0,
                 exploration_final_eps=0.05, max_grad_norm=10, seed=0, device="cuda", policy_kwargs=None, log_interval=100, double_q=False, n_step=1,
                 prioritized_replay=False, prioritized_replay_alpha=0.6, prioritized_replay_beta0=0.4, prioritized_replay_beta_final=1.0,
                 prioritized_replay_eps=1e-6, n_atoms=1, v_min=0.0, v_max=2.0, dueling=False, noisy=False, noisy_sigma0=0.5,
                 n_quantiles=0, huber_kappa=1.0, n_tau_samples=0, n_tau_prime_samples=0, n_act_samples=32, n_cos=64, munchausen=False,
                 munchausen_alpha=0.9, munchausen_tau=0.03, munchausen_clip=-1.0, fqf=False, fqf_fraction_lr=2.5e-9, fqf_ent_coef=0.0,
                 **ignored_sb3_kwargs):
        who = self._who = f"{_WHO}.{self.ALGO}"
        self.learning_rate = _check_constant(who, "learning_rate", learning_rate)
        if int(gradient_steps) < 1:
            raise ValueError(f"{who}: gradient_steps >= 1 (got {gradient_steps}; stable-baselines3's -1, as many as steps were collected, is not built)")
        if int(train_freq) < 1 or int(batch_size) < 1 or int(log_interval) < 1:
            raise ValueError(f"{who}: train_freq, batch_size and log_interval >= 1 (got {train_freq}, {batch_size}, {log_interval})")
        if not 0.0 < float(exploration_fraction) <= 1.0:
            raise ValueError(f"{who}: 0 < exploration_fraction <= 1 (got {exploration_fraction})")
        self.n_actions = _n_actions(env.action_space)                 # Discrete only: the policy's own message otherwise
        self.env, self.n_envs = env, int(env.num_envs)
        self.double_q, self.n_step, self.prioritized_replay = bool(double_q), int(n_step), bool(prioritized_replay)
        slots = max(2, int(buffer_size) // self.n_envs)
        if not 1 <= self.n_step <= MAX_N_STEP or self.n_step >= slots:
            raise ValueError(f"{who}: n_step must lie in 1 .. {MAX_N_STEP} and below the replay ring's {slots} slots (got {n_step})")
        for name, v in (("prioritized_replay_alpha", prioritized_replay_alpha), ("prioritized_replay_beta0", prioritized_replay_beta0),
                        ("prioritized_replay_beta_final", prioritized_replay_beta_final)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"{who}: 0 <= {name} <= 1 (got {v})")
        if not float(prioritized_replay_eps) >= 0.0:
            raise ValueError(f"{who}: prioritized_replay_eps >= 0 (got {prioritized_replay_eps})")
        self.prioritized_replay_alpha, self.prioritized_replay_eps = float(prioritized_replay_alpha), float(prioritized_replay_eps)
        self.prioritized_replay_beta0, self.prioritized_replay_beta_final = float(prioritized_replay_beta0), float(prioritized_replay_beta_final)
        self.n_atoms, self.v_min, self.v_max, self.dueling = int(n_atoms), float(v_min), float(v_max), bool(dueling)
        if self.n_atoms != 1 and not 2 <= self.n_atoms <= MAX_ATOMS:
            raise ValueError(f"{who}: n_atoms is 1 (the scalar head) or lies in 2 .. {MAX_ATOMS} (got {n_atoms})")
        if self.n_atoms > 1 and self.n_actions * self.n_atoms > MAX_LOGITS:
            raise ValueError(f"{who}: n_actions * n_atoms <= {MAX_LOGITS} (got {self.n_actions} actions and n_atoms = {n_atoms})")
        if self.n_atoms > 1 and not self.v_min < self.v_max:
            raise ValueError(f"{who}: v_min < v_max (got {v_min}, {v_max})")
        self.n_quantiles, self.huber_kappa = int(n_quantiles), float(huber_kappa)
        if not 0 <= self.n_quantiles <= MAX_QUANTILES:
            raise ValueError(f"{who}: n_quantiles is 0 (off) or lies in 1 .. {MAX_QUANTILES} (got {n_quantiles})")
        if self.n_actions * self.n_quantiles > MAX_QUANTILE_COLS:
            raise ValueError(f"{who}: n_actions * n_quantiles <= {MAX_QUANTILE_COLS} (got {self.n_actions} actions and n_quantiles = {n_quantiles})")
        if not (self.huber_kappa > 0.0 and math.isfinite(self.huber_kappa)):
            raise ValueError(f"{who}: huber_kappa > 0 and finite (got {huber_kappa})")
        if self.n_quantiles > 0 and self.n_atoms > 1:
            raise ValueError(f"{who}: n_quantiles > 0 and n_atoms > 1 name two return distributions: one at a time (got n_quantiles = "
                             f"{n_quantiles}, n_atoms = {n_atoms})")
        self.n_tau_samples, self.n_tau_prime_samples = int(n_tau_samples), int(n_tau_prime_samples)
        self.n_act_samples, self.n_cos = int(n_act_samples), int(n_cos)
        if not 0 <= self.n_tau_samples <= MAX_TAU_SAMPLES:
            raise ValueError(f"{who}: n_tau_samples is 0 (off) or lies in 1 .. {MAX_TAU_SAMPLES} (got {n_tau_samples})")
        if not 0 <= self.n_tau_prime_samples <= MAX_TAU_SAMPLES:
            raise ValueError(f"{who}: n_tau_prime_samples is 0 (as n_tau_samples) or lies in 1 .. {MAX_TAU_SAMPLES} (got {n_tau_prime_samples})")
        if not 1 <= self.n_act_samples <= MAX_TAU_SAMPLES:
            raise ValueError(f"{who}: n_act_samples lies in 1 .. {MAX_TAU_SAMPLES} (got {n_act_samples})")
        if not (4 <= self.n_cos <= MAX_COS and self.n_cos % 4 == 0):
            raise ValueError(f"{who}: n_cos is a multiple of 4 in 4 .. {MAX_COS} (got {n_cos})")
        if bool(fqf):
            _check_fqf(who, self.n_tau_samples, self.n_tau_prime_samples, bool(munchausen), self.dueling, self.n_atoms, self.n_quantiles)
        if self.n_tau_samples > 0 and (self.n_atoms > 1 or self.n_quantiles > 0):
            raise ValueError(f"{who}: n_tau_samples > 0 with n_atoms > 1 or n_quantiles > 0 names two return distributions: one at a time (got "
                             f"n_tau_samples = {n_tau_samples}, n_atoms = {n_atoms}, n_quantiles = {n_quantiles})")
        if self.n_tau_samples > 0 and self.dueling:
            raise ValueError(f"{who}: dueling is not built for the implicit quantile head: n_tau_samples = {n_tau_samples} takes dueling = False "
                             "(got dueling=True)")
        if self.dueling and self.n_atoms == 1 and self.n_quantiles == 0:
            raise ValueError(f"{who}: dueling is built for the categorical head only: set n_atoms >= 2 (got dueling=True with n_atoms=1)")
        self.noisy, self.noisy_sigma0 = bool(noisy), float(noisy_sigma0)
        if not self.noisy_sigma0 >= 0.0:
            raise ValueError(f"{who}: noisy_sigma0 >= 0 (got {noisy_sigma0})")
        self.munchausen = bool(munchausen)
        self.munchausen_alpha, self.munchausen_tau, self.munchausen_clip = float(munchausen_alpha), float(munchausen_tau), float(munchausen_clip)
        check_munchausen(who, munchausen_alpha, munchausen_tau, munchausen_clip)
        if self.munchausen and self.n_atoms > 1:
            raise ValueError(f"{who}: munchausen with n_atoms > 1: the categorical projection of a policy mixture is not built (got "
                             f"munchausen=True with n_atoms = {n_atoms})")
        if self.munchausen and self.double_q:
            raise ValueError(f"{who}: munchausen with double_q=True: the soft value of the target network's policy leaves no bootstrap action "
                             "to pick (got munchausen=True with double_q=True)")
        self.fqf, self.fqf_fraction_lr, self.fqf_ent_coef = bool(fqf), float(fqf_fraction_lr), float(fqf_ent_coef)
        if not (math.isfinite(self.fqf_fraction_lr) and self.fqf_fraction_lr >= 0.0):
            raise ValueError(f"{who}: fqf_fraction_lr >= 0 and finite (got {fqf_fraction_lr})")
        if not math.isfinite(self.fqf_ent_coef):
            raise ValueError(f"{who}: fqf_ent_coef finite (got {fqf_ent_coef})")
        self.buffer_size, self.learning_starts, self.batch_size = int(buffer_size), int(learning_starts), int(batch_size)
        self.tau, self.gamma = float(tau), float(gamma)
        self.train_freq, self.gradient_steps, self.target_update_interval = int(train_freq), int(gradient_steps), int(target_update_interval)
        self.exploration_fraction = float(exploration_fraction)
        self.exploration_initial_eps, self.exploration_final_eps = float(exploration_initial_eps), float(exploration_final_eps)
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.seed, self.log_interval = int(seed), int(log_interval)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if isinstance(policy, type):
            torch.manual_seed(self.seed)                              # the initialisation follows the seed, as set_random_seed does
            head = dict(n_atoms=self.n_atoms, v_min=self.v_min, v_max=self.v_max, dueling=self.dueling) if self.n_atoms > 1 else {}
            if self.n_quantiles > 0:
                head = dict(n_quantiles=self.n_quantiles, dueling=self.dueling)
            if self.n_tau_samples > 0:
                head = dict(n_tau_samples=self.n_tau_samples, n_act_samples=self.n_act_samples, n_cos=self.n_cos)
            if self.fqf:
                head["fqf"] = True
            if self.noisy:
                head.update(noisy=True, noisy_sigma0=self.noisy_sigma0)
            policy = policy(env.observation_space, env.action_space, None, **dict(policy_kwargs or {}, **head))
        if not isinstance(policy, DQNPolicy):
            raise TypeError(f"{who}: policy must be an ocrl_amd.sb3s.DQNPolicy (or the class), got {type(policy).__name__}")
        if (policy.n_atoms, policy.dueling) != (self.n_atoms, self.dueling):
            raise ValueError(f"{who}: the policy's head has n_atoms = {policy.n_atoms}, dueling = {policy.dueling}; the arguments say n_atoms = "
                             f"{self.n_atoms}, dueling = {self.dueling}")
        if policy.n_quantiles != self.n_quantiles:
            raise ValueError(f"{who}: the policy's head has n_quantiles = {policy.n_quantiles}; the arguments say n_quantiles = {self.n_quantiles}")
        if bool(policy.n_tau_samples) != bool(self.n_tau_samples) or (self.n_tau_samples and (policy.n_act_samples, policy.n_cos) != (
                self.n_act_samples, self.n_cos)):
            raise ValueError(f"{who}: the policy's head has n_tau_samples = {policy.n_tau_samples}, n_act_samples = {policy.n_act_samples}, n_cos = "
                             f"{policy.n_cos}; the arguments say n_tau_samples = {self.n_tau_samples}, n_act_samples = {self.n_act_samples}, n_cos = "
                             f"{self.n_cos}")
        if self.n_atoms > 1 and (policy.q_net.v_min, policy.q_net.v_max) != (self.v_min, self.v_max):
            raise ValueError(f"{who}: the policy's head has v_min, v_max = {policy.q_net.v_min}, {policy.q_net.v_max}; the arguments say "
                             f"{self.v_min}, {self.v_max}")
        if getattr(policy, "fqf", False) != self.fqf or (self.fqf and policy.n_tau_samples != self.n_tau_samples):
            raise ValueError(f"{who}: the policy's head has fqf = {getattr(policy, 'fqf', False)}, n_tau_samples = {policy.n_tau_samples}; the "
                             f"arguments say fqf = {self.fqf}, n_tau_samples = {self.n_tau_samples}")
        if policy.noisy != self.noisy:
            raise ValueError(f"{who}: the policy's head has noisy = {policy.noisy}; the arguments say noisy = {self.noisy}")
        for m in policy.modules():
            if isinstance(m, FlatParamModule):
                raise NotImplementedError(f"{who}: a trainable {m.backend} encoder behind the extractor keeps its own flat buffers and optimiser "
                                          f"step; stepping it from {self.ALGO} is not built: give the extractor a pre-trained, frozen encoder")
        self.policy = policy.to(self.device)
        self.policy.set_sampling(self.seed)
        self.policy.exploration_rate = 0.0 if self.noisy else self.exploration_initial_eps
        self._flatten_parameters()
        self.noise_draws = 0                                          # noisy: the draws handed out so far
        if self.noisy:
            self.target.set_sampling(self.seed + 1)                   # the target network's noise stream is its own
        self.num_timesteps, self.iteration, self.n_calls, self.n_updates, self.n_target_updates = 0, 0, 0, 0, 0
        self._total_timesteps = 0
        self._obs_shape = tuple(env.observation_space.shape)
        self.replay_buffer = None
        self.last_weights = None                                      # the importance weights [batch_size] of the last prioritized update
        self._last_obs = None
        self._ep_ret, self._ep_len = np.zeros(self.n_envs), np.zeros(self.n_envs, dtype=np.int64)
        self._episodes = collections.deque(maxlen=100)
        self._successes = collections.deque(maxlen=100)
        # what the callbacks report: sums of DQN_SCALARS and the gradient norm over the updates since the last one, and the finished
        # episodes of the vec steps since then (done, success, return, length per step), all on the device until the callback reads them
        self._acc, self._acc_n = torch.zeros(len(DQN_SCALARS) + 1, device=self.device), 0
        self._stats = torch.zeros(self.log_interval * self.train_freq, 4, self.n_envs, device=self.device, dtype=torch.float64)
        self._stats_n = 0
        self._last_train = self._train_stats([float("nan")] * (len(DQN_SCALARS) + 1), 1)
        if self.fqf:
            self._last_train.update(dict.fromkeys(FQF_SCALARS, float("nan")))

    n_steps = property(lambda self: self.train_freq)                  # vec steps per iteration (what the entry point's log line prints)
    exploration_rate = property(lambda self: self.policy.exploration_rate)

    # ---- the optimiser's view of the two policies: flat_p / flat_g / Adam's moments for the online one, flat_target for the target
    def _flatten_parameters(self):
        """re-seat every trainable parameter as a view of ``flat_p`` and its .grad as a view of ``flat_g``, in the layout of
        OnPolicyAlgorithm._flatten_parameters; then build the target policy, a copy whose trainable parameters are views of
        ``flat_target`` in the same layout and take no gradient.  What has no trainable parameter and is no nn.Module (a frozen encoder's
        wrapper) is shared between the two, not copied."""
        frac = list(self.policy.q_net.fraction_net.parameters()) if self.fqf else []      # fqf: stepped by an optimiser of its own
        params = [p for p in self.policy.parameters() if p.requires_grad and not any(p is f for f in frac)]
        for p in params + frac:
            if p.dtype != torch.float32 or p.device != self.device:
                raise RuntimeError(f"{self._who}: parameters must be float32 on {self.device} (got {p.dtype} on {p.device})")
        offs, n = _layout(params)
        self.flat_p, self.flat_g, self.flat_target = (torch.zeros(n, device=self.device) for _ in range(3))
        for p, o in zip(params, offs):
            view = self.flat_p[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = self.flat_g[o:o + p.numel()].view(p.shape)
        self._params = params
        if self.fqf:
            foffs, fn = _layout(frac)
            self.frac_p, self.frac_g = (torch.zeros(fn, device=self.device) for _ in range(2))
            self.frac_sq = torch.ones(fn, device=self.device)         # TF-style RMSprop starts its square average at ones
            for p, o in zip(frac, foffs):
                view = self.frac_p[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
        ext = self.policy.features_extractor
        frozen = getattr(ext, "_ocr", None)
        memo = {id(frozen): frozen} if frozen is not None and not getattr(ext, "_trainable", True) else {}
        memo[id(self.policy._config)] = self.policy._config
        for p in params:                                              # the copy must not drag flat_g along
            p.grad = None
        self.target = copy.deepcopy(self.policy, memo)
        for p, o in zip(params, offs):
            p.grad = self.flat_g[o:o + p.numel()].view(p.shape)
        if self.fqf:
            for p, o in zip(frac, foffs):
                p.grad = self.frac_g[o:o + p.numel()].view(p.shape)
            for p in self.target.q_net.fraction_net.parameters():     # a frozen copy, which nothing reads
                p.requires_grad_(False)
            self._frac_norm = torch.zeros(1, device=self.device)
            self._frac_ws = torch.empty(_lib.lib().ocrl_flat_clip_rmsprop_ws_floats(), device=self.device)
            self._frac_acc = torch.zeros(len(FQF_SCALARS), device=self.device)
        tparams = [p for p in self.target.parameters() if p.requires_grad]
        assert [tuple(p.shape) for p in tparams] == [tuple(p.shape) for p in params]
        for p, o in zip(tparams, offs):
            p.data = self.flat_target[o:o + p.numel()].view(p.shape)
            p.requires_grad_(False)
        self.flat_target.copy_(self.flat_p)
        self.target.eval()
        self._norm = torch.zeros(1, device=self.device)
        self.flat_m, self.flat_v = (torch.zeros_like(self.flat_p) for _ in range(2))
        self.adam_step = 0
        self._ws = torch.empty(_lib.lib().ocrl_flat_clip_adam_ws_floats(), device=self.device)

    def _adam_step(self):
        """L2 clip of the whole gradient to max_grad_norm, then Adam (eps 1e-8): one C call, no host synchronisation"""
        self.adam_step += 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ocrl_flat_clip_adam_l2(_lib.ptr(self.flat_p), _lib.ptr(self.flat_g), _lib.ptr(self.flat_m), _lib.ptr(self.flat_v),
                                                         self.flat_p.numel(), self.max_grad_norm, self.learning_rate, 0.9, 0.999, ADAM_EPS,
                                                         self.adam_step, _lib.ptr(self._norm), _lib.ptr(self._ws), self._ws.numel(),
                                                         _lib.stream(self.device)))

    def _fraction_step(self):
        """fqf: the proposal's own step, the library's TF-style RMSprop (epsilon inside the root, square average from ones) without a
        clip, at fqf_fraction_lr: one C call, no host synchronisation"""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ocrl_flat_clip_rmsprop_l2(_lib.ptr(self.frac_p), _lib.ptr(self.frac_g), _lib.ptr(self.frac_sq), self.frac_p.numel(),
                                                            0.0, self.fqf_fraction_lr, FQF_RMS_ALPHA, FQF_RMS_EPS, _lib.ptr(self._frac_norm),
                                                            _lib.ptr(self._frac_ws), self._frac_ws.numel(), _lib.stream(self.device)))

    def update_target(self):
        """the target network follows the online one: a copy at tau = 1 (DQN's hard update), else a step of size tau towards it"""
        if self.tau == 1.0:
            self.flat_target.copy_(self.flat_p)
        else:
            self.flat_target.lerp_(self.flat_p, self.tau)
        self.n_target_updates += 1

    _obs = OnPolicyAlgorithm._obs                                     # uint8 frames become floats in [0, 1] on the device
    ep_rew_mean, ep_len_mean, success_rate = OnPolicyAlgorithm.ep_rew_mean, OnPolicyAlgorithm.ep_len_mean, OnPolicyAlgorithm.success_rate
    _track_episodes = OnPolicyAlgorithm._track_episodes
    predict = OnPolicyAlgorithm.predict                               # epsilon-greedy at the current exploration_rate unless deterministic

    # ---- collection
    def epsilon(self):
        """the exploration rate of the next step: 1 while the buffer warms up, then the schedule of num_timesteps / total_timesteps"""
        if self.noisy:                                                # the noise explores: no coin, the warm-up included
            self.policy.exploration_rate = 0.0
            return 0.0
        frac = self.num_timesteps / max(self._total_timesteps, 1)
        rate = exploration_schedule(frac, self.exploration_initial_eps, self.exploration_final_eps, self.exploration_fraction)
        self.policy.exploration_rate = rate
        return 1.0 if self.num_timesteps < self.learning_starts else rate

    def collect_step(self):
        """one step of every environment into the replay buffer.  An environment with ``on_device`` set (ocrl_amd.envs) is stepped
        through ``step_device`` and nothing is read from the device."""
        E = self.n_envs
        on_device = getattr(self.env, "on_device", False)
        if self._last_obs is None:
            self._last_obs = _tensor(self.env.reset(), self.device)
            self._ep_ret[:], self._ep_len[:] = 0.0, 0
        if self.replay_buffer is None:
            self.replay_buffer = ReplayBuffer(self.buffer_size, E, self._obs_shape, self.device, self._last_obs.dtype, self.seed,
                                              prioritized=self.prioritized_replay, n_step=self.n_step)
        self.policy.eval()
        with torch.no_grad():
            eps = self.epsilon()
            if self.noisy:                                            # one fresh draw, shared by all rows of the step
                self.policy.set_noise(self.noise_draws)
                self.noise_draws += 1
            actions, _, _ = self.policy.act(self.policy.extract_features(self._obs(self._last_obs)), epsilon=eps)
            if on_device:
                new_obs, rewards, dones, extras = self.env.step_device(actions)
                k = self._stats_n
                self._stats[k, 0], self._stats[k, 1], self._stats[k, 2], self._stats[k, 3] = (dones, extras["is_success"], extras["episode_return"],
                                                                                              extras["episode_length"])
                self._stats_n += 1
            else:
                new_obs, rewards, dones, _ = self.env.step(actions.cpu().numpy())
                rewards = np.asarray(rewards.cpu() if isinstance(rewards, torch.Tensor) else rewards, dtype=np.float64).reshape(E)
                dones = np.asarray(dones.cpu() if isinstance(dones, torch.Tensor) else dones).reshape(E).astype(bool)
                self._track_episodes(rewards, dones)
                rewards = torch.as_tensor(rewards, dtype=torch.float32)
            new_obs = _tensor(new_obs, self.device)
            self.replay_buffer.add(self._last_obs, new_obs, actions, rewards, dones)
            self._last_obs = new_obs
        self.num_timesteps += E
        self.n_calls += 1
        if self.n_calls % max(self.target_update_interval // E, 1) == 0:
            self.update_target()
        if self._stats_n == self._stats.shape[0]:
            self._read_episodes()

    def _read_episodes(self):
        """the finished episodes of the steps since the last read, in (step, environment) order, into the 100-episode windows: one copy"""
        if self._stats_n == 0:
            return
        host = self._stats[:self._stats_n].cpu().numpy()
        self._stats_n = 0
        for t, e in zip(*np.nonzero(host[:, 0])):
            self._episodes.append((float(host[t, 2, e]), int(host[t, 3, e])))
            self._successes.append(bool(host[t, 1, e]))

    # ---- the update
    def beta(self):
        """the importance weights' exponent: linear from prioritized_replay_beta0 to prioritized_replay_beta_final over the current
        ``learn()``'s timesteps, like epsilon"""
        frac = min(self.num_timesteps / max(self._total_timesteps, 1), 1.0)
        return self.prioritized_replay_beta0 + frac * (self.prioritized_replay_beta_final - self.prioritized_replay_beta0)

    def _draw_train_noise(self):
        """noisy: the two fresh draws of a gradient step, one for every use of the online network in it, one for the target network"""
        if self.noisy:
            self.policy.set_noise(self.noise_draws)
            self.target.set_noise(self.noise_draws + 1)
            self.noise_draws += 2

    def _draw_batch(self):
        """(batch, transition ids, importance weights or None) of this update: drawn in proportion to the priorities, among the whole
        n-step windows or uniformly, and read with its n-step returns where n_step > 1.  The draw is a function of (seed, n_updates)."""
        buf = self.replay_buffer
        if (self.prioritized_replay or self.n_step > 1) and len(buf) == 0:
            raise RuntimeError(f"{self._who}.train_step: learning_starts = {self.learning_starts} leaves {buf.pos} vec steps in the replay ring at "
                               f"the first update, fewer than n_step = {self.n_step}: raise learning_starts to at least "
                               f"{self.n_step * self.n_envs} timesteps")
        weights = None
        if self.prioritized_replay:
            idx, weights = buf.sample_prioritized(self.batch_size, self.n_updates, self.beta())
        else:
            idx = buf.sample_indices(self.batch_size, self.n_updates, self.n_step)
        batch = buf.gather(idx, self.n_step, self.gamma) if self.n_step > 1 else buf.gather(idx)
        return batch, idx, weights

    def _online_turn(self):
        """the online network's turn in a gradient step: train mode and a zeroed ``flat_g``.  The steps call it once the target
        network's launches are queued, so that the walk over the policy's modules runs while the GPU works on them."""
        self.policy.train()
        self.flat_g.zero_()

    def _both_obs(self, batch):
        """munchausen: the next observations, then the observations, as one batch of 2 batch_size rows for the target network (a row's
        values do not depend on its position in the batch)"""
        return self._obs(torch.cat([batch.next_observations, batch.observations]))

    def _munchausen(self, batch, q2, quantiles2=None):
        """munchausen: (rewards, next_q, next_quantiles) as the heads' losses take them, from the target network's values q2 [2 B, n]
        (and quantile values [2 B, n, N']) on ``_both_obs``: one ``munchausen_targets`` launch"""
        B = q2.shape[0] // 2
        return munchausen_targets(q2[B:], q2[:B], batch.actions, batch.rewards, batch.dones, self.munchausen_alpha, self.munchausen_tau,
                                  self.munchausen_clip, next_quantiles=None if quantiles2 is None else quantiles2[:B])

    def _target_obs(self, batch):
        """the observations the target network is evaluated on: the next ones, or ``_both_obs`` under munchausen"""
        return self._both_obs(batch) if self.munchausen else self._obs(batch.next_observations)

    def _targets(self, batch, q, quantiles=None):
        """(rewards, next_q, next_quantiles) as the heads' losses take them, from the target network's values on ``_target_obs``:
        rewritten by ``_munchausen``, else the batch's rewards and the values as they are"""
        return self._munchausen(batch, q, quantiles) if self.munchausen else (batch.rewards, q, quantiles)

    def _train_step_dqn(self, batch, weights):
        """the scalar head's part of ``train_step``: (loss, metrics, the rows' |TD error| under prioritized replay).  The target network
        gives the next observations' Q, the online network names the bootstrap action under double_q; with neither that nor n_step > 1
        nor prioritized replay the step is ocrl_dqn_td_fwd_bwd's (``dqn_loss``)."""
        target_obs = self._target_obs(batch)
        with torch.no_grad():
            rewards, next_q, _ = self._targets(batch, self.target.q_values(target_obs))
        self._online_turn()
        next_q_online = None
        if self.double_q:                                             # refused with munchausen: target_obs is the next observations
            with torch.no_grad():
                next_q_online = self.policy.q_values(target_obs)
        features = self.policy.extract_features(self._obs(batch.observations))
        out = dqn_loss(self.policy, features, next_q, batch.actions, rewards, batch.dones, self.gamma, next_q_online=next_q_online,
                       discounts=batch.discounts, weights=weights, return_abs_td=self.prioritized_replay)
        return out if self.prioritized_replay else (*out, None)

    def _train_step_c51(self, batch, weights):
        """the categorical head's part of ``train_step``: (loss, metrics, the rows' cross-entropies, which take the place
        of |TD error| in the priority store).  The target network gives the next observations' distribution, the online network names
        the bootstrap action under double_q, ``c51_loss`` projects."""
        next_obs = self._obs(batch.next_observations)
        with torch.no_grad():
            next_probs, next_q = self.target.q_net.distribution(self.target.extract_features(next_obs))
        self._online_turn()
        if self.double_q:
            with torch.no_grad():
                _, next_q = self.policy.q_net.distribution(self.policy.extract_features(next_obs))
        features = self.policy.extract_features(self._obs(batch.observations))
        return c51_loss(self.policy, features, next_probs, next_q, batch.actions, batch.rewards, batch.dones, self.gamma,
                        discounts=batch.discounts, weights=weights)

    def _train_step_qr(self, batch, weights):
        """the quantile head's part of ``train_step``: (loss, metrics, the rows' quantile losses, which take the place of
        |TD error| in the priority store).  The target network gives the next observations' quantiles, the online network names the
        bootstrap action under double_q, ``qr_loss`` does the rest."""
        target_obs = self._target_obs(batch)
        with torch.no_grad():
            quantiles, q = self.target.q_net.quantiles(self.target.extract_features(target_obs))
            rewards, next_q, next_quantiles = self._targets(batch, q, quantiles)
        self._online_turn()
        if self.double_q:                                             # refused with munchausen: target_obs is the next observations
            with torch.no_grad():
                _, next_q = self.policy.q_net.quantiles(self.policy.extract_features(target_obs))
        features = self.policy.extract_features(self._obs(batch.observations))
        return qr_loss(self.policy, features, next_quantiles, next_q, batch.actions, rewards, batch.dones, self.gamma, self.huber_kappa,
                       discounts=batch.discounts, weights=weights)

    def _train_taus(self, k, n):
        """draw k (0: the online network's N, 1: the target network's N', 2: the online network's N' under double_q, or the target
        network's N' at the observations under munchausen, which refuses double_q) of this update:
        [batch_size, n] fractions of the training stream, rows (3 n_updates + k) batch_size ..., which no acting row shares"""
        return draw_taus(self.seed + TRAIN_SEED_SALT, (3 * self.n_updates + k) * self.batch_size, self.batch_size, n, self.device)

    def _train_step_iqn(self, batch, weights):
        """the implicit quantile head's part of ``train_step``: (loss, metrics, the rows' quantile losses, which take the
        place of |TD error| in the priority store).  The target network gives the next observations' quantile values at N' fractions
        of its own and their mean, the online network names the bootstrap action under double_q from N' fractions of its own, and
        ``iqn_loss`` evaluates the online network at N fractions and does the rest."""
        N, Np = self.n_tau_samples, self.n_tau_prime_samples or self.n_tau_samples
        target_obs = self._target_obs(batch)
        with torch.no_grad():
            target_features = self.target.extract_features(target_obs)
            taus = self._train_taus(1, Np)
            if self.munchausen:                                       # the observations' rows of _both_obs take draw 2
                taus = torch.cat([taus, self._train_taus(2, Np)])
            quantiles, q = self.target.q_net.quantiles(target_features, taus)
            rewards, next_q, next_quantiles = self._targets(batch, q, quantiles)
        self._online_turn()
        if self.double_q:                                             # refused with munchausen: target_obs is the next observations
            with torch.no_grad():
                _, next_q = self.policy.q_net.quantiles(self.policy.extract_features(target_obs), self._train_taus(2, Np))
        features = self.policy.extract_features(self._obs(batch.observations))
        return iqn_loss(self.policy, features, self._train_taus(0, N), next_quantiles, next_q, batch.actions, rewards, batch.dones, self.gamma,
                        self.huber_kappa, discounts=batch.discounts, weights=weights)

    def _train_step_fqf(self, batch, weights):
        """FQF's part of ``train_step``: (loss, metrics, the rows' quantile losses).  Every fraction is the row's own,
        proposed by the online ``fraction_net`` from the online features of the observation (the paper's Algorithm 1): the target
        network gives the next observations' quantile values at those tau_hats and their interval-weighted q (the online network's q
        under double_q), ``iqn_loss`` runs unchanged with N' = N, and one head forward at the 2 N - 1 fractions of eval_taus feeds
        ``fqf_fraction_loss``, which leaves the proposal's gradient in ``frac_g``."""
        self._online_turn()
        features = self.policy.extract_features(self._obs(batch.observations))
        next_obs = self._obs(batch.next_observations)
        with torch.no_grad():
            fr = self.policy.q_net.fractions(features)
            next_quantiles, next_q = self.target.q_net.quantiles(self.target.extract_features(next_obs), fr.taus)
            if self.double_q:
                _, next_q = self.policy.q_net.quantiles(self.policy.extract_features(next_obs), fr.taus)
        out = iqn_loss(self.policy, features, fr.tau_hats, next_quantiles, next_q, batch.actions, batch.rewards, batch.dones, self.gamma,
                       self.huber_kappa, discounts=batch.discounts, weights=weights)
        with torch.no_grad():
            self._frac_m = fqf_fraction_loss(self.policy, features, batch.actions, weights, self.fqf_ent_coef, fractions=fr)
        self.last_fractions = fr
        return out

    def train_step(self):
        """one gradient step: a batch from the replay buffer (``_draw_batch``), the head's loss against the target network
        (``_train_step_`` + the policy's ``head_kind``, looked up on the instance at the call), the backward through the
        extractor, clip + Adam, and under prioritized replay the rows' errors back into the priority store.  Nothing is read from the device: the scalars
        add up in ``_acc`` until a callback reads them."""
        batch, idx, weights = self._draw_batch()
        self._draw_train_noise()
        loss, m, row_err = getattr(self, "_train_step_" + self.policy.head_kind)(batch, weights)
        loss.backward()
        self._adam_step()
        if self.fqf:
            self._fraction_step()
            self._frac_acc += torch.stack([self._frac_m[k] for k in FQF_SCALARS])
        if self.prioritized_replay:
            if self.n_tau_samples > 0:
                # a transition drawn twice sits in two rows with fractions of their own, so its rows' losses differ, and the priority
                # store takes one value per id (include/ocrl_hip_replay.h): the largest of them, whatever the rows' order
                same = idx.unsqueeze(1) == idx.unsqueeze(0)
                row_err = torch.where(same, row_err.unsqueeze(0), row_err.new_full((), -math.inf)).amax(dim=1)
            self.replay_buffer.update_priorities(idx, row_err, self.prioritized_replay_alpha, self.prioritized_replay_eps)
            self.last_weights = weights
        self.n_updates += 1
        self._acc += torch.cat([torch.stack([m[k] for k in DQN_SCALARS]), self._norm])
        self._acc_n += 1
        return loss

    def _train_stats(self, sums, n):
        out = {k: sums[i] / n for i, k in enumerate(DQN_SCALARS)}
        out.update(grad_norm=sums[len(DQN_SCALARS)] / n, n_updates=self.n_updates, exploration_rate=self.policy.exploration_rate)
        return out

    def train_stats(self):
        """means of DQN_SCALARS and the gradient norm over the updates since the last call (the last values again when there were none;
        NaN before the first update), ``n_updates`` and ``exploration_rate``.  Reads the device once."""
        if self._acc_n:
            self._last_train = self._train_stats(self._acc.tolist(), self._acc_n)
            if self.fqf:
                self._last_train.update({k: v / self._acc_n for k, v in zip(FQF_SCALARS, self._frac_acc.tolist())})
                self._frac_acc.zero_()
            self._acc.zero_()
            self._acc_n = 0
        self._last_train.update(n_updates=self.n_updates, exploration_rate=self.policy.exploration_rate)
        return dict(self._last_train)

    def learn(self, total_timesteps, callback=None):
        """steps and updates in turn until ``num_timesteps >= total_timesteps``; ``callback(locals_dict)`` every ``log_interval``
        iterations with the keys PPO's has.  Between the callbacks nothing is read from the device."""
        self._total_timesteps = int(total_timesteps)
        while self.num_timesteps < self._total_timesteps:
            for _ in range(self.train_freq):
                self.collect_step()
            if self.num_timesteps > self.learning_starts:
                for _ in range(self.gradient_steps):
                    self.train_step()
            self.iteration += 1
            if callback is not None and self.iteration % self.log_interval == 0:
                self._read_episodes()
                callback(dict(self=self, iteration=self.iteration, num_timesteps=self.num_timesteps, train=self.train_stats(),
                              ep_rew_mean=self.ep_rew_mean, ep_len_mean=self.ep_len_mean))
        self._read_episodes()
        return self

    # ---- checkpoints: plain dicts of tensors and numbers (torch.load(..., weights_only=True) reads them).  The replay buffer's contents
    # are not saved: a resumed run collects again before it updates (learning_starts counts from 0 only if the caller sets it so)
    def save(self, path):
        hyper = {k: getattr(self, k) for k in self.HYPER + ("seed", "num_timesteps", "iteration", "n_calls", "n_updates", "n_target_updates",
                                                            "_total_timesteps", "noise_draws")}
        opt = {"m": self.flat_m, "v": self.flat_v, "step": self.adam_step, "sampling_rows": self.policy._sample_rows}
        if self.fqf:
            opt["frac_sq"] = self.frac_sq
        torch.save({"algo": self.ALGO, "policy": self.policy.state_dict(), "target": self.target.state_dict(), "optimizer": opt, "hyper": hyper,
                    "exploration_rate": float(self.policy.exploration_rate)}, path)

    # load(): the keys (with the default a checkpoint from before them stands for) that must agree once the row's switch is on in the
    # checkpoint or in this instance, in the order they are reported
    _LOAD_GATED = (("n_tau_samples", (("n_tau_samples", 0), ("n_tau_prime_samples", 0), ("n_act_samples", 32), ("n_cos", 64))),
                   ("munchausen", (("munchausen", False), ("munchausen_alpha", 0.9), ("munchausen_tau", 0.03), ("munchausen_clip", -1.0))),
                   ("fqf", (("fqf", False), ("fqf_fraction_lr", 2.5e-9), ("fqf_ent_coef", 0.0))))

    def load(self, path):
        """restore the policy, the target network, Adam's state, the counters and the hyper-parameters saved by ``save`` into this instance
        (same policy layout); returns self.  The replay buffer stays as it is, unless the loaded ``n_step`` / ``prioritized_replay`` are not
        the ones it was built with: then it is dropped, and the next ``collect_step`` builds one that fits."""
        ck = torch.load(path, map_location=self.device, weights_only=True)
        wrote = ck.get("algo", "PPO")
        if wrote != self.ALGO:
            raise ValueError(f"{self._who}.load: {path} was written by {wrote}, not by {self.ALGO} (each algorithm loads its own checkpoints only)")
        hyper = ck["hyper"]
        if self.n_atoms > 1 and (float(hyper.get("v_min", self.v_min)), float(hyper.get("v_max", self.v_max))) != (self.v_min, self.v_max):
            raise ValueError(f"{self._who}.load: the checkpoint's support v_min, v_max = {hyper['v_min']}, {hyper['v_max']} is not this "
                             f"policy's {self.v_min}, {self.v_max}")
        if int(hyper.get("n_quantiles", 0)) != self.n_quantiles:
            raise ValueError(f"{self._who}.load: the checkpoint was written with n_quantiles = {int(hyper.get('n_quantiles', 0))}, this instance "
                             f"has n_quantiles = {self.n_quantiles}")
        for switch, pairs in self._LOAD_GATED:
            gate = bool(getattr(self, switch)) or bool(hyper.get(switch, False))
            for k, dflt in pairs:
                have, mine = type(dflt)(hyper.get(k, dflt)), getattr(self, k)
                if gate and have != mine:
                    raise ValueError(f"{self._who}.load: the checkpoint was written with {k} = {have}, this instance has {k} = {mine}")
        opt = ck["optimizer"]
        if self.fqf and ("frac_sq" not in opt or opt["frac_sq"].shape != self.frac_sq.shape):
            raise ValueError(f"{self._who}.load: the checkpoint's optimiser state has no frac_sq of this policy's {self.frac_sq.numel()} entries")
        if "m" not in opt or opt["m"].shape != self.flat_m.shape:
            n = opt["m"].numel() if "m" in opt else "no"
            raise ValueError(f"{self._who}.load: the checkpoint's optimiser state has {n} Adam entries, this policy's {self.flat_m.numel()}")
        self.policy.load_state_dict(ck["policy"])                       # copies in place: the parameters stay views of flat_p
        self.target.load_state_dict(ck["target"])                       # ... and of flat_target
        self.flat_m.copy_(opt["m"])
        self.flat_v.copy_(opt["v"])
        if self.fqf:
            self.frac_sq.copy_(opt["frac_sq"])
        self.adam_step = int(opt["step"])
        self.policy._sample_rows = int(opt["sampling_rows"])
        self.policy._sample_seed = int(ck["hyper"]["seed"]) & (2 ** 64 - 1)
        if bool(hyper.get("noisy", False)) != self.noisy:
            raise ValueError(f"{self._who}.load: the checkpoint was written with noisy = {bool(hyper.get('noisy', False))}, this instance has "
                             f"noisy = {self.noisy}")
        if self.noisy:
            self.target._sample_seed = (int(ck["hyper"]["seed"]) + 1) & (2 ** 64 - 1)
        for k, v in ck["hyper"].items():
            setattr(self, k, v)
        self.policy.exploration_rate = float(ck["exploration_rate"])
        buf = self.replay_buffer
        if buf is not None and (buf.prioritized, buf.n_step) != (self.prioritized_replay, self.n_step):
            self.replay_buffer = None
        return self


__all__ = ["DQN", "DQNPolicy", "QNetwork", "CategoricalQNetwork", "QuantileQNetwork", "ImplicitQuantileQNetwork", "dqn_loss", "c51_loss", "qr_loss", "iqn_loss", "munchausen_targets", "FullyParameterizedQuantileQNetwork", "fqf_fraction_loss", "exploration_schedule", "DQN_SCALARS"]
