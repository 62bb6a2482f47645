"""Actor-critic network of the RL agent (sb3s/custom_acnets.py:8-128) and the PPO and A2C losses it is trained with.

``CustomNetwork`` holds the parameters in the reference's containers (``shared_net`` / ``policy_net`` / ``value_net``: nn.Sequential
of [nn.Linear, nn.ReLU | nn.Tanh] pairs), so ``state_dict()`` keys, shapes and initialisation are the reference's and its checkpoints
load unchanged; the containers' ``forward`` is never called.  The arithmetic is ``ocrl_acnet_fwd/_bwd`` (HIP: the whole chain of a
row tile in one kernel) under a ``torch.autograd.Function``.  No CPU fallback: a CPU tensor raises.

``CustomActorCriticPolicy`` subclasses stable-baselines3's ``ActorCriticPolicy`` as the reference does when that package is
installed.  Without it, it is a plain nn.Module with the heads that base class adds (``action_net``, ``value_net``, a categorical
distribution), restated from the published algorithm; ``ppo_loss`` is the loss of ``PPO.train`` (clip_range_vf = None) through
``ocrl_acnet_ppo_fwd_bwd``, ``a2c_loss`` the loss of ``A2C.train`` through ``ocrl_acnet_a2c_fwd_bwd`` and ``compute_gae`` the rollout buffer's advantage estimation through ``ocrl_gae``."""
import ctypes
import math
import numbers

import torch
from torch import nn

from .. import _bridge, _lib

_WHO = "ocrl_amd.sb3s"
_ACT_CODE = {nn.ReLU: 1, nn.Tanh: 2}
PPO_SCALARS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")
A2C_SCALARS = PPO_SCALARS[:4]


def _desc(B, F, A, dims, acts, dev, keep=True):
    """(descriptor, workspace) of a call"""
    d = _lib.acnet_desc(B, F, A, dims, acts)
    return d, _bridge.workspace(_WHO, _lib.lib().ocrl_acnet_ws_floats(ctypes.byref(d)), dev,
                                f"batch {B}, feature_dim {F}, {A} actions, trunk widths {[list(x) for x in dims]}", keep)


class _AcnetFn(torch.autograd.Function):
    """(latent_pi, latent_vf) for A == 0, (logits, values) for A > 0"""

    @staticmethod
    def forward(ctx, features, dims, acts, A, *params):
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        need_grad = any(ctx.needs_input_grad)
        d, ws = _desc(B, F, A, dims, acts, dev, need_grad)
        h = dims[0][-1] if dims[0] else F
        if A > 0:
            outs = (torch.empty(B, A, device=dev), torch.empty(B, device=dev))
            args = (None, None, _lib.ptr(outs[0]), _lib.ptr(outs[1]))
        else:
            outs = (torch.empty(B, dims[1][-1] if dims[1] else h, device=dev), torch.empty(B, dims[2][-1] if dims[2] else h, device=dev))
            args = (_lib.ptr(outs[0]), _lib.ptr(outs[1]), None, None)
        _bridge.launch(dev, _lib.lib().ocrl_acnet_fwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps) if ps else None, *args, int(need_grad),
                       _lib.ptr(ws) if need_grad else None, ws.numel())
        ctx.save_for_backward(x, *ps)
        ctx.d, ctx.ws, ctx.A = d, ws, A
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, g0, g1):
        x, *ps = ctx.saved_tensors
        g0, g1 = _bridge.cotangent(g0), _bridge.cotangent(g1)          # kept alive to the launch: the conversion may have copied them
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        cot = (None, None, _lib.ptr(g0), _lib.ptr(g1)) if ctx.A > 0 else (_lib.ptr(g0), _lib.ptr(g1), None, None)
        _bridge.launch(x.device, _lib.lib().ocrl_acnet_bwd, ctypes.byref(ctx.d), _lib.ptr(x), _lib.ptrs(ps) if gs else None, *cot, _lib.ptr(dx),
                       _lib.ptrs(gs) if gs else None, _lib.ptr(ctx.ws), ctx.ws.numel())
        return (dx, None, None, None, *gs)


class _PPOFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, actions, old_log_prob, advantages, returns, hyper, dims, acts, A, *params):
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        clip_range, vf_coef, ent_coef, normalize = hyper
        if normalize and B < 2:
            raise ValueError(f"{_WHO}.ppo_loss: normalize_advantage needs a batch of at least 2 (the std of one advantage is undefined)")
        vec = lambda t, dt: t.to(device=dev, dtype=dt).reshape(-1).contiguous()
        actions, old_log_prob = vec(actions, torch.int64), vec(old_log_prob, torch.float32)
        advantages, returns = vec(advantages, torch.float32), vec(returns, torch.float32)
        for name, t in (("actions", actions), ("old_log_prob", old_log_prob), ("advantages", advantages), ("returns", returns)):
            if t.numel() != B:
                raise ValueError(f"{_WHO}.ppo_loss: {name} has {t.numel()} entries for a batch of {B}")
        d, ws = _desc(B, F, A, dims, acts, dev)
        scal = torch.empty(6, device=dev, dtype=torch.float32)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(dev, _lib.lib().ocrl_acnet_ppo_fwd_bwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(actions), _lib.ptr(old_log_prob),
                       _lib.ptr(advantages), _lib.ptr(returns), float(clip_range), float(vf_coef), float(ent_coef), int(bool(normalize)),
                       _lib.ptr(scal), _lib.ptr(dx), _lib.ptrs(gs), _lib.ptr(ws), ws.numel())
        ctx.gs, ctx.dx = gs, dx              # the gradients are the forward's own outputs: the backward reads nothing else again
        ctx.mark_non_differentiable(scal)
        return scal[0].clone(), scal

    @staticmethod
    def backward(ctx, gloss, _gscal):
        dx = None if ctx.dx is None else ctx.dx * gloss
        return (dx, None, None, None, None, None, None, None, None, *[g * gloss for g in ctx.gs])


class _A2CFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, actions, advantages, returns, hyper, dims, acts, A, *params):
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        B, F = x.shape
        vf_coef, ent_coef, normalize = hyper
        if normalize and B < 2:
            raise ValueError(f"{_WHO}.a2c_loss: normalize_advantage needs a batch of at least 2 (the std of one advantage is undefined)")
        vec = lambda t, dt: t.to(device=dev, dtype=dt).reshape(-1).contiguous()
        actions, advantages, returns = vec(actions, torch.int64), vec(advantages, torch.float32), vec(returns, torch.float32)
        for name, t in (("actions", actions), ("advantages", advantages), ("returns", returns)):
            if t.numel() != B:
                raise ValueError(f"{_WHO}.a2c_loss: {name} has {t.numel()} entries for a batch of {B}")
        d, ws = _desc(B, F, A, dims, acts, dev)
        scal = torch.empty(4, device=dev, dtype=torch.float32)
        gs = [torch.empty_like(p) for p in ps]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _bridge.launch(dev, _lib.lib().ocrl_acnet_a2c_fwd_bwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(actions), _lib.ptr(advantages),
                       _lib.ptr(returns), float(vf_coef), float(ent_coef), int(bool(normalize)), _lib.ptr(scal), _lib.ptr(dx), _lib.ptrs(gs),
                       _lib.ptr(ws), ws.numel())
        ctx.gs, ctx.dx = gs, dx              # as in _PPOFn: the gradients are the forward's own outputs
        ctx.mark_non_differentiable(scal)
        return scal[0].clone(), scal

    @staticmethod
    def backward(ctx, gloss, _gscal):
        dx = None if ctx.dx is None else ctx.dx * gloss
        return (dx, None, None, None, None, None, None, None, *[g * gloss for g in ctx.gs])


def _mlp(in_dim, cfg):
    """nn.Sequential([nn.Linear, nn.ReLU | nn.Tanh] x len(dims)) with the reference's indices (custom_acnets.py:37-48)"""
    layers = []
    for dim, act in zip(cfg.dims, cfg.acts):
        layers.append(nn.Linear(in_dim, dim))
        if act == "relu":
            layers.append(nn.ReLU())
        elif act == "tanh":
            layers.append(nn.Tanh())
        else:
            raise ValueError(f"{act} is not implemented")
        in_dim = dim
    return nn.Sequential(*layers)


class CustomNetwork(nn.Module):
    def __init__(self, feature_dim: int, config) -> None:
        super().__init__()
        # custom_acnets.py:27-34: the widths the distributions and the value head are built on
        self.latent_dim_pi = config.policy_net.dims[-1] if len(config.policy_net.dims) > 0 else feature_dim
        self.latent_dim_vf = config.value_net.dims[-1] if len(config.value_net.dims) > 0 else feature_dim
        self.shared_net = _mlp(feature_dim, config.shared_net)
        in_dim = config.shared_net.dims[-1] if len(config.shared_net.dims) > 0 else feature_dim
        self.policy_net = _mlp(in_dim, config.policy_net)
        self.value_net = _mlp(in_dim, config.value_net)

    def _trunks(self):
        return (self.shared_net, self.policy_net, self.value_net)

    def _layout(self):
        """(widths, activation codes) of the three trunks, as the C ABI takes them"""
        dims = tuple(tuple(m.out_features for m in seq if isinstance(m, nn.Linear)) for seq in self._trunks())
        acts = tuple(tuple(_ACT_CODE[type(m)] for m in seq if not isinstance(m, nn.Linear)) for seq in self._trunks())
        return dims, acts

    def _param_list(self):
        return [p for seq in self._trunks() for m in seq if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]

    def forward(self, features):
        dims, acts = self._layout()
        if not any(dims):                                   # the reference returns its input object itself, twice
            _bridge.gpu_input(_WHO, features)               # no CPU path, even where nothing is computed
            return features, features
        return _AcnetFn.apply(features, dims, acts, 0, *self._param_list())

    def forward_actor(self, features):
        return self.forward(features)[0]

    def forward_critic(self, features):
        return self.forward(features)[1]


try:                                                          # optional dependency, exactly as in the reference when present
    from stable_baselines3.common.policies import ActorCriticPolicy as _SB3Policy
except Exception:                                             # pragma: no cover - stable_baselines3 is not in this image
    _SB3Policy = None


def _n_actions(action_space):
    n = getattr(action_space, "n", None)
    if isinstance(n, bool) or not isinstance(n, numbers.Integral):
        raise NotImplementedError(f"CustomActorCriticPolicy supports Discrete action spaces only (an integer .n); got {action_space!r} "
                                  f"of type {type(action_space).__name__} (a continuous Box space, as CausalWorld's, is not built)")
    return int(n)


def _ortho(module, gain):
    """stable-baselines3's init_weights: orthogonal weights of the given gain and zero biases on every Linear / Conv2d"""
    for m in module.modules():
        if isinstance(m, (nn.Linear, nn.Conv2d)):
            nn.init.orthogonal_(m.weight, gain=gain)
            if m.bias is not None:
                m.bias.data.fill_(0.0)


if _SB3Policy is not None:                                    # pragma: no cover - stable_baselines3 is not in this image
    class CustomActorCriticPolicy(_SB3Policy):
        def __init__(self, observation_space, action_space, lr_schedule, net_arch=None, activation_fn=nn.Tanh, config=None, *args, **kwargs):
            self._config = config
            super().__init__(observation_space, action_space, lr_schedule, net_arch, activation_fn, *args, **kwargs)
            self.ortho_init = config.sb3_acnet.ortho_init

        def _build_mlp_extractor(self) -> None:
            self.mlp_extractor = CustomNetwork(self.features_dim, self._config.sb3_acnet)
else:
    class CustomActorCriticPolicy(nn.Module):
        """features_extractor -> CustomNetwork -> action_net (Linear(latent_dim_pi, n)) / value_net (Linear(latent_dim_vf, 1)) with a
        categorical distribution over the logits.  ``features_extractor`` is a module with ``features_dim`` (an OCRExtractor), or
        ``features_extractor_class(observation_space, **features_extractor_kwargs)``; without either the observations are flattened."""

        def __init__(self, observation_space, action_space, lr_schedule=None, net_arch=None, activation_fn=nn.Tanh, config=None,
                     features_extractor=None, features_extractor_class=None, features_extractor_kwargs=None, **kwargs):
            super().__init__()
            self._config = config
            self.observation_space, self.action_space = observation_space, action_space
            n = _n_actions(action_space)
            if features_extractor is None and features_extractor_class is not None:
                features_extractor = features_extractor_class(observation_space, **(features_extractor_kwargs or {}))
            if features_extractor is None:
                features_extractor = nn.Flatten()
                self.features_dim = int(math.prod(observation_space.shape))
            else:
                self.features_dim = int(features_extractor.features_dim)
            self.features_extractor = features_extractor
            self.ortho_init = bool(config.sb3_acnet.ortho_init)
            self.mlp_extractor = CustomNetwork(self.features_dim, config.sb3_acnet)
            self.action_net = nn.Linear(self.mlp_extractor.latent_dim_pi, n)
            self.value_net = nn.Linear(self.mlp_extractor.latent_dim_vf, 1)
            if self.ortho_init:
                for module, gain in ((self.features_extractor, math.sqrt(2)), (self.mlp_extractor, math.sqrt(2)), (self.action_net, 0.01),
                                     (self.value_net, 1.0)):
                    _ortho(module, gain)

        def extract_features(self, obs):
            return self.features_extractor(obs)

        def _head_args(self):
            dims, acts = self.mlp_extractor._layout()
            params = self.mlp_extractor._param_list() + [self.action_net.weight, self.action_net.bias, self.value_net.weight, self.value_net.bias]
            return dims, acts, self.action_net.out_features, params

        def logits_values(self, features):
            """(logits [B, n], values [B]) of a feature batch: one kernel launch"""
            dims, acts, A, params = self._head_args()
            return _AcnetFn.apply(features, dims, acts, A, *params)

        _sample_seed = None                                   # set_sampling(): forward then samples inside the head's launch
        _sample_rows = 0

        def set_sampling(self, seed):
            """give the policy a sampling stream: ``forward`` then acts through ``ocrl_acnet_act`` (one launch after the extractor), row
            r of the n-th call drawing from (seed, rows of the earlier calls + r); ``None`` returns to torch's sampler"""
            self._sample_seed = None if seed is None else int(seed) & (2 ** 64 - 1)
            self._sample_rows = 0

        def act(self, features, row_offset=None, uniforms=None, deterministic: bool = False):
            """(actions int64 [B], values [B], log_prob [B]) of a feature batch in one kernel launch, detached (the rollout's step; the
            sampling rule is include/ocrl_hip.h's).  Row r draws from (the set_sampling seed, row_offset + r); ``row_offset=None`` takes and
            advances the policy's own row counter.  ``uniforms`` [B] in [0, 1) replaces the draw."""
            dims, acts, A, params = self._head_args()
            x, ps = _bridge.inputs(_WHO, features.detach(), params)
            B, F = x.shape
            if uniforms is not None:
                uniforms = uniforms.to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
                if uniforms.numel() != B:
                    raise ValueError(f"{_WHO}.act: {uniforms.numel()} uniforms for a batch of {B}")
            elif not deterministic and self._sample_seed is None:
                raise RuntimeError(f"{_WHO}.act: no sampling stream: call policy.set_sampling(seed) or pass uniforms")
            if row_offset is None:
                row_offset = self._sample_rows
                self._sample_rows += B
            d, _ = _desc(B, F, A, dims, acts, x.device, keep=False)
            actions = torch.empty(B, device=x.device, dtype=torch.int64)
            values, logp = torch.empty(B, device=x.device), torch.empty(B, device=x.device)
            _bridge.launch(x.device, _lib.lib().ocrl_acnet_act, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), self._sample_seed or 0, int(row_offset),
                           _lib.ptr(uniforms), int(bool(deterministic)), _lib.ptr(actions), _lib.ptr(values), _lib.ptr(logp), None)
            return actions, values, logp

        def forward(self, obs, deterministic: bool = False):
            if self._sample_seed is not None:
                actions, values, logp = self.act(self.extract_features(obs), deterministic=deterministic)
                return actions, values.unsqueeze(-1), logp
            logits, values = self.logits_values(self.extract_features(obs))
            logp = torch.log_softmax(logits, dim=-1)
            actions = logits.argmax(dim=-1) if deterministic else torch.multinomial(logp.exp(), 1).squeeze(-1)
            return actions, values.unsqueeze(-1), logp.gather(1, actions.unsqueeze(-1)).squeeze(-1)

        def evaluate_actions(self, obs, actions):
            logits, values = self.logits_values(self.extract_features(obs))
            logp = torch.log_softmax(logits, dim=-1)
            entropy = -(logp.exp() * logp).sum(-1)
            return values.unsqueeze(-1), logp.gather(1, actions.long().reshape(-1, 1)).squeeze(-1), entropy

        def predict_values(self, obs):
            return self.logits_values(self.extract_features(obs))[1].unsqueeze(-1)


def ppo_loss(policy, features, actions, old_log_prob, advantages, returns, clip_range, vf_coef, ent_coef, normalize_advantage=True):
    """PPO's minibatch loss of ``policy`` on a feature batch [B, F] (``policy.extract_features(obs)``): (loss, metrics).  ``loss`` is
    attached to autograd: ``backward()`` puts the gradients on the policy's trunk and head parameters and on ``features``.  ``metrics``
    maps PPO_SCALARS to detached 0-d tensors."""
    dims, acts = policy.mlp_extractor._layout()
    params = policy.mlp_extractor._param_list() + [policy.action_net.weight, policy.action_net.bias, policy.value_net.weight, policy.value_net.bias]
    loss, scal = _PPOFn.apply(features, actions, old_log_prob, advantages, returns, (clip_range, vf_coef, ent_coef, normalize_advantage), dims, acts,
                              policy.action_net.out_features, *params)
    return loss, {k: scal[i] for i, k in enumerate(PPO_SCALARS)}


def a2c_loss(policy, features, actions, advantages, returns, vf_coef, ent_coef, normalize_advantage=False):
    """A2C's loss of ``policy`` on a feature batch [B, F]: (loss, metrics), attached to autograd as ``ppo_loss`` is.  ``metrics`` maps
    A2C_SCALARS to detached 0-d tensors."""
    dims, acts = policy.mlp_extractor._layout()
    params = policy.mlp_extractor._param_list() + [policy.action_net.weight, policy.action_net.bias, policy.value_net.weight, policy.value_net.bias]
    loss, scal = _A2CFn.apply(features, actions, advantages, returns, (vf_coef, ent_coef, normalize_advantage), dims, acts,
                              policy.action_net.out_features, *params)
    return loss, {k: scal[i] for i, k in enumerate(A2C_SCALARS)}


def compute_gae(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda):
    """advantages, returns [T, E] of a rollout on the device (rewards, values, episode_starts [T, E]; last_values, dones [E])"""
    rewards = _bridge.gpu_input(_WHO + ".compute_gae", rewards)
    f = lambda t: t.to(device=rewards.device, dtype=torch.float32).contiguous()
    values, episode_starts = f(values), f(episode_starts)
    T, E = rewards.shape
    last_values, dones = f(last_values).reshape(E), f(dones).reshape(E)
    if values.shape != (T, E) or episode_starts.shape != (T, E):
        raise ValueError(f"{_WHO}.compute_gae: rewards, values and episode_starts must share the shape [T, E] (got {tuple(rewards.shape)}, "
                         f"{tuple(values.shape)}, {tuple(episode_starts.shape)})")
    adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    _bridge.launch(rewards.device, _lib.lib().ocrl_gae, _lib.ptr(rewards), _lib.ptr(values), _lib.ptr(episode_starts), _lib.ptr(last_values),
                   _lib.ptr(dones), _lib.ptr(adv), _lib.ptr(ret), T, E, float(gamma), float(gae_lambda))
    return adv, ret
