"""What the on-policy algorithms share (the reference's ``train_sb3.py:97-118`` calls ``getattr(sb3, config.sb3.name)(...).learn(...)``
of stable-baselines3; that package is not a dependency here): the rollout buffer, rollout collection, episode tracking, ``predict``, the
flat parameter / gradient buffers, the L2 clip + Adam step, ``learn`` and the checkpoint's frame.  ``PPO`` (ppo.py) and ``A2C`` (a2c.py)
add their ``train()`` and their hyper-parameters.

``RolloutBuffer`` and ``OnPolicyAlgorithm`` restate stable-baselines3 1.5's classes of the same names from the published algorithms: none
of their text is copied.  The GPU work is the library's: acting is ``CustomActorCriticPolicy.forward`` with a sampling stream
(``ocrl_acnet_act``: one launch after the extractor), advantages are ``compute_gae`` and the Adam update ``ocrl_flat_clip_adam_l2`` on one
flat parameter buffer.  A trainable SLATE / Slot-Attention encoder behind the extractor keeps its parameters in its engine's flat buffer;
the update then is ``ocrl_flat_clip_adam_l2_multi`` / ``ocrl_flat_clip_rmsprop_l2_multi`` over two segments, the policy's buffer and the
encoder's range, as stable-baselines3 clips and steps all of ``policy.parameters()`` together.  Where this departs from
stable-baselines3 is listed in DESIGN.md §7."""
import collections
import numbers

import numpy as np
import torch

from .. import _lib
from ..ocrs.flat_module import FlatParamModule
from .custom_acnets import _n_actions, compute_gae

ALGOS = ("PPO", "A2C")          # the classes built on OnPolicyAlgorithm; a checkpoint names the one that wrote it
ADAM_EPS = 1e-5                 # stable-baselines3's ActorCriticPolicy builds Adam with eps = 1e-5
ENCODER_TENSORS = ("_enc.", "_enc_pos.", "_slotattn.")        # what ocrl_slate_encode_backward writes: SLATE's group 1 up to the slot projection
RolloutBatch = collections.namedtuple("RolloutBatch", "observations actions old_values old_log_prob advantages returns")


def _tensor(x, device, dtype=None):
    """a numpy array or a tensor -> a tensor on `device` (dtype kept unless given)"""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=device, dtype=dtype) if dtype is not None else t.to(device=device)


class RolloutBuffer:
    """n_steps x n_envs transitions in tensors [T, E, ...] on ``device``; observations stay in the dtype they arrive in (``obs_dtype``;
    uint8 frames stay uint8).  Storage and ``get`` are pure indexing and work on any device; ``compute_returns_and_advantage`` is
    ``compute_gae`` and needs the GPU."""

    def __init__(self, n_steps, n_envs, obs_shape, device="cuda", gamma=0.99, gae_lambda=0.95, obs_dtype=torch.float32):
        self.n_steps, self.n_envs, self.obs_shape = int(n_steps), int(n_envs), tuple(obs_shape)
        self.device, self.gamma, self.gae_lambda = torch.device(device), float(gamma), float(gae_lambda)
        T, E = self.n_steps, self.n_envs
        f = lambda: torch.zeros(T, E, device=self.device, dtype=torch.float32)
        self.observations = torch.zeros(T, E, *self.obs_shape, device=self.device, dtype=obs_dtype)
        self.actions = torch.zeros(T, E, device=self.device, dtype=torch.int64)
        self.rewards, self.episode_starts, self.values, self.log_probs, self.advantages, self.returns = f(), f(), f(), f(), f(), f()
        self.reset()

    def reset(self):
        self.pos, self.full, self._flat = 0, False, None

    def add(self, obs, actions, rewards, episode_starts, values, log_probs):
        """one step of every environment: obs [E, ...], the others [E] (values may be [E, 1])"""
        if self.pos >= self.n_steps:
            raise RuntimeError(f"RolloutBuffer.add: the buffer already holds its {self.n_steps} steps (reset() it)")
        t, E = self.pos, self.n_envs
        self.observations[t].copy_(_tensor(obs, self.device).reshape(E, *self.obs_shape))
        self.actions[t].copy_(_tensor(actions, self.device).reshape(E))
        for dst, src in ((self.rewards, rewards), (self.episode_starts, episode_starts), (self.values, values), (self.log_probs, log_probs)):
            dst[t].copy_(_tensor(src, self.device).reshape(E))
        self.pos += 1
        self.full = self.pos == self.n_steps
        self._flat = None

    def compute_returns_and_advantage(self, last_values, dones):
        """GAE(lambda) over the stored steps: last_values, dones [E] belong to the observation after the last step"""
        E = self.n_envs
        adv, ret = compute_gae(self.rewards, self.values, self.episode_starts, _tensor(last_values, self.device, torch.float32).reshape(E),
                               _tensor(dones, self.device, torch.float32).reshape(E), self.gamma, self.gae_lambda)
        self.advantages.copy_(adv)
        self.returns.copy_(ret)
        self._flat = None

    @staticmethod
    def swap_and_flatten(t):
        """[T, E, ...] -> [E * T, ...]: row e * T + t is environment e's step t"""
        return t.transpose(0, 1).reshape(t.shape[0] * t.shape[1], *t.shape[2:])

    def flat(self):
        """the whole buffer as one RolloutBatch of T * E rows in flattened order (row e * T + t), no copy of the generator's state"""
        if not self.full:
            raise RuntimeError(f"RolloutBuffer.flat: the buffer holds {self.pos} of {self.n_steps} steps")
        if self._flat is None:
            self._flat = RolloutBatch(*[self.swap_and_flatten(t) for t in (self.observations, self.actions, self.values, self.log_probs,
                                                                           self.advantages, self.returns)])
        return self._flat

    def get(self, batch_size=None, perm=None, generator=None):
        """minibatches of ``batch_size`` rows (None: one batch of everything) of the flattened buffer, in the order of ``perm`` (a
        permutation of T * E; None: drawn on the buffer's device from ``generator``).  The last one may be short."""
        if not self.full:
            raise RuntimeError(f"RolloutBuffer.get: the buffer holds {self.pos} of {self.n_steps} steps")
        n = self.n_steps * self.n_envs
        flat = self.flat()
        if perm is None:
            perm = torch.randperm(n, device=self.device, generator=generator)
        perm = _tensor(perm, self.device, torch.int64).reshape(-1)
        if perm.numel() != n:
            raise ValueError(f"RolloutBuffer.get: perm has {perm.numel()} entries for {n} rows")
        batch_size = n if batch_size is None else int(batch_size)
        for start in range(0, n, batch_size):
            idx = perm[start:start + batch_size]
            yield RolloutBatch(*[t[idx] for t in flat])


def _check_constant(who, name, v):
    if callable(v):
        raise NotImplementedError(f"{who}: a schedule (callable) for {name} is not built; pass a number")
    if not isinstance(v, numbers.Real):
        raise TypeError(f"{who}: {name} must be a number (got {v!r})")
    return float(v)


class OnPolicyAlgorithm:
    """An on-policy actor-critic algorithm for Discrete actions on a VecEnv.  ``env`` has ``num_envs``, ``observation_space``,
    ``action_space``, ``reset() -> obs [E, ...]`` and ``step(actions) -> (obs, rewards [E], dones [E], infos)`` with numpy arrays or
    tensors.  ``policy`` is a CustomActorCriticPolicy or its class (built as ``policy(env.observation_space, env.action_space, None,
    **policy_kwargs)``).  A subclass names itself in ``ALGO``, lists what ``save`` keeps in ``HYPER``, and provides ``train()``,
    ``_init_optimizer()``, ``_optimizer_state()`` and ``_load_optimizer_state()``."""
    ALGO = None
    HYPER = ()

    def __init__(self, policy, env, learning_rate, n_steps, gamma, gae_lambda, ent_coef, vf_coef, max_grad_norm, normalize_advantage, seed, device,
                 policy_kwargs):
        _WHO = self._who = f"ocrl_amd.sb3s.{self.ALGO}"
        self.learning_rate = _check_constant(_WHO, "learning_rate", learning_rate)
        self.n_actions = _n_actions(env.action_space)                 # Discrete only: the policy's own message otherwise
        self.env, self.n_envs = env, int(env.num_envs)
        self.n_steps = int(n_steps)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.ent_coef, self.vf_coef = float(ent_coef), float(vf_coef)
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.normalize_advantage, self.seed = bool(normalize_advantage), int(seed)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if isinstance(policy, type):
            torch.manual_seed(self.seed)                              # the initialisation follows the seed, as set_random_seed does
            policy = policy(env.observation_space, env.action_space, None, **(policy_kwargs or {}))
        if not hasattr(policy, "set_sampling"):
            raise TypeError(f"{_WHO}: policy must be an ocrl_amd.sb3s.CustomActorCriticPolicy (or the class), got {type(policy).__name__}")
        self.policy = policy.to(self.device)
        self._encoder = None
        for m in self.policy.modules():
            if isinstance(m, FlatParamModule):
                if self._encoder is not None or m.backend != "SLATE" or not getattr(m, "finetune_through_slots", False):
                    raise NotImplementedError(f"{_WHO}: a trainable {m.backend} encoder behind the extractor keeps its own flat buffers and optimiser "
                                              f"step; stepping it from {self.ALGO} is not built: give the extractor a pre-trained, frozen encoder")
                self._encoder = m
        if self._encoder is not None:
            # sized once for the rollouts and the minibatches alike: no rebuild, and so no re-seating of its flat buffers, inside learn()
            if getattr(self._encoder, "_device", None) is None:
                self._encoder.to(self.device)
            self._encoder._ensure_engine(max(self.n_envs, self.batch_size))
        self.policy.set_sampling(self.seed)
        self.generator = torch.Generator(device=self.device).manual_seed(self.seed)
        self._flatten_parameters()
        self.num_timesteps, self.iteration = 0, 0
        obs_shape = tuple(env.observation_space.shape)
        self.rollout_buffer = None
        self._obs_shape = obs_shape
        self._last_obs, self._last_starts = None, None
        self._ep_ret, self._ep_len = np.zeros(self.n_envs), np.zeros(self.n_envs, dtype=np.int64)
        self._episodes = collections.deque(maxlen=100)
        self._successes = collections.deque(maxlen=100)               # is_success of the same episodes (the on-device path fills it)

    # ---- the optimiser's view of the policy: one flat buffer each for parameters, gradients and the optimiser's state
    def _flatten_parameters(self):
        """re-seat every trainable parameter as a view of ``flat_p`` and its .grad as a view of ``flat_g`` (each starts on a multiple of
        4 floats; the padding stays zero).  state_dict() keeps its keys and shapes and reads the same memory the optimiser writes.  The
        optimiser's own state is the subclass's (``_init_optimizer``).  A trainable SLATE encoder's parameters are left where they are:
        views of its engine's flat buffer, which the HIP model is bound to; the step reaches them as a second segment
        (``_encoder_range``)."""
        own = set() if self._encoder is None else {id(p) for p in self._encoder.parameters()}
        params = [p for p in self.policy.parameters() if p.requires_grad and id(p) not in own]
        for p in params:
            if p.dtype != torch.float32 or p.device != self.device:
                raise RuntimeError(f"{self._who}: parameters must be float32 on {self.device} (got {p.dtype} on {p.device})")
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + 3) & ~3
        n = max(n, 4)
        self.flat_p, self.flat_g = (torch.zeros(n, device=self.device) for _ in range(2))
        for p, o in zip(params, offs):
            view = self.flat_p[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = self.flat_g[o:o + p.numel()].view(p.shape)
        self._params = params
        self._norm = torch.zeros(1, device=self.device)
        self._enc_range = self._encoder_range()
        self._init_optimizer()

    # ---- a trainable SLATE encoder: the second segment of the step
    def _encoder_range(self):
        """(first float, length) of the smallest contiguous range of the encoder engine's flat buffer that covers the tensors
        ocrl_slate_encode_backward writes (ENCODER_TENSORS), from the engine's own parameter table; None without such an encoder.  The
        16-byte gaps between the tensors are zero in every buffer and stay so under the step."""
        if self._encoder is None:
            return None
        eng = self._encoder.engine
        live = [p for p in eng.params if p.name.startswith(ENCODER_TENSORS)]
        lo, hi = min((p.offset for p in live), default=0), max((p.offset + p.numel for p in live), default=0)
        other = [p.name for p in eng.params if not p.name.startswith(ENCODER_TENSORS) and p.offset < hi and p.offset + p.numel > lo]
        if not live or other or lo % 4:
            raise RuntimeError(f"{self._who}: the encoder's tensors do not form one 16-byte aligned range of its flat buffer ({lo}..{hi}, {other})")
        return lo, hi - lo

    def _new_encoder_state(self, value):
        """a fresh optimiser-state buffer for the encoder's range (the reference builds a fresh optimiser over policy.parameters(): the
        engine's flat_m / flat_v belong to the pre-training optimiser and are neither read nor written here); None without an encoder"""
        return None if self._enc_range is None else torch.full((self._enc_range[1],), float(value), device=self.device)

    def _segments(self, s0, s1, enc_s0, enc_s1):
        """the two segments of one step, policy then encoder; the encoder's pointers are resolved from its engine at every step"""
        eng, (lo, n) = self._encoder.engine, self._enc_range
        if eng.device != self.device:
            raise RuntimeError(f"{self._who}: the encoder lives on {eng.device}, the policy on {self.device}")
        return _lib.flat_segments([(_lib.ptr(self.flat_p), _lib.ptr(self.flat_g), _lib.ptr(s0), _lib.ptr(s1), self.flat_p.numel()),
                                   (_lib.ptr(eng.flat_p[lo:lo + n]), _lib.ptr(eng.flat_g[lo:lo + n]), _lib.ptr(enc_s0), _lib.ptr(enc_s1), n)])

    def _check_encoder_state(self, opt, keys):
        """load(): the checkpoint carries the encoder's optimiser state exactly when this policy has such an encoder, at its length"""
        have = [k for k in keys if k in opt]
        if self._enc_range is None:
            if have:
                raise ValueError(f"{self._who}.load: the checkpoint carries a trainable encoder's optimiser state ({', '.join(have)}), this policy "
                                 "has no such encoder")
            return
        n = self._enc_range[1]
        for k in keys:
            if k not in opt or opt[k].numel() != n:
                got = opt[k].numel() if k in opt else "no"
                raise ValueError(f"{self._who}.load: the checkpoint's optimiser state has {got} {k} entries, this policy's encoder range {n}")

    def _init_adam(self):
        """Adam's two moments beside flat_p (and the encoder range's own), the step counter and the step's workspace"""
        self.flat_m, self.flat_v = (torch.zeros_like(self.flat_p) for _ in range(2))
        self.enc_m, self.enc_v = self._new_encoder_state(0.0), self._new_encoder_state(0.0)
        self.adam_step = 0
        L = _lib.lib()
        self._ws = torch.empty(L.ocrl_flat_clip_adam_ws_floats() if self._encoder is None else L.ocrl_flat_clip_multi_ws_floats(), device=self.device)

    def _adam_step(self):
        """L2 clip of the whole gradient to max_grad_norm, then Adam (eps 1e-5): one C call, no host synchronisation.  With a trainable
        encoder the norm is the joint one of the policy's and the encoder's gradients and the one call steps both segments."""
        self.adam_step += 1
        with torch.cuda.device(self.device):
            if self._encoder is not None:
                seg = self._segments(self.flat_m, self.flat_v, self.enc_m, self.enc_v)
                _lib.check(_lib.lib().ocrl_flat_clip_adam_l2_multi(seg, len(seg), self.max_grad_norm, self.learning_rate, 0.9, 0.999, ADAM_EPS,
                                                                   self.adam_step, _lib.ptr(self._norm), _lib.ptr(self._ws), self._ws.numel(),
                                                                   _lib.stream(self.device)))
                return
            _lib.check(_lib.lib().ocrl_flat_clip_adam_l2(_lib.ptr(self.flat_p), _lib.ptr(self.flat_g), _lib.ptr(self.flat_m), _lib.ptr(self.flat_v),
                                                         self.flat_p.numel(), self.max_grad_norm, self.learning_rate, 0.9, 0.999, ADAM_EPS,
                                                         self.adam_step, _lib.ptr(self._norm), _lib.ptr(self._ws), self._ws.numel(),
                                                         _lib.stream(self.device)))

    # ---- observations
    def _obs(self, obs):
        """observations as the policy takes them: on the device; uint8 frames become floats in [0, 1] (stable-baselines3's preprocess_obs)"""
        t = _tensor(obs, self.device)
        return t.float() / 255.0 if t.dtype == torch.uint8 else t

    # ---- rollouts
    def _reset_env(self):
        self._last_obs = _tensor(self.env.reset(), self.device)
        self._last_starts = np.ones(self.n_envs, dtype=np.float32)
        self._ep_ret[:], self._ep_len[:] = 0.0, 0

    def collect_rollouts(self):
        """n_steps steps of every environment into a fresh buffer, then its returns and advantages.  An environment with ``on_device``
        set (ocrl_amd.envs) is stepped through ``step_device`` and nothing is read from the device between the steps."""
        if getattr(self.env, "on_device", False):
            return self._collect_rollouts_on_device()
        if self._last_obs is None:
            self._reset_env()
        if self.rollout_buffer is None:
            self.rollout_buffer = RolloutBuffer(self.n_steps, self.n_envs, self._obs_shape, self.device, self.gamma, self.gae_lambda, self._last_obs.dtype)
        buf = self.rollout_buffer
        buf.reset()
        self.policy.eval()
        with torch.no_grad():
            for _ in range(self.n_steps):
                actions, values, log_probs = self.policy(self._obs(self._last_obs))
                new_obs, rewards, dones, infos = self.env.step(actions.cpu().numpy())
                rewards_h = np.asarray(rewards.cpu() if isinstance(rewards, torch.Tensor) else rewards, dtype=np.float64).reshape(self.n_envs)
                dones_h = np.asarray(dones.cpu() if isinstance(dones, torch.Tensor) else dones).reshape(self.n_envs).astype(bool)
                self.num_timesteps += self.n_envs
                self._track_episodes(rewards_h, dones_h)
                rewards_d = torch.as_tensor(rewards_h, dtype=torch.float32).to(self.device)
                # an episode cut by its time limit is not over: its last reward is bootstrapped with the value of the observation it ended on
                cut = [i for i in np.nonzero(dones_h)[0] if infos[i].get("terminal_observation") is not None and infos[i].get("TimeLimit.truncated", False)]
                if cut:
                    term = torch.stack([_tensor(infos[i]["terminal_observation"], self.device) for i in cut])
                    rewards_d[torch.as_tensor(cut, device=self.device)] += self.gamma * self.policy.predict_values(self._obs(term))[:, 0]
                buf.add(self._last_obs, actions, rewards_d, self._last_starts, values, log_probs)
                self._last_obs = _tensor(new_obs, self.device)
                self._last_starts = dones_h.astype(np.float32)
            last_values = self.policy.predict_values(self._obs(self._last_obs))[:, 0]
        buf.compute_returns_and_advantage(last_values, self._last_starts)
        return buf

    def _collect_rollouts_on_device(self):
        """the same rollout with rewards, dones and the episode statistics left on the device: ``step_device`` returns tensors, the buffer
        takes them as they are, and the finished episodes of the whole rollout are read in one copy at its end, in (step, environment)
        order, so the 100-episode window fills as on the host path.  Such an environment ends its own episodes (no TimeLimit.truncated)."""
        T, E = self.n_steps, self.n_envs
        if self._last_obs is None:
            self._last_obs = _tensor(self.env.reset(), self.device)
            self._last_starts = torch.ones(E, device=self.device)
        if self.rollout_buffer is None:
            self.rollout_buffer = RolloutBuffer(T, E, self._obs_shape, self.device, self.gamma, self.gae_lambda, self._last_obs.dtype)
        buf = self.rollout_buffer
        buf.reset()
        stats = torch.zeros(T, 4, E, device=self.device, dtype=torch.float64)      # done, success, return, length of the episodes each step ended
        self.policy.eval()
        with torch.no_grad():
            for t in range(T):
                actions, values, log_probs = self.policy(self._obs(self._last_obs))
                new_obs, rewards, dones, extras = self.env.step_device(actions)
                self.num_timesteps += E
                buf.add(self._last_obs, actions, rewards, self._last_starts, values, log_probs)
                stats[t, 0], stats[t, 1], stats[t, 2], stats[t, 3] = dones, extras["is_success"], extras["episode_return"], extras["episode_length"]
                self._last_obs, self._last_starts = new_obs, dones.float()
            last_values = self.policy.predict_values(self._obs(self._last_obs))[:, 0]
        buf.compute_returns_and_advantage(last_values, self._last_starts)
        host = stats.cpu().numpy()                                    # the rollout's one read
        for t, e in zip(*np.nonzero(host[:, 0])):
            self._episodes.append((float(host[t, 2, e]), int(host[t, 3, e])))
            self._successes.append(bool(host[t, 1, e]))
        return buf

    def _track_episodes(self, rewards, dones):
        self._ep_ret += rewards
        self._ep_len += 1
        for i in np.nonzero(dones)[0]:
            self._episodes.append((float(self._ep_ret[i]), int(self._ep_len[i])))
            self._ep_ret[i], self._ep_len[i] = 0.0, 0

    @property
    def ep_rew_mean(self):
        return float(np.mean([r for r, _ in self._episodes])) if self._episodes else float("nan")

    @property
    def ep_len_mean(self):
        return float(np.mean([n for _, n in self._episodes])) if self._episodes else float("nan")

    @property
    def success_rate(self):
        """share of successes among the last 100 finished episodes (of an on-device environment)"""
        return float(np.mean(self._successes)) if self._successes else float("nan")

    # ---- the update
    def train(self):
        """one update phase on the full rollout buffer -> a dict of statistics (the subclass's)"""
        raise NotImplementedError

    def _explained_variance(self):
        """1 - Var(returns - values) / Var(returns) of the rollout buffer as a 0-d device tensor (NaN for constant returns)"""
        y, v = self.rollout_buffer.returns.reshape(-1), self.rollout_buffer.values.reshape(-1)
        var_y = y.var(unbiased=False)
        return torch.where(var_y == 0, torch.full_like(var_y, float("nan")), 1 - (y - v).var(unbiased=False) / var_y)

    def learn(self, total_timesteps, callback=None):
        """rollouts and updates in turn until ``num_timesteps >= total_timesteps``; ``callback(locals_dict)`` after every iteration"""
        while self.num_timesteps < int(total_timesteps):
            self.collect_rollouts()
            stats = self.train()
            self.iteration += 1
            if callback is not None:
                callback(dict(self=self, iteration=self.iteration, num_timesteps=self.num_timesteps, train=stats, ep_rew_mean=self.ep_rew_mean,
                              ep_len_mean=self.ep_len_mean))
        return self

    def predict(self, obs, deterministic=False):
        """(actions as a numpy array, None)"""
        self.policy.eval()
        with torch.no_grad():
            actions, _, _ = self.policy(self._obs(obs), deterministic=deterministic)
        return actions.cpu().numpy(), None

    # ---- checkpoints: plain dicts of tensors and numbers (torch.load(..., weights_only=True) reads them)
    def _hyper(self):
        return {k: getattr(self, k) for k in self.HYPER + ("seed", "num_timesteps", "iteration")}

    def _adam_state(self):
        out = {"m": self.flat_m, "v": self.flat_v, "step": self.adam_step}
        if self._encoder is not None:
            out.update(enc_m=self.enc_m, enc_v=self.enc_v)
        return out

    def _load_adam_state(self, opt):
        if "m" not in opt or opt["m"].shape != self.flat_m.shape:
            n = opt["m"].numel() if "m" in opt else "no"
            raise ValueError(f"{self._who}.load: the checkpoint's optimiser state has {n} Adam entries, this policy's {self.flat_m.numel()}")
        self._check_encoder_state(opt, ("enc_m", "enc_v"))
        self.flat_m.copy_(opt["m"])
        self.flat_v.copy_(opt["v"])
        if self._encoder is not None:
            self.enc_m.copy_(opt["enc_m"])
            self.enc_v.copy_(opt["enc_v"])
        self.adam_step = int(opt["step"])

    def save(self, path):
        opt = dict(self._optimizer_state())
        opt["sampling_rows"] = self.policy._sample_rows
        if self._encoder is not None:
            opt["enc_step_seed"] = self._encoder._step_seed          # where the encoder's slot-noise stream stands: a resumed run goes on from it
        torch.save({"algo": self.ALGO, "policy": self.policy.state_dict(), "optimizer": opt, "hyper": self._hyper(),
                    "generator": self.generator.get_state()}, path)     # where the minibatch permutations' stream stands

    def load(self, path):
        """restore policy, optimiser state and hyper-parameters saved by ``save`` into this instance (same algorithm and policy layout);
        returns self.  A file without "algo" was written by PPO before A2C existed."""
        ck = torch.load(path, map_location=self.device, weights_only=True)
        wrote = ck.get("algo", "PPO")
        if wrote != self.ALGO:
            raise ValueError(f"{self._who}.load: {path} was written by {wrote}, not by {self.ALGO} (the built algorithms are "
                             f"{' and '.join(ALGOS)}; each loads its own checkpoints only)")
        self._load_optimizer_state(ck["optimizer"])                     # checks the layout before anything is changed
        self.policy.load_state_dict(ck["policy"])                       # copies in place: the parameters stay views of flat_p
        self.policy._sample_rows = int(ck["optimizer"]["sampling_rows"])
        if self._encoder is not None:
            self._encoder._step_seed = int(ck["optimizer"].get("enc_step_seed", self._encoder._step_seed))
        for k, v in ck["hyper"].items():
            setattr(self, k, v)
        if "generator" in ck:                                           # a resumed learn() draws the permutations and the actions the saved
            self.generator.set_state(ck["generator"].cpu())             # run would have drawn next; older files leave both streams alone
            self.policy._sample_seed = int(self.seed) & (2 ** 64 - 1)
        return self


__all__ = ["OnPolicyAlgorithm", "RolloutBuffer", "RolloutBatch"]
