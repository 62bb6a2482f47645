"""DQN's replay buffer on the device: a ring of vec steps that stores every observation once.

``ReplayBuffer`` restates what stable-baselines3 1.5's ``ReplayBuffer`` does with ``optimize_memory_usage=True`` from the published
algorithm (Mnih et al. 2015): none of its text is copied.  Slot ``t`` holds one step of all ``n_envs`` environments; the observation
that step led to is slot ``(t + 1) % N``'s, which the next ``add`` rewrites with the same tensor.  Storage and the position arithmetic are
pure indexing and work on any device; ``sample`` is ``ocrl_replay_sample`` + ``ocrl_replay_gather`` (include/ocrl_hip_dqn.h: two
launches, no host read) and needs the GPU.

The extensions of include/ocrl_hip_replay.h sit on the same ring: ``n_step`` returns are read from the slots that follow a transition
(``ocrl_replay_sample_nstep`` + ``ocrl_replay_gather_nstep``), and ``prioritized=True`` keeps a proportional priority store beside it
(4 bytes per transition and the sums above them; ``ocrl_per_*``), which ``add`` keeps valid without a host read."""
import collections
import math

import torch

from .. import _bridge, _lib
from .on_policy import _tensor

_WHO = "ocrl_amd.sb3s.ReplayBuffer"
# ``discounts`` is gamma^m of an n-step read (the factor of the bootstrap), None for the plain one-step read
ReplayBatch = collections.namedtuple("ReplayBatch", "observations next_observations actions rewards dones discounts", defaults=(None,))
MAX_N_STEP = 16


class ReplayBuffer:
    """``N = max(2, buffer_size // n_envs)`` slots of one vec step each in tensors [N, E, ...] on ``device``; observations stay in the
    dtype they arrive in (``obs_dtype``; uint8 frames stay uint8).  ``pos`` is the slot the next ``add`` writes, ``full`` whether the ring
    has wrapped.  A slot is a valid transition when its own and its successor's observation are stored: slots ``0 .. pos - 1`` before the
    wrap, every slot but ``pos`` after it.  ``seed`` names the sampling stream: ``sample(B, update)`` is a pure function of it and
    ``update``.

    ``n_step`` is the window the buffer keeps whole: a slot then counts as a transition when the ``n_step`` steps from it on and the
    observation after them are stored (``len()``, ``sample_indices``' default reach, the priority store's sampleable leaves).
    ``prioritized`` adds the priority store (``priorities``, a uint8 buffer in the layout of include/ocrl_hip_replay.h): ``add`` zeroes
    the leaves of the slot the next write goes to and gives those of the slot whose window just became whole the running maximum."""

    def __init__(self, buffer_size, n_envs, obs_shape, device="cuda", obs_dtype=torch.float32, seed=0, prioritized=False, n_step=1):
        self.n_envs, self.obs_shape = int(n_envs), tuple(int(s) for s in obs_shape)
        self.n_slots = max(2, int(buffer_size) // self.n_envs)
        self.device, self.seed = torch.device(device), int(seed) & (2 ** 64 - 1)
        N, E = self.n_slots, self.n_envs
        self.obs_bytes = math.prod(self.obs_shape) * torch.empty(0, dtype=obs_dtype).element_size()
        if self.obs_bytes % 4:
            raise ValueError(f"{_WHO}: an observation of shape {self.obs_shape} and dtype {obs_dtype} is {self.obs_bytes} bytes, not a multiple of 4")
        if N * E >= 2 ** 31:
            raise ValueError(f"{_WHO}: {N} slots of {E} environments leave the int32 range of transition ids")
        self.observations = torch.empty(N, E, *self.obs_shape, device=self.device, dtype=obs_dtype)
        self.actions = torch.empty(N, E, device=self.device, dtype=torch.int64)
        self.rewards = torch.empty(N, E, device=self.device, dtype=torch.float32)
        self.dones = torch.empty(N, E, device=self.device, dtype=torch.uint8)
        self.pos, self.full = 0, False
        self.n_step, self.prioritized = int(n_step), bool(prioritized)
        if not 1 <= self.n_step <= MAX_N_STEP or self.n_step >= N:
            raise ValueError(f"{_WHO}: n_step must lie in 1 .. {MAX_N_STEP} and below the {N} slots of the ring (got {n_step})")
        self.priorities = None
        if self.prioritized:
            if self.device.type != "cuda":
                raise RuntimeError(f"{_WHO}: the priority store lives on the GPU (there is no CPU fallback)")
            nbytes = _lib.lib().ocrl_per_bytes(N * E)
            if nbytes == 0:
                _lib.check(1)
            self.priorities = torch.empty(nbytes // 8, device=self.device, dtype=torch.int64).view(torch.uint8)      # 8-byte aligned
            _bridge.launch(self.device, _lib.lib().ocrl_per_init, _lib.ptr(self.priorities), N * E)

    def __len__(self):
        """transitions that can be sampled: slots whose ``n_step`` window is stored, times the environments"""
        return (self.n_slots - self.n_step if self.full else max(self.pos - self.n_step + 1, 0)) * self.n_envs

    def add(self, obs, next_obs, actions, rewards, dones):
        """one step of every environment: obs, next_obs [E, ...], the others [E].  A finished environment's next_obs is whatever the
        environment returned (its next episode's first frame where it resets inside the step): the TD target selects on ``dones`` and
        never reads it."""
        t, E = self.pos, self.n_envs
        nxt = (t + 1) % self.n_slots
        self.observations[t].copy_(_tensor(obs, self.device).reshape(E, *self.obs_shape))
        self.observations[nxt].copy_(_tensor(next_obs, self.device).reshape(E, *self.obs_shape))
        self.actions[t].copy_(_tensor(actions, self.device).reshape(E))
        self.rewards[t].copy_(_tensor(rewards, self.device).reshape(E))
        self.dones[t].copy_(_tensor(dones, self.device).reshape(E).ne(0))
        self.pos = nxt
        self.full = self.full or nxt == 0
        if self.prioritized:
            # slot nxt is about to be rewritten: not sampleable.  Slot nxt - n_step has its whole window and the observation after it
            # stored now (once it has been written at all): it enters with the largest priority seen so far
            self._set_range(nxt, 0)
            if self.full or nxt >= self.n_step:
                self._set_range((nxt - self.n_step) % self.n_slots, 1)

    def _set_range(self, slot, mode):
        E = self.n_envs
        _bridge.launch(self.device, _lib.lib().ocrl_per_set_range, _lib.ptr(self.priorities), self.n_slots * E, slot * E, E, mode)

    def sample_indices(self, batch_size, update, n_step=1):
        """transition ids ``t * E + e`` int64 [batch_size] of update ``update`` (ocrl_replay_sample; ``n_step`` > 1: among the slots whose
        ``n_step`` window is stored, ocrl_replay_sample_nstep)"""
        if self.device.type != "cuda":
            raise RuntimeError(f"{_WHO}.sample: the buffer must live on the GPU (there is no CPU fallback)")
        n = int(n_step)
        if not self.full and self.pos < n:
            raise RuntimeError(f"{_WHO}.sample: the buffer holds no transition yet" if n == 1 else
                               f"{_WHO}.sample: the buffer holds {self.pos} steps, no whole window of n_step = {n} yet")
        idx = torch.empty(int(batch_size), device=self.device, dtype=torch.int64)
        if n == 1:
            _bridge.launch(self.device, _lib.lib().ocrl_replay_sample, self.seed, int(update) & (2 ** 64 - 1), int(batch_size), self.n_slots,
                           self.n_envs, self.pos, int(self.full), _lib.ptr(idx))
        else:
            _bridge.launch(self.device, _lib.lib().ocrl_replay_sample_nstep, self.seed, int(update) & (2 ** 64 - 1), int(batch_size), self.n_slots,
                           self.n_envs, self.pos, int(self.full), n, _lib.ptr(idx))
        return idx

    def sample_prioritized(self, batch_size, update, beta):
        """(ids int64 [batch_size], importance weights fp32 [batch_size]) of update ``update``, drawn in proportion to the stored
        priorities (ocrl_per_sample: two launches, no host read); the weights are (q_min / q)^beta, 1 for the batch's rarest row"""
        if self.priorities is None:
            raise RuntimeError(f"{_WHO}.sample_prioritized: the buffer was built without prioritized=True")
        if len(self) == 0:
            raise RuntimeError(f"{_WHO}.sample_prioritized: the buffer holds no whole window of n_step = {self.n_step} yet")
        idx = torch.empty(int(batch_size), device=self.device, dtype=torch.int64)
        weights = torch.empty(int(batch_size), device=self.device, dtype=torch.float32)
        _bridge.launch(self.device, _lib.lib().ocrl_per_sample, _lib.ptr(self.priorities), self.n_slots * self.n_envs, self.seed,
                       int(update) & (2 ** 64 - 1), int(batch_size), float(beta), None, _lib.ptr(idx), _lib.ptr(weights))
        return idx, weights

    def update_priorities(self, idx, abs_td, alpha, eps):
        """the priorities of the transitions ``idx`` become (|td| + eps)^alpha (ocrl_per_update: one launch); ids that are not sampleable
        stay so"""
        if self.priorities is None:
            raise RuntimeError(f"{_WHO}.update_priorities: the buffer was built without prioritized=True")
        idx = idx.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        abs_td = abs_td.detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        if abs_td.numel() != idx.numel():
            raise ValueError(f"{_WHO}.update_priorities: {abs_td.numel()} errors for {idx.numel()} ids")
        _bridge.launch(self.device, _lib.lib().ocrl_per_update, _lib.ptr(self.priorities), self.n_slots * self.n_envs, _lib.ptr(idx), _lib.ptr(abs_td),
                       idx.numel(), float(alpha), float(eps))

    def gather(self, idx, n_step=1, gamma=None):
        """the transitions ``idx`` (int64 ids ``t * E + e``, clamped into range) as a ReplayBatch of fresh device tensors
        (ocrl_replay_gather).  With ``gamma`` given (any ``n_step``) the read is ocrl_replay_gather_nstep's: ``rewards`` holds the
        discounted return of up to ``n_step`` steps, cut at the first done, ``next_observations`` the observation after them, ``dones``
        whether the walk ended on a done and ``discounts`` the factor gamma^m of the bootstrap."""
        if self.device.type != "cuda":
            raise RuntimeError(f"{_WHO}.sample: the buffer must live on the GPU (there is no CPU fallback)")
        if int(n_step) != 1 and gamma is None:
            raise ValueError(f"{_WHO}.gather: an n-step read (n_step = {n_step}) needs gamma")
        idx = idx.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        B = idx.numel()
        obs, nxt = (torch.empty(B, *self.obs_shape, device=self.device, dtype=self.observations.dtype) for _ in range(2))
        actions = torch.empty(B, device=self.device, dtype=torch.int64)
        rewards = torch.empty(B, device=self.device, dtype=torch.float32)
        dones = torch.empty(B, device=self.device, dtype=torch.uint8)
        if gamma is not None:
            discounts = torch.empty(B, device=self.device, dtype=torch.float32)
            _bridge.launch(self.device, _lib.lib().ocrl_replay_gather_nstep, _lib.ptr(self.observations), _lib.ptr(self.actions),
                           _lib.ptr(self.rewards), _lib.ptr(self.dones), self.n_slots, self.n_envs, self.obs_bytes, int(n_step), float(gamma),
                           _lib.ptr(idx), B, _lib.ptr(obs), _lib.ptr(nxt), _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones), _lib.ptr(discounts))
            return ReplayBatch(obs, nxt, actions, rewards, dones, discounts)
        _bridge.launch(self.device, _lib.lib().ocrl_replay_gather, _lib.ptr(self.observations), _lib.ptr(self.actions), _lib.ptr(self.rewards),
                       _lib.ptr(self.dones), self.n_slots, self.n_envs, self.obs_bytes, _lib.ptr(idx), B, _lib.ptr(obs), _lib.ptr(nxt),
                       _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones))
        return ReplayBatch(obs, nxt, actions, rewards, dones)

    def sample(self, batch_size, update):
        """``batch_size`` valid transitions of update ``update``: two launches, device tensors, no host read"""
        return self.gather(self.sample_indices(batch_size, update))


__all__ = ["ReplayBuffer", "ReplayBatch"]
