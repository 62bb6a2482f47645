"""DQN's replay buffer on the device: a ring of vec steps that stores every observation once.

``ReplayBuffer`` restates what stable-baselines3 1.5's ``ReplayBuffer`` does with ``optimize_memory_usage=True`` from the published
algorithm (Mnih et al. 2015): none of its text is copied.  Slot ``t`` holds one step of all ``n_envs`` environments; the observation
that step led to is slot ``(t + 1) % N``'s, which the next ``add`` rewrites with the same tensor.  Storage and the position arithmetic are
pure indexing and work on any device; ``sample`` is ``ocrl_replay_sample`` + ``ocrl_replay_gather`` (include/ocrl_hip_dqn.h: two
launches, no host read) and needs the GPU."""
import collections
import math

import torch

from .. import _bridge, _lib
from .on_policy import _tensor

_WHO = "ocrl_amd.sb3s.ReplayBuffer"
ReplayBatch = collections.namedtuple("ReplayBatch", "observations next_observations actions rewards dones")


class ReplayBuffer:
    """``N = max(2, buffer_size // n_envs)`` slots of one vec step each in tensors [N, E, ...] on ``device``; observations stay in the
    dtype they arrive in (``obs_dtype``; uint8 frames stay uint8).  ``pos`` is the slot the next ``add`` writes, ``full`` whether the ring
    has wrapped.  A slot is a valid transition when its own and its successor's observation are stored: slots ``0 .. pos - 1`` before the
    wrap, every slot but ``pos`` after it.  ``seed`` names the sampling stream: ``sample(B, update)`` is a pure function of it and
    ``update``."""

    def __init__(self, buffer_size, n_envs, obs_shape, device="cuda", obs_dtype=torch.float32, seed=0):
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

    def __len__(self):
        """transitions that can be sampled"""
        return (self.n_slots - 1 if self.full else self.pos) * self.n_envs

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

    def sample_indices(self, batch_size, update):
        """transition ids ``t * E + e`` int64 [batch_size] of update ``update`` (ocrl_replay_sample)"""
        if self.device.type != "cuda":
            raise RuntimeError(f"{_WHO}.sample: the buffer must live on the GPU (there is no CPU fallback)")
        if not self.full and self.pos < 1:
            raise RuntimeError(f"{_WHO}.sample: the buffer holds no transition yet")
        idx = torch.empty(int(batch_size), device=self.device, dtype=torch.int64)
        _bridge.launch(self.device, _lib.lib().ocrl_replay_sample, self.seed, int(update) & (2 ** 64 - 1), int(batch_size), self.n_slots, self.n_envs,
                       self.pos, int(self.full), _lib.ptr(idx))
        return idx

    def gather(self, idx):
        """the transitions ``idx`` (int64 ids ``t * E + e``, clamped into range) as a ReplayBatch of fresh device tensors (ocrl_replay_gather)"""
        if self.device.type != "cuda":
            raise RuntimeError(f"{_WHO}.sample: the buffer must live on the GPU (there is no CPU fallback)")
        idx = idx.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        B = idx.numel()
        obs, nxt = (torch.empty(B, *self.obs_shape, device=self.device, dtype=self.observations.dtype) for _ in range(2))
        actions = torch.empty(B, device=self.device, dtype=torch.int64)
        rewards = torch.empty(B, device=self.device, dtype=torch.float32)
        dones = torch.empty(B, device=self.device, dtype=torch.uint8)
        _bridge.launch(self.device, _lib.lib().ocrl_replay_gather, _lib.ptr(self.observations), _lib.ptr(self.actions), _lib.ptr(self.rewards),
                       _lib.ptr(self.dones), self.n_slots, self.n_envs, self.obs_bytes, _lib.ptr(idx), B, _lib.ptr(obs), _lib.ptr(nxt),
                       _lib.ptr(actions), _lib.ptr(rewards), _lib.ptr(dones))
        return ReplayBatch(obs, nxt, actions, rewards, dones)

    def sample(self, batch_size, update):
        """``batch_size`` valid transitions of update ``update``: two launches, device tensors, no host read"""
        return self.gather(self.sample_indices(batch_size, update))


__all__ = ["ReplayBuffer", "ReplayBatch"]
