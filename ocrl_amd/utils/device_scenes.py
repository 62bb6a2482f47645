"""The pre-training scenes made on the GPU (include/ocrl_hip.h: ocrl_scenes_*): a loader with a DataLoader's surface whose batches never
exist on the host.  Scene i of a seed is a function of (seed, i) alone, so an epoch is a list of indices: the host shuffles and shards
integers (``epoch_indices``, pure torch), uploads them once per epoch, and every batch is one ocrl_scenes_batch call on the current
stream.  Nothing is read back.  Same distribution and draw order as ocrl_amd/utils/data.py:random_sprite_scenes, not numpy's bit stream:
dataset.on_device=True trains on other scenes of the same kind than the host loader does."""
import ctypes

import torch

from .. import _bridge, _lib


def _rank_indices(n, seed, epoch, rank, world, shuffle):
    """the scene indices rank `rank` of `world` sees in epoch `epoch`, in order: elements rank::world of the first n - n % world of the
    epoch's permutation (shuffle: torch.randperm from a CPU generator seeded by (seed, epoch); else arange)"""
    n, world, rank = int(n), int(world), int(rank)
    if n < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_indices: n >= 1 and 0 <= rank < world (got n {n}, rank {rank}, world {world})")
    if shuffle:
        g = torch.Generator()
        g.manual_seed((int(seed) * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
        order = torch.randperm(n, generator=g)
    else:
        order = torch.arange(n, dtype=torch.int64)
    return order[:n - n % world][rank::world].contiguous()


def epoch_indices(n, seed, epoch, rank, world, batch_size, shuffle, drop_last=True):
    """-> CPU int64 [batches, batch_size]: the batches of one rank's epoch, the incomplete last one dropped.  drop_last=False keeps it:
    then a list of 1-D tensors, the last of which may be shorter"""
    idx, bs = _rank_indices(n, seed, epoch, rank, world, shuffle), int(batch_size)
    if bs < 1:
        raise ValueError(f"epoch_indices: batch_size >= 1 (got {bs})")
    if drop_last:
        return idx[:len(idx) - len(idx) % bs].view(-1, bs)
    return list(idx.split(bs))


class _Scenes:
    """the `.dataset` of a DeviceScenes: scene i of the seed, as a one-scene batch without its batch dimension"""

    def __init__(self, loader):
        self._loader = loader

    def __len__(self):
        return self._loader.n

    def __getitem__(self, i):
        i = int(i)
        if not -self._loader.n <= i < self._loader.n:
            raise IndexError(f"scene {i} of {self._loader.n}")
        idx = torch.tensor([i % self._loader.n], dtype=torch.int64).to(self._loader.device)
        return {k: v[0] for k, v in self._loader.batch(idx).items()}


class _DeviceLoader:
    """what the on-device loaders share: the surface train_ocr.py uses of a DataLoader (len() = batches, .dataset, .sampler.set_epoch) and
    an epoch as a list of indices, shuffled and sharded on the host, uploaded once, one ``batch(idx)`` call per batch"""

    def __init__(self, n, size, seed, batch_size, device, with_masks, with_objs, shuffle, drop_last, rank, world):
        who = type(self).__name__
        self.device = torch.device(device) if device is not None else None
        if self.device is None or self.device.type != "cuda":
            raise ValueError(f"{who}: the scenes are made on a CUDA device (got device={device!r})")
        self.n, self.size, self.seed, self.batch_size = int(n), int(size), int(seed), int(batch_size)
        self.with_masks, self.with_objs, self.shuffle, self.drop_last = bool(with_masks), bool(with_objs), bool(shuffle), bool(drop_last)
        self.rank, self.world, self.epoch = int(rank), int(world), 0
        self._check()
        _rank_indices(self.n, 0, 0, self.rank, self.world, False)            # the same refusals as an epoch's, before the first one
        if self.batch_size < 1:
            raise ValueError(f"{who}: batch_size >= 1 (got {self.batch_size})")
        self.dataset, self.sampler = _Scenes(self), self

    def _check(self):
        """the subclass's own refusals, raised before the index rules'"""

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        per_rank = (self.n - self.n % self.world) // self.world
        return per_rank // self.batch_size if self.drop_last else -(-per_rank // self.batch_size)

    def __iter__(self):
        idx = _rank_indices(self.n, self.seed, self.epoch, self.rank, self.world, self.shuffle).to(self.device)    # one upload per epoch
        if self.shuffle:
            self.epoch += 1                # a pass that no set_epoch precedes takes the next order, as a shuffling DataLoader's would
        bs = self.batch_size
        for b in range(len(self)):
            yield self.batch(idx[b * bs:(b + 1) * bs])


class DeviceScenes(_DeviceLoader):
    """an iterable of batches {"obss": fp32 [B,3,H,W], "masks": [B,K+1,H,W,1] (with_masks), "objs": [B,K,5] (with_objs)} of fresh
    tensors on `device`, with the surface train_ocr.py uses of a DataLoader: len() = batches, .dataset, .sampler.set_epoch"""

    def __init__(self, n, size, seed, batch_size, device, num_objs=5, with_masks=False, with_objs=False, shuffle=False, drop_last=False,
                 rank=0, world=1):
        self.num_objs = int(num_objs)
        super().__init__(n, size, seed, batch_size, device, with_masks, with_objs, shuffle, drop_last, rank, world)
        self._desc = _lib.ScenesDesc(H=self.size, K=self.num_objs)

    def _check(self):
        if not (8 <= self.size <= 512 and self.size % 4 == 0 and 1 <= self.num_objs <= 15):
            raise ValueError(f"DeviceScenes: obs_size a multiple of 4 in [8, 512] and 1 to 15 objects (got {self.size}, {self.num_objs})")

    def batch(self, idx):
        """the scenes of idx (int64 [B] on the device, contiguous) as one ocrl_scenes_batch call on the current stream"""
        B, H, K = idx.shape[0], self.size, self.num_objs
        obs = torch.empty(B, 3, H, H, dtype=torch.float32, device=self.device)
        masks = torch.empty(B, K + 1, H, H, dtype=torch.float32, device=self.device) if self.with_masks else None
        objs = torch.empty(B, K, 5, dtype=torch.float32, device=self.device) if self.with_objs else None
        _bridge.launch(self.device, _lib.lib().ocrl_scenes_batch, self._desc, self.seed & 0xFFFFFFFFFFFFFFFF, _lib.ptr(idx), B, _lib.ptr(obs), None,
                       _lib.ptr(masks), _lib.ptr(objs))
        out = {"obss": obs}
        if masks is not None:
            out["masks"] = masks.unsqueeze(-1)
        if objs is not None:
            out["objs"] = objs
        return out


class DeviceTaskScenes(_DeviceLoader):
    """frames of a sprite task's episodes (``desc`` from ocrl_amd.envs.env_desc, its H the frame size): batches {"obss": fp32 [B,3,H,W],
    "masks": [B,hi+2,H,W,1] (with_masks: each row alone, the agent's after the objects', the background last), "objs": [B,hi+1,5] and
    "labels": int64 [B,1], the target's row (with_objs)}.  Scene i is episode i of environment 0 of the seed's streams.
    rollout_steps=None: its first frame (ocrl_task_scenes_batch), what a vectorised environment of that seed shows when it starts that
    episode.  rollout_steps=T, an integer in [0, 255]: one frame of that episode at a step drawn uniformly in [0, T] from the episode's own
    stream, reached under a uniform random policy (ocrl_task_scenes_rollout_batch, include/ocrl_hip_rollout.h): still a function of (seed, i)
    alone, and never a terminal frame -- an episode that ends sooner gives its last frame before the end."""

    def __init__(self, desc, n, seed, batch_size, device, with_masks=False, with_objs=False, shuffle=False, drop_last=False, rank=0, world=1,
                 rollout_steps=None):
        self._desc = desc
        self.rollout_steps = None if rollout_steps is None else int(rollout_steps)
        super().__init__(n, desc.H, seed, batch_size, device, with_masks, with_objs, shuffle, drop_last, rank, world)

    def _check(self):
        d = self._desc
        if not (8 <= self.size <= 512 and self.size % 4 == 0):
            raise ValueError(f"DeviceTaskScenes: obs_size a multiple of 4 in [8, 512] (got {self.size})")
        if self.with_objs and d.lo != d.hi:
            raise ValueError(f"DeviceTaskScenes: with_objs needs num_objects_range [lo, hi] with lo == hi (got [{d.lo}, {d.hi}]): the zero row "
                             "after the agent of a smaller episode would be matched as an object")
        if self.n > 1 << 24:
            raise ValueError(f"DeviceTaskScenes: at most 2^24 scenes, the episodes of one environment's stream (got {self.n})")
        if self.rollout_steps is not None and not 0 <= self.rollout_steps <= 255:
            raise ValueError(f"DeviceTaskScenes: rollout_steps is None (first frames) or an integer in [0, 255] (got {self.rollout_steps})")

    def batch(self, idx, steps=None):
        """the scenes of idx (int64 [B] on the device, contiguous) as one call on the current stream: ocrl_task_scenes_batch for first
        frames, ocrl_task_scenes_rollout_batch at a drawn step (rollout_steps) or at ``steps`` (int32 [B] on the device, contiguous:
        frame steps[b] of episode idx[b], whatever rollout_steps is)"""
        B, H, R = idx.shape[0], self.size, self._desc.hi + 1
        obs = torch.empty(B, 3, H, H, dtype=torch.float32, device=self.device)
        masks = torch.empty(B, R + 1, H, H, dtype=torch.float32, device=self.device) if self.with_masks else None
        objs = torch.empty(B, R, 5, dtype=torch.float32, device=self.device) if self.with_objs else None
        labels = torch.empty(B, 1, dtype=torch.int64, device=self.device) if self.with_objs else None
        seed = self.seed & 0xFFFFFFFFFFFFFFFF
        if steps is None and self.rollout_steps is None:
            _bridge.launch(self.device, _lib.lib().ocrl_task_scenes_batch, self._desc, seed, _lib.ptr(idx), B, _lib.ptr(obs), None, _lib.ptr(masks),
                           _lib.ptr(objs), _lib.ptr(labels))
        else:
            if steps is not None and (steps.dtype != torch.int32 or steps.shape != (B,) or steps.device != idx.device or not steps.is_contiguous()):
                raise ValueError(f"DeviceTaskScenes.batch: steps is a contiguous int32 [{B}] tensor beside idx (got {steps.dtype} {tuple(steps.shape)} on {steps.device})")
            _bridge.launch(self.device, _lib.lib().ocrl_task_scenes_rollout_batch, ctypes.byref(self._desc), seed, _lib.ptr(idx), _lib.ptr(steps),
                           self.rollout_steps or 0, B, _lib.ptr(obs), None, _lib.ptr(masks), _lib.ptr(objs), _lib.ptr(labels), None)
        out = {"obss": obs}
        if masks is not None:
            out["masks"] = masks.unsqueeze(-1)
        if objs is not None:
            out["objs"], out["labels"] = objs, labels
        return out
