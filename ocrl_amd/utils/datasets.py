"""Datasets for train_ocr.py.  Same sample content as the reference's utils/datasets.py:8-27 ("obss", optional "masks" [K+1,H,W,1] with
the background last).  Reads the reference's HDF5 when h5py and the file are available, otherwise generates random-N5C4S4S2-style
scenes deterministically per index.  With raw_uint8 (the default of get_dataloaders) a sample carries the image as the dataset stores
it — "obss_u8", uint8 HWC — and the permute + /255 of utils/datasets.py:17 runs on the GPU (ocrl_obs_u8_to_f32) after a 4x smaller
upload; raw_uint8=False gives the reference's float CHW "obss".  With dataset.on_device the synthetic scenes never exist on the host:
device_scenes.py makes each batch on the GPU; so it does the task datasets (target-*, odd-one-out-*), the first frames of the sprite
tasks' episodes or (dataset.only_initial=False) frames from later steps of a random walk, which exist on the device only."""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .data import random_sprite_scenes


class SyntheticScenes(Dataset):
    def __init__(self, n, size, seed=0, with_masks=False, num_objs=5, raw_uint8=False, with_objs=False):
        self.n, self.size, self.seed, self.with_masks, self.num_objs = int(n), int(size), int(seed), bool(with_masks), num_objs
        self.raw_uint8, self.with_objs = bool(raw_uint8), bool(with_objs)

    def _obs(self, img):
        if self.raw_uint8:
            return {"obss_u8": torch.from_numpy(img)}
        return {"obss": torch.from_numpy(img).permute(2, 0, 1).float() / 255.0}

    def __len__(self):
        return self.n

    def __getitem__(self, index):
        s = (self.seed * 1000003 + index) & 0x7FFFFFFF
        if self.with_objs:                                # "objs" [num_objs, 5], the key H5DataSet forwards from the reference's files
            res = random_sprite_scenes(1, self.size, seed=s, num_objs=self.num_objs, with_masks=self.with_masks, with_objs=True)
            sample = {**self._obs(res[0][0]), "objs": torch.from_numpy(res[-1][0])}
            if self.with_masks:
                sample["masks"] = torch.from_numpy(res[1][0])
            return sample
        if self.with_masks:
            img, m = random_sprite_scenes(1, self.size, seed=s, num_objs=self.num_objs, with_masks=True)
            return {**self._obs(img[0]), "masks": torch.from_numpy(m[0])}
        img = random_sprite_scenes(1, self.size, seed=s, num_objs=self.num_objs)
        return self._obs(img[0])


class H5DataSet(Dataset):
    """utils/datasets.py:8-27"""

    def __init__(self, data, raw_uint8=False):
        self._data = data
        self._num_samples = data["obss"].shape[0]
        # the raw path uploads the stored bytes; it is taken only when the file really stores uint8 (the reference's
        # torch.Tensor(x) / 255 accepts any dtype, a blind uint8 cast would wrap or truncate other storage types)
        self._raw_uint8 = bool(raw_uint8) and np.dtype(data["obss"].dtype) == np.uint8

    def __getitem__(self, index):
        res = {}
        for key in self._data.keys():
            if key == "obss" and self._raw_uint8:
                res["obss_u8"] = torch.from_numpy(np.ascontiguousarray(self._data[key][index]))
            elif key == "obss":
                res[key] = torch.Tensor(self._data[key][index]).permute(2, 0, 1) / 255.0
            elif key == "labels":
                res[key] = torch.LongTensor([self._data[key][index]])
            elif key != "num_objs":
                res[key] = torch.Tensor(self._data[key][index])
        return res

    def __len__(self):
        return self._num_samples


def _device_loaders(config, batch_size, rank, world, seed, device, datafile):
    """dataset.on_device: the synthetic scenes made on `device` batch by batch (device_scenes.py); no worker, no upload"""
    from .device_scenes import DeviceScenes
    if datafile and os.path.isfile(datafile):
        raise ValueError(f"dataset.on_device generates the scenes, but dataset.datadir {datafile} exists: unset one of the two keys")
    if device is None or torch.device(device).type != "cuda":
        raise ValueError(f"dataset.on_device needs the CUDA device the model trains on (got device={device!r})")
    if config.get("task") is not None:
        return _task_loaders(config, batch_size, rank, world, seed, device)
    kw = dict(num_objs=5, with_masks=bool(config.get("with_masks", False)), with_objs=bool(config.get("with_objs", False)))
    train = DeviceScenes(config.get("synthetic_train", 100000), config.obs_size, seed * 2 + 1, batch_size, device, shuffle=True, drop_last=True,
                         rank=rank, world=world, **kw)
    val = DeviceScenes(config.get("synthetic_val", 1000), config.obs_size, seed * 2 + 2, batch_size, device, **kw)
    return train, val


def _task_loaders(config, batch_size, rank, world, seed, device):
    """a dataset config with a `task` mapping (an env config): frames of that task's episodes (device_scenes.py: DeviceTaskScenes).  The
    descriptor is the environment's, so every refusal of ocrl_amd.envs applies; the frame size is the dataset's.  dataset.only_initial
    (default True): the first frame of every episode; False: one frame per episode at a step drawn in [0, dataset.rollout_steps] of a
    uniform random policy's walk (default task.max_steps - 1, the last step an episode can show, capped at 255)"""
    from ..envs import env_desc
    from .device_scenes import DeviceTaskScenes
    desc = env_desc(config.task, 1)
    desc.H = int(config.obs_size)
    kw = dict(with_masks=bool(config.get("with_masks", False)), with_objs=bool(config.get("with_objs", False)))
    if not config.get("only_initial", True):
        steps = config.get("rollout_steps", None)
        kw["rollout_steps"] = min(int(config.task.max_steps) - 1, 255) if steps is None else int(steps)
    train = DeviceTaskScenes(desc, config.get("synthetic_train", 100000), seed * 2 + 1, batch_size, device, shuffle=True, drop_last=True, rank=rank,
                             world=world, **kw)
    val = DeviceTaskScenes(desc, config.get("synthetic_val", 1000), seed * 2 + 2, batch_size, device, **kw)
    return train, val


def get_dataloaders(config, batch_size, num_workers, rank=0, world=1, seed=0, raw_uint8=True, device=None):
    """utils/tools.py:155-178 without the wandb download path; with dataset.on_device the scenes are made on `device` and num_workers
    is ignored.  A config with a `task` mapping (configs/dataset/target-*.yaml, odd-one-out-*.yaml) is a sprite task's first frames: made
    on the device, or read from its datadir file; there is no host generator for them"""
    datafile = config.datadir if config.get("datadir") else None
    if config.get("on_device", False):
        return _device_loaders(config, batch_size, rank, world, seed, device, datafile)
    if config.get("task") is not None and not (datafile and os.path.isfile(datafile)):
        raise ValueError(f"dataset {config.get('name')}: a task's frames are made on the GPU only: set dataset.on_device=True, or dataset.datadir to "
                         "an existing HDF5 file")
    if datafile and os.path.isfile(datafile):
        try:
            import h5py
        except ImportError as e:
            raise RuntimeError(f"{datafile} exists but h5py is not installed") from e
        f = h5py.File(datafile, "r")
        train, val = H5DataSet(f["TrainingSet"], raw_uint8), H5DataSet(f["ValidationSet"], raw_uint8)
    else:
        wm, wo = bool(config.get("with_masks", False)), bool(config.get("with_objs", False))
        train = SyntheticScenes(config.get("synthetic_train", 100000), config.obs_size, seed=seed * 2 + 1, with_masks=wm, raw_uint8=raw_uint8,
                                with_objs=wo)
        val = SyntheticScenes(config.get("synthetic_val", 1000), config.obs_size, seed=seed * 2 + 2, with_masks=wm, raw_uint8=raw_uint8,
                              with_objs=wo)
    sampler = None
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(train, num_replicas=world, rank=rank, shuffle=True, seed=seed, drop_last=True)
    train_dl = DataLoader(train, batch_size, num_workers=num_workers, shuffle=(sampler is None), sampler=sampler, drop_last=True)
    val_dl = DataLoader(val, batch_size)
    return train_dl, val_dl
