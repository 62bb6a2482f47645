"""CPU-only checks of the on-device pre-training scenes' host side: the epoch's index lists (ocrl_amd/utils/device_scenes.py:
epoch_indices), two hand-worked scenes of the numpy restatement (tests/scenes_ref.py, the reference the GPU tests hold the kernel to),
the C entry points' rejections, and the dataset.on_device switch of get_dataloaders."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from ocrl_amd.utils.config import compose
from ocrl_amd.utils.datasets import get_dataloaders
from ocrl_amd.utils.device_scenes import DeviceScenes, epoch_indices
from tests import scenes_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
F = np.float32


# ---------------------------------------------------------------------------------------------------------------- epoch_indices
@pytest.mark.parametrize("world", [1, 2, 3])
def test_ranks_are_disjoint_and_cover_the_permutations_head(world):
    n, bs = 23, 2
    perm = epoch_indices(n, 7, 4, 0, 1, 1, True).flatten()
    assert perm.dtype == torch.int64 and sorted(perm.tolist()) == list(range(n))
    per_rank = [epoch_indices(n, 7, 4, r, world, bs, True, drop_last=False) for r in range(world)]
    flat = [torch.cat(b) for b in per_rank]
    for r in range(world):
        assert torch.equal(flat[r], perm[:n - n % world][r::world])
    union = torch.cat(flat)
    assert len(set(union.tolist())) == len(union) == n - n % world
    assert set(union.tolist()) == set(perm[:n - n % world].tolist())


def test_same_seed_and_epoch_same_order_another_epoch_another_order():
    a = epoch_indices(100, 3, 5, 0, 1, 10, True)
    assert a.shape == (10, 10) and a.dtype == torch.int64 and a.device.type == "cpu"
    assert torch.equal(a, epoch_indices(100, 3, 5, 0, 1, 10, True))
    b = epoch_indices(100, 3, 6, 0, 1, 10, True)
    assert not torch.equal(a, b) and sorted(b.flatten().tolist()) == list(range(100))
    assert not torch.equal(a, epoch_indices(100, 4, 5, 0, 1, 10, True))


def test_without_shuffle_the_indices_count_up():
    assert torch.equal(epoch_indices(12, 9, 3, 0, 1, 4, False), torch.arange(12).view(3, 4))
    assert torch.equal(epoch_indices(12, 9, 3, 1, 2, 3, False), torch.tensor([[1, 3, 5], [7, 9, 11]]))


def test_drop_last_and_the_ragged_last_batch():
    full = epoch_indices(10, 0, 0, 0, 1, 4, False)
    assert full.shape == (2, 4) and torch.equal(full.flatten(), torch.arange(8))
    ragged = epoch_indices(10, 0, 0, 0, 1, 4, False, drop_last=False)
    assert [b.tolist() for b in ragged] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert len(DeviceScenes(10, 16, 0, 4, "cuda:0", drop_last=True)) == 2 and len(DeviceScenes(10, 16, 0, 4, "cuda:0")) == 3
    assert len(DeviceScenes(10, 16, 0, 4, "cuda:0", rank=1, world=3)) == 1              # 9 of 10 scenes, 3 to a rank


# ---------------------------------------------------------------------------------------------------------------- scenes by hand
def test_a_second_object_too_close_to_the_first_takes_its_second_candidate():
    """object 0: scale index below(2) at 0 = 0, so [a, b] = [0.155, 0.845]; the candidate (.1, .1) lies at (0.224, 0.224), far from the
    middle; shape below(4) at .3 = 1, colour at .8 = 3.  Object 1: scale 0; the candidate (.15, .15) lies 0.049 from object 0 and is
    rejected, (.9, .1) at (0.776, 0.224) stands; shape at .6 = 2, colour at .1 = 0.  12 draws."""
    u = np.array([0, .1, .1, .3, .8, 0, .15, .15, .9, .1, .6, .1], dtype=np.float64)
    u = (np.floor(u * 2 ** 24) / 2 ** 24).astype(np.float32)
    objs, centres, used, exhausted = S.scene(u, K=2)
    a, b, r = S.interval(0)
    assert (a, b, r) == (F(F(0.075) + F(0.08)), F(F(F(1) - F(0.075)) - F(0.08)), F(0.075)) and r == F(F(0.15) * F(0.5))
    at = lambda v: F(a + F(F(b - a) * F(v)))
    assert used == 12 and exhausted == []
    assert objs[0].tolist() == [3, 1, 0, at(u[1]), at(u[2])] and objs[1].tolist() == [0, 2, 0, at(u[8]), at(u[9])]
    assert abs(float(objs[0, 3]) - 0.224) < 1e-6 and abs(float(objs[1, 3]) - 0.776) < 1e-6
    assert S.dist(at(u[6]), at(u[7]), objs[0, 3], objs[0, 4]) < F(0.15)              # the rejected candidate
    assert np.array_equal(centres, np.array([[objs[0, 3], objs[0, 4], F(0.15)], [objs[1, 3], objs[1, 4], F(0.15)]], dtype=np.float32))
    with pytest.raises(IndexError):
        S.scene(u[:11], K=2)                                                          # every one of the 12 is taken
    assert np.array_equal(S.rows(objs)[:, 2], [F(0.15), F(0.15)]) and np.array_equal(S.rows(objs)[:, [0, 1, 3, 4]], objs[:, [0, 1, 3, 4]])


def test_uniforms_that_always_hit_the_middle_leave_the_64th_candidate():
    """scale index 1 (.5): [a, b] = [0.19, 0.81], whose middle is .5: all 64 candidates lie within 0.15 of (0.5, 0.5), the last one (a
    little off, to tell it from the others) stands; shape at .3 = 1, colour at .8 = 3.  1 + 128 + 2 draws."""
    u = np.array([.5] + [.5] * 126 + [.51, .49] + [.3, .8], dtype=np.float64)
    u = (np.floor(u * 2 ** 24) / 2 ** 24).astype(np.float32)
    objs, centres, used, exhausted = S.scene(u, K=1)
    a, b, _ = S.interval(1)
    assert used == 131 and exhausted == [0]
    assert objs[0].tolist() == [3, 1, 1, F(a + F(F(b - a) * u[127])), F(a + F(F(b - a) * u[128]))]
    assert objs[0, 3] != objs[0, 4] and S.dist(F(0.5), F(0.5), objs[0, 3], objs[0, 4]) < F(0.15) and centres[0, 2] == F(0.22)
    assert S.MAX_DRAWS == 15 * 131 < 2 ** 16


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_the_entry_points_exist_and_reject_with_a_message():
    from ocrl_amd import _lib
    L = _lib.lib()
    assert L.ocrl_abi_version() == 5 and ctypes.sizeof(_lib.ScenesDesc) == 8
    some = (ctypes.c_longlong * 4)()                   # never read: every call below is refused before a launch
    idx, out = ctypes.cast(some, ctypes.c_void_p), ctypes.cast(some, ctypes.c_void_p)

    def rejected(rc, *words):
        msg = L.ocrl_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)
    ok = _lib.ScenesDesc(H=16, K=5)
    rejected(L.ocrl_scenes_batch(None, 0, idx, 1, None, None, None, out, None), "ocrl_scenes_batch", "null descriptor")
    for H in (4, 10, 516, -8):
        rejected(L.ocrl_scenes_batch(_lib.ScenesDesc(H=H, K=5), 0, idx, 1, None, None, None, out, None), "obs_size", "[8, 512]", str(H))
    for K in (0, 16, -1):
        rejected(L.ocrl_scenes_batch(_lib.ScenesDesc(H=16, K=K), 0, idx, 1, None, None, None, out, None), "objects", "15", str(K))
    for B in (0, -3):
        rejected(L.ocrl_scenes_batch(ok, 0, idx, B, None, None, None, out, None), "batch >= 1", str(B))
    rejected(L.ocrl_scenes_batch(ok, 0, None, 1, None, None, None, out, None), "null indices")
    rejected(L.ocrl_scenes_batch(ok, 0, idx, 1, None, None, None, None, None), "no output", "obs, obs_u8, masks and objs")
    rejected(L.ocrl_scenes_batch(ok, 0, idx, 1, ctypes.c_void_p(out.value + 4), None, None, None, None), "16-byte aligned")
    # 512 rows are 256 bands of 2: 2^23 scenes are 2^31 workgroups
    rejected(L.ocrl_scenes_batch(_lib.ScenesDesc(H=512, K=1), 0, idx, 1 << 23, None, None, None, out, None), "exceed one launch", "8388608")
    rejected(L.ocrl_scenes_uniforms(0, 0, 0, 4, None, None), "ocrl_scenes_uniforms", "null output")
    rejected(L.ocrl_scenes_uniforms(0, 0, 0, 0, out, None), "ocrl_scenes_uniforms", "n < 1")
    rejected(L.ocrl_scenes_uniforms(0, 0, 65536 - 3, 4, out, None), "ocrl_scenes_uniforms", "2^16")
    rejected(L.ocrl_scenes_uniforms(0, 0, -1, 4, out, None), "ocrl_scenes_uniforms", "2^16")


# ---------------------------------------------------------------------------------------------------------------- get_dataloaders
def dataset_cfg(*over):
    return compose(CFG, "train_ocr", ["ocr=slate", "dataset=random-N5C4S4S2", "dataset.synthetic_train=16", "dataset.synthetic_val=8", *over]).dataset


def test_the_config_composes_with_the_switch():
    assert dataset_cfg().on_device is False and dataset_cfg("dataset.on_device=True").on_device is True


def test_on_device_needs_a_cuda_device_and_no_data_file(tmp_path):
    c = dataset_cfg("dataset.on_device=True")
    with pytest.raises(ValueError, match="on_device.*CUDA"):
        get_dataloaders(c, 4, 0)
    with pytest.raises(ValueError, match="on_device.*CUDA"):
        get_dataloaders(c, 4, 0, device="cpu")
    f = tmp_path / "scenes.hdf5"
    f.write_bytes(b"")
    with pytest.raises(ValueError, match="on_device.*datadir"):
        get_dataloaders(dataset_cfg("dataset.on_device=True", f"dataset.datadir={f}"), 4, 0, device="cuda:0")
    with pytest.raises(ValueError, match="CUDA"):
        DeviceScenes(8, 16, 0, 4, "cpu")
    # a CUDA device: the two loaders, made without touching the device
    tr, va = get_dataloaders(dataset_cfg("dataset.on_device=True", "dataset.with_masks=True"), 4, 8, rank=1, world=2, seed=3, device="cuda:0")
    assert isinstance(tr, DeviceScenes) and isinstance(va, DeviceScenes)
    assert (tr.n, tr.seed, tr.shuffle, tr.drop_last, tr.rank, tr.world, tr.with_masks, tr.with_objs, tr.size) == (16, 7, True, True, 1, 2, True, False, 64)
    assert (va.n, va.seed, va.shuffle, va.drop_last, va.rank, va.world, va.with_masks, va.num_objs) == (8, 8, False, False, 0, 1, True, 5)
    assert len(tr) == 2 and len(va) == 2 and len(tr.dataset) == 16 and tr.sampler is tr and hasattr(tr.sampler, "set_epoch")


def test_without_the_key_the_host_loaders_come_back():
    for c in (dataset_cfg(), dataset_cfg("dataset.on_device=False")):
        tr, va = get_dataloaders(c, 4, 0, device="cuda:0")
        assert type(tr) is DataLoader and type(va) is DataLoader
        assert next(iter(tr))["obss_u8"].shape == (4, 64, 64, 3) and len(va.dataset) == 8
    from ocrl_amd.utils.config import Config
    c = Config({k: v for k, v in dataset_cfg().to_dict().items() if k != "on_device"})       # a config file from before the key
    assert "on_device" not in c and type(get_dataloaders(c, 4, 0)[0]) is DataLoader
