"""CPU-only checks of the task datasets' host side (the first frames of the sprite tasks' episodes, ocrl_task_scenes_batch): the symbol
and its declaration, the entry point's rejections (a host pointer, no launch), the three dataset configs and the `- /env@task: name`
defaults form that builds them, and the routing of get_dataloaders to DeviceTaskScenes."""
import ctypes
import os
import re

import pytest
import torch
from torch.utils.data import DataLoader

from ocrl_amd.utils.config import compose
from ocrl_amd.utils.datasets import get_dataloaders
from ocrl_amd.utils.device_scenes import DeviceScenes, DeviceTaskScenes, _DeviceLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
NAMES = ["target-N4C4S3S1", "odd-one-out-N4C2S2S1", "odd-one-out-N4C2S2S1-oc"]


def dataset_cfg(name, *over):
    return compose(CFG, "train_ocr", ["ocr=slate", f"dataset={name}", "dataset.synthetic_train=16", "dataset.synthetic_val=8", *over]).dataset


def env_cfg(name, *over):
    return compose(CFG, "train_sb3", ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", f"env={name}", *over]).env


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_the_symbol_is_exported_and_declared():
    from ocrl_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "ocrl_task_scenes_batch") and len(L.ocrl_task_scenes_batch.argtypes) == 10
    header = open(os.path.join(ROOT, "include", "ocrl_hip.h")).read()
    decl = re.search(r"int ocrl_task_scenes_batch\((.*?)\);", header, re.S)
    assert decl and re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).count(",") == 9 and "const ocrl_sprite_env_desc* d" in decl.group(1) and "long long* labels" in decl.group(1)
    assert header.index("int ocrl_scenes_uniforms(") < decl.start()                   # next to the scenes block


def test_the_entry_point_rejects_with_a_message():
    from ocrl_amd import _lib, envs
    L = _lib.lib()
    some = (ctypes.c_longlong * 4)()                   # never read: every call below is refused before a launch
    idx, out = ctypes.cast(some, ctypes.c_void_p), ctypes.cast(some, ctypes.c_void_p)
    assert out.value % 8 == 0

    def rejected(rc, *words):
        msg = L.ocrl_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)

    def desc(name="target-N4C4S3S1", **fields):
        d = envs.env_desc(env_cfg(name), 1)
        for k, v in fields.items():
            setattr(d, k, v)
        return d
    call = L.ocrl_task_scenes_batch
    rejected(call(None, 0, idx, 1, None, None, None, out, None, None), "ocrl_task_scenes_batch", "null descriptor")
    # the descriptor is the environment's: what ocrl_sprite_env_reset refuses is refused here, in its words
    rejected(call(desc(task=2), 0, idx, 1, None, None, None, out, None, None), "ocrl_task_scenes_batch", "task 0 (Target) or 1 (Odd-One-Out)")
    for H in (4, 10, 516):
        rejected(call(desc(H=H), 0, idx, 1, None, None, None, out, None, None), "obs_size", "[8, 512]", str(H))
    rejected(call(desc(E=0), 0, idx, 1, None, None, None, out, None, None), "environments", "(got 0)")
    rejected(call(desc(max_steps=0), 0, idx, 1, None, None, None, out, None, None), "max_steps >= 1")
    rejected(call(desc(hi=16), 0, idx, 1, None, None, None, out, None, None), "num_objects_range", "15")
    rejected(call(desc(mode=0, lo=1), 0, idx, 1, None, None, None, out, None, None), "easy mode")
    rejected(call(desc(obj_comp=1), 0, idx, 1, None, None, None, out, None, None), "obj_comp and unseen_mode belong to task 1")
    rejected(call(desc("odd-one-out-N4C2S2S1", lo=2), 0, idx, 1, None, None, None, out, None, None), "Odd-One-Out needs num_objects_range lo >= 3")
    ok = desc()
    for B in (0, -3):
        rejected(call(ok, 0, idx, B, None, None, None, out, None, None), "batch >= 1", str(B))
    rejected(call(ok, 0, None, 1, None, None, None, out, None, None), "null indices")
    rejected(call(ok, 0, idx, 1, None, None, None, None, None, None), "no output", "obs, obs_u8, masks, objs and labels")
    off = lambda n: ctypes.c_void_p(out.value + n)
    base16 = out.value % 16                            # out is 8-byte aligned: make one pointer that is 16-byte aligned and shift it
    al16 = ctypes.c_void_p(out.value + (16 - base16) % 16)
    rejected(call(ok, 0, idx, 1, ctypes.c_void_p(al16.value + 4), None, None, None, None, None), "16-byte aligned")
    rejected(call(ok, 0, idx, 1, None, None, ctypes.c_void_p(al16.value + 8), None, None, None), "16-byte aligned")
    rejected(call(ok, 0, idx, 1, None, off(2), None, None, None, None), "obs_u8 4-byte aligned")
    # 512 rows are 256 bands of 2: 2^23 scenes are 2^31 workgroups
    rejected(call(desc(H=512), 0, idx, 1 << 23, None, None, None, out, None, None), "exceed one launch", "8388608")


# ---------------------------------------------------------------------------------------------------------------- configs
@pytest.mark.parametrize("name", NAMES)
def test_the_dataset_configs_compose_and_carry_the_env_file(name):
    c = dataset_cfg(name)
    assert c.task.to_dict() == env_cfg(name).to_dict()                                # key for key
    assert c.on_device is True and c.with_masks is False and c.with_objs is False and c.tags == name and c.name and c.datadir is None
    assert (c.synthetic_train, c.synthetic_val) == (16, 8) and c.obs_size == 64
    assert list(c.property_order_in_state) == ["color", "shape", "scale", "xy"]     # what the probe reads of a dataset config
    raw = compose(CFG, "train_ocr", ["ocr=slate", f"dataset={name}"]).dataset
    assert (raw.synthetic_train, raw.synthetic_val) == (100000, 1000)
    assert dataset_cfg(name, "dataset.task.num_objects_range=[3,4]").task.num_objects_range == [3, 4]


def test_an_absolute_group_in_a_defaults_list_lands_under_its_package(tmp_path):
    (tmp_path / "env").mkdir(), (tmp_path / "dataset").mkdir()
    (tmp_path / "env" / "_b.yaml").write_text("x: 1\ny: 2\n")
    (tmp_path / "env" / "e.yaml").write_text("defaults:\n  - _b\n  - _self_\ny: 3\n")
    (tmp_path / "dataset" / "d.yaml").write_text("defaults:\n  - /env@task: e\n  - /env: e\n  - _self_\nz: 4\ntask:\n  x: 7\n")
    (tmp_path / "dataset" / "bad.yaml").write_text("defaults:\n  - /env@task: ???\n")
    (tmp_path / "top.yaml").write_text("defaults:\n  - dataset: ???\n  - _self_\n")
    c = compose(str(tmp_path), "top", ["dataset=d", "dataset.task.y=5"])
    assert c.dataset.to_dict() == {"task": {"x": 7, "y": 5}, "env": {"x": 1, "y": 3}, "z": 4}
    with pytest.raises(ValueError, match="/env"):
        compose(str(tmp_path), "top", ["dataset=bad"])
    with pytest.raises(FileNotFoundError):
        (tmp_path / "dataset" / "gone.yaml").write_text("defaults:\n  - /env@task: nope\n")
        compose(str(tmp_path), "top", ["dataset=gone"])


# ---------------------------------------------------------------------------------------------------------------- get_dataloaders
@pytest.mark.parametrize("name", NAMES)
def test_get_dataloaders_returns_the_task_loader(name):
    c = dataset_cfg(name, "dataset.with_masks=True", "dataset.obs_size=16")
    tr, va = get_dataloaders(c, 4, 8, rank=1, world=2, seed=3, device="cuda:0")       # made without touching the device
    assert type(tr) is DeviceTaskScenes and type(va) is DeviceTaskScenes
    assert (tr.n, tr.seed, tr.shuffle, tr.drop_last, tr.rank, tr.world, tr.with_masks, tr.with_objs, tr.size) == (16, 7, True, True, 1, 2, True, False, 16)
    assert (va.n, va.seed, va.shuffle, va.drop_last, va.rank, va.world, va.with_masks, va.with_objs, va.size) == (8, 8, False, False, 0, 1, True, False, 16)
    assert len(tr) == 2 and len(va) == 2 and len(tr.dataset) == 16 and tr.sampler is tr and hasattr(tr.sampler, "set_epoch")
    d = tr._desc
    assert (d.H, d.lo, d.hi, d.task, d.obj_comp) == (16, 4, 4, int(name != NAMES[0]), int(name == NAMES[2])) and c.task.obs_size == 64
    assert isinstance(tr, _DeviceLoader) and issubclass(DeviceScenes, _DeviceLoader)  # one base
    assert DeviceTaskScenes.__iter__ is DeviceScenes.__iter__ and DeviceTaskScenes.__len__ is DeviceScenes.__len__


def test_what_the_task_loader_refuses(tmp_path):
    c = dataset_cfg(NAMES[0])
    with pytest.raises(ValueError, match="dataset.on_device"):
        get_dataloaders(dataset_cfg(NAMES[0], "dataset.on_device=False"), 4, 0, device="cuda:0")
    with pytest.raises(ValueError, match="on_device.*CUDA"):
        get_dataloaders(c, 4, 0)
    with pytest.raises(ValueError, match="on_device.*CUDA"):
        get_dataloaders(c, 4, 0, device="cpu")
    from ocrl_amd import envs
    with pytest.raises(ValueError, match="CUDA"):
        DeviceTaskScenes(envs.env_desc(c.task, 1), 8, 0, 4, "cpu")
    ragged = dataset_cfg(NAMES[0], "dataset.with_objs=True", "dataset.task.num_objects_range=[1,3]")
    with pytest.raises(ValueError, match="num_objects_range"):
        get_dataloaders(ragged, 4, 0, device="cuda:0")
    tr, _ = get_dataloaders(dataset_cfg(NAMES[0], "dataset.task.num_objects_range=[1,3]"), 4, 0, device="cuda:0")      # without objs: fine
    assert (tr._desc.lo, tr._desc.hi) == (1, 3)
    assert get_dataloaders(dataset_cfg(NAMES[0], "dataset.with_objs=True"), 4, 0, device="cuda:0")[0].with_objs is True
    # the environment's refusals apply: the descriptor is env_desc's
    with pytest.raises(NotImplementedError, match="agent_pos"):
        get_dataloaders(dataset_cfg(NAMES[0], "dataset.task.agent_pos=null"), 4, 0, device="cuda:0")
    with pytest.raises(NotImplementedError, match="use_bg"):
        get_dataloaders(dataset_cfg(NAMES[1], "dataset.task.background.use_bg=True"), 4, 0, device="cuda:0")
    with pytest.raises(ValueError, match="pentagon"):
        get_dataloaders(dataset_cfg(NAMES[1], "dataset.task.SHAPES=[square,pentagon]"), 4, 0, device="cuda:0")
    with pytest.raises(ValueError, match="obs_size"):
        get_dataloaders(dataset_cfg(NAMES[0], "dataset.obs_size=18"), 4, 0, device="cuda:0")
    # an existing data file: on the device it contradicts on_device as for the random scenes; without on_device it is read as HDF5
    f = tmp_path / "frames.hdf5"
    f.write_bytes(b"")
    with pytest.raises(ValueError, match="on_device.*datadir"):
        get_dataloaders(dataset_cfg(NAMES[0], f"dataset.datadir={f}"), 4, 0, device="cuda:0")
    with pytest.raises(Exception) as e:                                              # h5py, or its absence, gets the file: not the task loader
        get_dataloaders(dataset_cfg(NAMES[0], "dataset.on_device=False", f"dataset.datadir={f}"), 4, 0, device="cuda:0")
    assert "on_device" not in str(e.value)


def test_the_random_scenes_still_come_from_where_they_did():
    rnd = lambda *o: compose(CFG, "train_ocr", ["ocr=slate", "dataset=random-N5C4S4S2", "dataset.synthetic_train=16", "dataset.synthetic_val=8", *o]).dataset
    assert "task" not in rnd()
    tr, va = get_dataloaders(rnd(), 4, 0, device="cuda:0")
    assert type(tr) is DataLoader and type(va) is DataLoader and next(iter(tr))["obss_u8"].shape == (4, 64, 64, 3)
    tr, va = get_dataloaders(rnd("dataset.on_device=True"), 4, 0, seed=3, device="cuda:0")
    assert type(tr) is DeviceScenes and type(va) is DeviceScenes and (tr.n, tr.seed, tr.num_objs, va.seed) == (16, 7, 5, 8)
    with pytest.raises(ValueError, match="DeviceScenes: obs_size"):
        DeviceScenes(8, 18, 0, 4, "cuda:0")
    assert torch.device("cuda:0") == tr.device
