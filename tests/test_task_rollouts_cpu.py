"""CPU-only checks of the task datasets' later frames (ocrl_task_scenes_rollout_batch, include/ocrl_hip_rollout.h): the third header
parses and its function is bound while the other two tables stay what they were; every refusal the entry point makes before a launch (on
host pointers that are never read); the two dataset keys and their defaults; and the routing of get_dataloaders, where only_initial=True
builds exactly the first-frame loader.  The walk's restatement (tests/task_rollout_ref.py) is checked on hand-made episodes."""
import ctypes
import os
import re

import numpy as np
import pytest

from ocrl_amd import _abi, _lib
from ocrl_amd.utils.config import compose
from ocrl_amd.utils.datasets import get_dataloaders
from ocrl_amd.utils.device_scenes import DeviceTaskScenes
from tests import sprite_env_ref as R
from tests import task_rollout_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
NAMES = ["target-N4C4S3S1", "odd-one-out-N4C2S2S1", "odd-one-out-N4C2S2S1-oc"]
NAME = "ocrl_task_scenes_rollout_batch"


def dataset_cfg(name, *over):
    return compose(CFG, "train_ocr", ["ocr=slate", f"dataset={name}", "dataset.synthetic_train=16", "dataset.synthetic_val=8", *over]).dataset


def env_cfg(name, *over):
    return compose(CFG, "train_sb3", ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", f"env={name}", *over]).env


def header():
    return open(os.path.join(ROOT, "include", "ocrl_hip_rollout.h")).read()


# ---------------------------------------------------------------------------------------------------------------- header and binding
def test_the_header_parses_and_its_function_is_bound():
    abi = _abi.read(header())
    assert {n: len(a) for n, (_, a) in abi.functions.items()} == {NAME: 13} and abi.consts == {} and abi.structs == {}
    ret, args = abi.functions[NAME]
    V, I = ctypes.c_void_p, ctypes.c_int
    assert ret is I and args == [V, ctypes.c_ulonglong, V, V, I, I, V, V, V, V, V, V, V]
    assert set(_lib.ABI_ROLLOUT.functions) == {NAME}
    # the other tables are their own headers' alone
    assert len(_lib.ABI.functions) == 146 and NAME not in _lib.ABI.functions and NAME not in _lib.ABI_DQN.functions
    f = getattr(_lib.lib(), NAME)
    assert f.argtypes == args and f.restype is I
    # the dialect: an #ifndef guard, self-contained (the reader follows no #include "..."), the descriptor as const void*
    text = header()
    assert "#pragma once" not in text and re.search(r"^#ifndef OCRL_HIP_ROLLOUT_H$", text, re.M) and "#include <stddef.h>" in text
    assert not re.search(r'#include\s+"', text) and "const void* desc" in text and "ocrl_sprite_env_desc" in text
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    assert "ocrl_hip_rollout.h" in makefile


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_the_entry_point_rejects_with_a_message_naming_the_argument():
    from ocrl_amd import envs
    L = _lib.lib()
    call = getattr(L, NAME)
    some = (ctypes.c_longlong * 4)()                   # never read: every call below is refused before a launch
    idx, out = ctypes.cast(some, ctypes.c_void_p), ctypes.cast(some, ctypes.c_void_p)

    def rejected(rc, *words):
        msg = L.ocrl_last_error().decode()
        assert rc != 0 and all(w in msg for w in (NAME,) + words), (rc, msg)

    def desc(name="target-N4C4S3S1", **fields):
        d = envs.env_desc(env_cfg(name), 1)
        for k, v in fields.items():
            setattr(d, k, v)
        return ctypes.byref(d)
    ok = desc()
    for m in (-1, 256, 1000):                          # steps null: the step is drawn in [0, max_step]
        rejected(call(ok, 0, idx, None, m, 1, None, None, None, out, None, None, None), "max_step", "[0, 255]", str(m))
    rejected(call(ok, 0, None, None, 5, 1, None, None, None, out, None, None, None), "null indices")
    rejected(call(ok, 0, None, idx, 5, 1, None, None, None, out, None, None, None), "null indices")
    for B in (0, -3):
        rejected(call(ok, 0, idx, None, 5, B, None, None, None, out, None, None, None), "batch >= 1", str(B))
        rejected(call(ok, 0, idx, idx, 5, B, None, None, None, out, None, None, None), "batch >= 1", str(B))
    # a bad descriptor: what ocrl_task_scenes_batch refuses, in its words
    rejected(call(None, 0, idx, None, 5, 1, None, None, None, out, None, None, None), "null descriptor")
    rejected(call(desc(task=2), 0, idx, None, 5, 1, None, None, None, out, None, None, None), "task 0 (Target) or 1 (Odd-One-Out)")
    for H in (4, 10, 516):
        rejected(call(desc(H=H), 0, idx, None, 5, 1, None, None, None, out, None, None, None), "obs_size", "[8, 512]", str(H))
    rejected(call(desc(E=0), 0, idx, None, 5, 1, None, None, None, out, None, None, None), "environments", "(got 0)")
    rejected(call(desc(max_steps=0), 0, idx, None, 5, 1, None, None, None, out, None, None, None), "max_steps >= 1")
    rejected(call(desc(hi=16), 0, idx, None, 5, 1, None, None, None, out, None, None, None), "num_objects_range", "15")
    rejected(call(desc(mode=0, lo=1), 0, idx, None, 5, 1, None, None, None, out, None, None, None), "easy mode")
    rejected(call(desc(obj_comp=1), 0, idx, None, 5, 1, None, None, None, out, None, None, None), "obj_comp and unseen_mode belong to task 1")
    rejected(call(desc("odd-one-out-N4C2S2S1", lo=2), 0, idx, None, 5, 1, None, None, None, out, None, None, None), "Odd-One-Out needs num_objects_range lo >= 3")
    # the outputs
    rejected(call(ok, 0, idx, None, 5, 1, None, None, None, None, None, None, None), "no output", "labels and steps_taken")
    al16 = ctypes.c_void_p(out.value + (16 - out.value % 16) % 16)
    rejected(call(ok, 0, idx, None, 5, 1, ctypes.c_void_p(al16.value + 4), None, None, None, None, None, None), "16-byte aligned")
    rejected(call(ok, 0, idx, None, 5, 1, None, None, ctypes.c_void_p(al16.value + 8), None, None, None, None), "16-byte aligned")
    rejected(call(ok, 0, idx, None, 5, 1, None, ctypes.c_void_p(out.value + 2), None, None, None, None, None), "obs_u8 4-byte aligned")
    rejected(call(desc(H=512), 0, idx, None, 5, 1 << 23, None, None, None, out, None, None, None), "exceed one launch", "8388608")
    # the first-frame entry point words its refusals as before
    assert L.ocrl_task_scenes_batch(ok, 0, idx, 1, None, None, None, None, None, None) != 0
    msg = L.ocrl_last_error().decode()
    assert "ocrl_task_scenes_batch: no output requested (obs, obs_u8, masks, objs and labels are all null)" in msg


# ---------------------------------------------------------------------------------------------------------------- configs and routing
@pytest.mark.parametrize("name", NAMES)
def test_the_dataset_keys_and_their_defaults(name):
    c = dataset_cfg(name)
    assert c.only_initial is True and c.rollout_steps is None
    c = dataset_cfg(name, "dataset.only_initial=False")
    assert c.only_initial is False and c.rollout_steps is None
    tr, va = get_dataloaders(c, 4, 0, rank=1, world=2, seed=3, device="cuda:0")       # made without touching the device
    assert type(tr) is DeviceTaskScenes and type(va) is DeviceTaskScenes
    assert c.task.max_steps == 100 and tr.rollout_steps == va.rollout_steps == 99     # task.max_steps - 1: the last step an episode can show
    assert (tr.n, tr.seed, tr.shuffle, tr.drop_last, tr.rank, tr.world) == (16, 7, True, True, 1, 2)
    assert (va.n, va.seed, va.shuffle, va.drop_last, va.rank, va.world) == (8, 8, False, False, 0, 1)
    long = get_dataloaders(dataset_cfg(name, "dataset.only_initial=False", "dataset.task.max_steps=1000"), 4, 0, device="cuda:0")[0]
    assert long.rollout_steps == 255                                                   # capped: the drawn step has 8 bits
    assert get_dataloaders(dataset_cfg(name, "dataset.only_initial=False", "dataset.task.max_steps=1"), 4, 0, device="cuda:0")[0].rollout_steps == 0
    own = get_dataloaders(dataset_cfg(name, "dataset.only_initial=False", "dataset.rollout_steps=7"), 4, 0, device="cuda:0")
    assert own[0].rollout_steps == own[1].rollout_steps == 7
    for bad in (-1, 256):
        with pytest.raises(ValueError, match=r"rollout_steps.*\[0, 255\]"):
            get_dataloaders(dataset_cfg(name, "dataset.only_initial=False", f"dataset.rollout_steps={bad}"), 4, 0, device="cuda:0")


@pytest.mark.parametrize("name", NAMES)
def test_only_initial_builds_exactly_the_first_frame_loader(name):
    from ocrl_amd.utils.config import Config
    for c in (dataset_cfg(name), dataset_cfg(name, "dataset.only_initial=True", "dataset.rollout_steps=7"),
              Config({k: v for k, v in dataset_cfg(name).to_dict().items() if k not in ("only_initial", "rollout_steps")})):   # a config from before the keys
        tr, va = get_dataloaders(c, 4, 8, rank=1, world=2, seed=3, device="cuda:0")
        assert type(tr) is DeviceTaskScenes and type(va) is DeviceTaskScenes and tr.rollout_steps is None and va.rollout_steps is None
        assert (tr.n, tr.seed, tr.shuffle, tr.drop_last, tr.rank, tr.world, tr.with_masks, tr.with_objs, tr.size) == (16, 7, True, True, 1, 2, False, False, 64)
        assert (va.n, va.seed, va.shuffle, va.drop_last, va.rank, va.world, va.with_masks, va.with_objs, va.size) == (8, 8, False, False, 0, 1, False, False, 64)


def test_the_loaders_own_refusals():
    from ocrl_amd import envs
    d = envs.env_desc(env_cfg(NAMES[0]), 1)
    assert DeviceTaskScenes(d, 8, 0, 4, "cuda:0").rollout_steps is None
    assert DeviceTaskScenes(d, 8, 0, 4, "cuda:0", rollout_steps=0).rollout_steps == 0
    assert DeviceTaskScenes(d, 8, 0, 4, "cuda:0", rollout_steps=255).rollout_steps == 255
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="rollout_steps"):
            DeviceTaskScenes(d, 8, 0, 4, "cuda:0", rollout_steps=bad)
    with pytest.raises(ValueError, match="CUDA"):
        DeviceTaskScenes(d, 8, 0, 4, "cpu", rollout_steps=3)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def hand_episode(positions, target=0):
    """uniforms that make a hard-mode Target episode of 4 objects at the given centres (no placement is rejected)"""
    s = R.spec()
    a, b = np.float32(np.float32(np.float32(0) + np.float32(0.075)) + np.float32(0.08)), np.float32(np.float32(np.float32(1) - np.float32(0.075)) - np.float32(0.08))
    u = [0.0, target / 4 + 0.01]                                  # n = 4 (one count), the target index
    for i in range(4):
        if i != target:
            u += [0.3, 0.4, 0.0]                                  # colour 1, shape 1, the one scale: not the target's triple
    for x, y in positions:
        u += [(x - float(a)) / float(b - a), (y - float(a)) / float(b - a)]
    return s, np.asarray(u + [0.5] * 8, dtype=np.float32)


def test_the_walk_stops_before_the_step_that_ends_the_episode():
    d = _desc_like(R.spec())
    s, u = hand_episode([(0.5, 0.82), (0.2, 0.2), (0.8, 0.2), (0.2, 0.8)])
    rows = R.reset(s, u)[0]
    assert np.allclose(rows[:4, 3:], [(0.5, 0.82), (0.2, 0.2), (0.8, 0.2), (0.2, 0.8)], atol=1e-6) and tuple(rows[4, 3:]) == (0.5, 0.5)
    up, left, down, right = 0.1, 0.3, 0.6, 0.8                    # uniforms of the four actions
    assert W.actions([up, left, down, right, 0.0, 0.249999, 0.25, 0.999999]) == [0, 1, 2, 3, 0, 0, 1, 3]
    # up: 0.55, 0.60, 0.65 are 0.27, 0.22, 0.17 from the object at (0.5, 0.82); the fourth step, 0.70, is within agent_scale = 0.15 of it
    frames, L = W.walk(d, u, [up] * 10)
    env = R.Env(s, lambda k: u)
    dones = [env.step(0)[1] for _ in range(L)]
    assert dones == [False] * (L - 1) + [True] and L == 4 and len(frames) == L
    assert [tuple(f[4, 3:]) for f in frames[:3]] == [(np.float32(0.5), np.float32(0.5)), (np.float32(0.5), np.float32(0.5) + np.float32(0.05)),
                                                      (np.float32(0.5), np.float32(np.float32(0.5) + np.float32(0.05)) + np.float32(0.05))]
    assert all(np.array_equal(f[:4], rows[:4]) for f in frames)  # only the agent moves
    for t, want in ((0, 0), (1, 1), (L - 1, L - 1), (L, L - 1), (50, L - 1), (-3, 0), (1000, L - 1)):
        got, taken = W.scene(frames, L, t, 100)
        assert taken == want and got is frames[want]
    # left and right cancel: the walk is cut by the time limit alone, at step max_steps; frame max_steps - 1 is the last one shown
    d.max_steps = 12
    frames, L = W.walk(d, u, [left, right] * 10)
    assert L == 12 and len(frames) == 12 and W.scene(frames, L, 20, 12)[1] == 11
    # the actions run out before the episode ends
    d.max_steps = 100
    frames, L = W.walk(d, u, [left, right] * 3)
    assert L is None and len(frames) == 7 and W.scene(frames, L, 6, 100)[1] == 6
    with pytest.raises(IndexError):
        W.scene(frames, L, 7, 100)
    # the wall: 20 steps left from 0.5 stop at r_agent
    frames, L = W.walk(d, hand_episode([(0.5, 0.8), (0.8, 0.8), (0.8, 0.2), (0.5, 0.2)])[1], [left] * 20)
    assert L is None and frames[-1][4, 3] == np.float32(0.15) * np.float32(0.5) and frames[-1][4, 4] == np.float32(0.5)
    assert W.drawn_step(0.0, 99) == 0 and W.drawn_step(0.999999, 99) == 99 and W.drawn_step(0.5, 0) == 0 and W.drawn_step(0.5, 255) == 128


def _desc_like(s):
    """a SpriteEnvDesc of the Target task with the numbers of a sprite_env_ref.spec()"""
    d = _lib.SpriteEnvDesc(E=1, H=16, lo=s.lo, hi=s.hi, mode=s.mode, rew_type=s.rew_type, occlusion=int(s.occlusion), max_steps=s.max_steps,
                           n_colors=len(s.colors), n_shapes=len(s.shapes), n_scales=len(s.scales), target_color=s.target[0], target_shape=s.target[1],
                           target_scale=s.target[2], agent_color=s.agent[0], agent_shape=s.agent[1], agent_scale=s.agent[2], agent_x=s.agent_pos[0],
                           agent_y=s.agent_pos[1], step_size=s.step_size, dist_agent=s.dist_agent, dist_objs=s.dist_objs, dist_wall=s.dist_wall)
    for i, v in enumerate(s.colors):
        d.colors[i] = v
    for i, v in enumerate(s.shapes):
        d.shapes[i] = v
    for i, v in enumerate(s.scales):
        d.scales[i] = v
    return d
