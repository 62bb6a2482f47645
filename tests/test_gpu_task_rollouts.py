"""GPU checks of the task datasets' later frames (ocrl_task_scenes_rollout_batch, include/ocrl_hip_rollout.h;
DeviceTaskScenes(rollout_steps=...), dataset.only_initial=False): an episode walked t steps under the uniform random policy.

Bounds.  Everything is exact: bit for bit and byte for byte, no tolerance.  Step 0 is compared with ocrl_task_scenes_batch; later steps with
a vectorised environment of the same seed that is handed the walk's own actions (read back through ocrl_sprite_env_uniforms), frame by
frame and row by row, and with the numpy restatement (tests/task_rollout_ref.py, which imports the stepping of tests/sprite_env_ref.py and
tests/oddoneout_ref.py) for where each episode ends.  The pixels are compared with entry points that predate the dataset
(ocrl_sprite_render, ocrl_obs_u8_to_f32).  Every output buffer starts as NaN / 77 / -1, so an element the kernel leaves out fails."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import task_rollout_ref as W
from tests.gpu_util import log
from tests.test_gpu_task_scenes import (BATCHES, CFG, DEV, ROOT, SEEDS, TASKS, desc_of, env_config, generate, indices, raw_rows, reference, same_bits,
                                        sprite_render, state_rows, uniforms)

pytestmark = pytest.mark.gpu

NAMES = ("obs", "u8", "masks", "objs", "labels", "taken")
ENV_TASKS = ["target-hard-44", "target-easy-24", "ooo-N4C2S2S1"]
WALK_SEED = SEEDS[1]             # chosen so that, in each of ENV_TASKS, the 32 episodes of test 2 hold both kinds the test asserts it has


def rollout(d, seed, idx, steps=None, max_step=0, obs=True, u8=True, masks=True, objs=True, labels=True, taken=True):
    """one ocrl_task_scenes_rollout_batch call -> dict of the requested outputs (device tensors), prefilled with NaN / 77 / -1.
    steps: a list or tensor of B step counts, or None for the drawn mode with max_step"""
    import ctypes
    from ocrl_amd import _bridge, _lib
    idx = torch.as_tensor(idx, dtype=torch.int64).to(DEV)
    st = None if steps is None else torch.as_tensor(steps, dtype=torch.int32).to(DEV).contiguous()
    B, H, R_ = idx.shape[0], d.H, d.hi + 1
    assert st is None or st.shape == (B,)
    out = {}
    if obs:
        out["obs"] = torch.full((B, 3, H, H), math.nan, dtype=torch.float32, device=DEV)
    if u8:
        out["u8"] = torch.full((B, H, H, 3), 77, dtype=torch.uint8, device=DEV)
    if masks:
        out["masks"] = torch.full((B, R_ + 1, H, H), math.nan, dtype=torch.float32, device=DEV)
    if objs:
        out["objs"] = torch.full((B, R_, 5), math.nan, dtype=torch.float32, device=DEV)
    if labels:
        out["labels"] = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    if taken:
        out["taken"] = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _bridge.launch(torch.device(DEV), _lib.lib().ocrl_task_scenes_rollout_batch, ctypes.byref(d), seed, _lib.ptr(idx), _lib.ptr(st), max_step, B,
                   _lib.ptr(out.get("obs")), _lib.ptr(out.get("u8")), _lib.ptr(out.get("masks")), _lib.ptr(out.get("objs")), _lib.ptr(out.get("labels")),
                   _lib.ptr(out.get("taken")))
    return out


def walk_uniforms(seed, envs, first, n):
    """draws first .. first + n - 1 of episode 0 of environments 0 .. envs - 1 -> device fp32 [envs, n]"""
    from ocrl_amd import _bridge, _lib
    out = torch.full((envs, n), math.nan, dtype=torch.float32, device=DEV)
    _bridge.launch(torch.device(DEV), _lib.lib().ocrl_sprite_env_uniforms, seed, 0, envs, 0, first, n, _lib.ptr(out))
    assert not out.isnan().any() and (out >= 0).all() and (out < 1).all()
    return out


def bits_equal(a, b):
    """two dicts of device tensors: the same keys, and every tensor the same bits"""
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) and same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)


def some_steps(B, most):
    """B step counts in [0, most]: 0, the largest, one beyond max_steps and a negative one among them"""
    return [[0, most, most + 40, -2, 1][r] if r < 5 else (r * 7) % (most + 1) for r in range(B)]


# ---------------------------------------------------------------------------------------------------------------- 1. step 0
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("task", list(TASKS))
def test_step_zero_is_the_first_frame_bit_for_bit(task, B):
    d = desc_of(task)
    for w, seed in enumerate(SEEDS):
        idx = indices(B, w)
        want = generate(d, seed, idx)
        got = rollout(d, seed, idx, steps=[0] * B)
        assert torch.equal(got.pop("taken"), torch.zeros(B, dtype=torch.int32, device=DEV))
        assert bits_equal(got, want)
        drawn = rollout(d, seed, idx, max_step=0)                          # a step drawn in [0, 0]
        assert torch.equal(drawn.pop("taken"), torch.zeros(B, dtype=torch.int32, device=DEV)) and bits_equal(drawn, want)
        neg = rollout(d, seed, idx, steps=[-1 - r for r in range(B)])     # clamped to 0
        assert torch.equal(neg.pop("taken"), torch.zeros(B, dtype=torch.int32, device=DEV)) and bits_equal(neg, want)


# ---------------------------------------------------------------------------------------------------------------- 2. the environment
@pytest.mark.parametrize("max_steps, T", [(100, 100), (12, 20)])
@pytest.mark.parametrize("task", ENV_TASKS)
def test_a_scene_is_the_frame_the_environment_shows_at_that_step(task, max_steps, T):
    """32 environments at episode 0 are stepped with the walk's own actions, t = 0 .. T.  While environment e is in episode 0, scene
    ((e << 24) | 0, t) is its frame and its rows; from the step L that ended the episode on, the scene stays the one at L - 1.
    max_steps 100: the test asserts that some episode ended by touching an object before the time limit (L < max_steps) and that some
    walk was cut by nothing but the time limit (L == max_steps: every step t <= max_steps - 1 was committed).  max_steps 12 with t up to
    20: every episode is cut by the time limit at the latest, steps_taken <= 11 everywhere."""
    from ocrl_amd import envs
    E, H, seed = 32, 16, WALK_SEED
    cfg = env_config(task, f"env.obs_size={H}", f"env.max_steps={max_steps}")
    env = envs.make_env(cfg, num_envs=E, seed=seed, device="cuda")
    d = envs.env_desc(cfg.env, 1)
    d.H = H
    assert d.max_steps == max_steps
    ua = walk_uniforms(seed, E, W.WALK_DRAW0, T)
    acts = ((ua.double() * 2 ** 24).long() * 4) >> 24                      # [E, T]
    assert set(acts.unique().tolist()) == {0, 1, 2, 3}
    frames, rows, episode = [], [], []
    env.reset()
    for t in range(T + 1):
        st = env.get_state()
        frames.append(env.render("rgb_array"))
        rows.append(env.state_obs(st["rows"]))
        episode.append(st["episode"])
        if t < T:
            env.step_device(acts[:, t].contiguous())
    frames, rows, episode = torch.stack(frames), torch.stack(rows), torch.stack(episode).cpu()      # [T + 1, E, ..]
    assert (episode[0] == 0).all()
    in0 = episode == 0
    assert (in0[:-1] | ~in0[1:]).all()                                     # an environment does not come back to episode 0
    L = in0.sum(0)                                                         # the step that ended episode 0; T + 1: none did
    assert (L <= max_steps).all()                                          # T >= max_steps: every episode 0 has ended
    # the scenes of every (e, t), four values of t to a call
    idx = [(e << 24) | 0 for e in range(E)]
    got = {k: [] for k in NAMES}
    for t0 in range(0, T + 1, 4):
        ts = list(range(t0, min(t0 + 4, T + 1)))
        part = rollout(d, seed, idx * len(ts), steps=[t for t in ts for _ in range(E)])
        for k in NAMES:
            got[k].append(part[k].view(len(ts), E, *part[k].shape[1:]))
    got = {k: torch.cat(v) for k, v in got.items()}                        # [T + 1, E, ..]
    taken = got["taken"].cpu()
    t_of = torch.arange(T + 1).view(-1, 1).expand(T + 1, E)
    last = (L - 1).view(1, E).expand(T + 1, E)
    assert torch.equal(taken.long(), torch.minimum(t_of, last))            # min(t, L - 1)
    assert torch.equal(got["u8"][in0], frames[in0]) and same_bits(got["objs"][in0].cpu().numpy(), rows[in0].cpu().numpy())
    at_end = last.to(DEV).clamp(max=T)                                     # from L on: the scene at L - 1, in every output
    ar = torch.arange(E, device=DEV)
    for k in ("obs", "u8", "masks", "objs", "labels"):
        frozen = got[k][at_end, ar.view(1, E).expand(T + 1, E)]
        assert torch.equal(got[k][~in0], frozen[~in0]) and same_bits(got[k][~in0].cpu().numpy(), frozen[~in0].cpu().numpy()), k
    assert (got["labels"] == got["labels"][0]).all()                      # the target does not change during the walk
    moved = (got["objs"][:, :, :, 3:] != got["objs"][0][None][:, :, :, 3:]).any(-1)                 # [T + 1, E, R]: rows whose position differs from step 0
    assert moved.any() and not moved[:, :, :d.lo].any()                   # only the agent moves (its row is at index n >= lo)
    # the restatement on the same uniforms ends every episode at the same step, in the same rows
    ua_h, objs_h = ua.cpu().numpy(), got["objs"].cpu().numpy()
    for e in range(E):
        try:
            ref_frames, Lref = W.walk(d, uniforms(seed, [idx[e]], 1024)[0], ua_h[e])
        except IndexError:
            ref_frames, Lref = W.walk(d, uniforms(seed, [idx[e]], 80000)[0], ua_h[e])
        assert Lref == int(L[e]) == len(ref_frames), (e, Lref, int(L[e]))
        for t in range(T + 1):
            want, n_taken = W.scene(ref_frames, Lref, t, max_steps)
            assert n_taken == int(taken[t, e]) and same_bits(objs_h[t, e], state_rows(want)), (e, t)
    if max_steps == 100:
        assert (L < max_steps).any() and (L == max_steps).any(), sorted(L.tolist())
    else:
        assert (taken <= max_steps - 1).all() and int(taken.max()) == max_steps - 1 and (L < max_steps).any()
    log(f"[task rollouts] {task} max_steps {max_steps}: episode 0 ended at steps {sorted(L.tolist())}")


# ---------------------------------------------------------------------------------------------------------------- 3. purity
@pytest.mark.parametrize("task", ["target-hard-13", "ooo-N4C2S2S1"])
def test_a_scene_is_its_seed_index_and_step_alone(task):
    d = desc_of(task, 8)
    steps = some_steps(130, d.max_steps)
    per_seed = []
    for w, seed in enumerate(SEEDS):
        idx = indices(130, w)
        full = rollout(d, seed, idx, steps=steps)
        assert bits_equal(full, rollout(d, seed, idx, steps=steps))                           # two calls
        for rows in ([4], [9], [9, 4, 100], [129, 1, 2], list(range(66, -1, -1)), list(range(63, 130))):       # batches of 1, 3 and 67, any position
            part = rollout(d, seed, [idx[r] for r in rows], steps=[steps[r] for r in rows])
            assert bits_equal(part, {k: v[rows] for k, v in full.items()}), rows
        assert idx[1] == idx[2] and steps[1] == d.max_steps < steps[2]                       # the repeated index: a step beyond max_steps is clamped to it
        assert all(torch.equal(v[1], v[2]) for v in full.values())
        per_seed.append(full)
        # any subset of the six outputs
        idx67, st67 = idx[:67], steps[:67]
        for bits in range(1, 63):
            keep = {k: bool(bits >> j & 1) for j, k in enumerate(NAMES)}
            part = rollout(d, seed, idx67, steps=st67, **keep)
            assert list(part) == [k for k in NAMES if keep[k]] and bits_equal(part, {k: full[k][:67] for k in part}), bits
    assert not torch.equal(per_seed[0]["objs"], per_seed[1]["objs"])                          # another seed, other scenes
    full = per_seed[1]
    first = generate(d, SEEDS[1], indices(130, 1))
    walked = (full["objs"] != first["objs"]).flatten(1).any(1)
    assert walked.any() and not walked[[0, 3]].any()                                          # steps 0 and -2 are the first frame; others have moved
    assert (full["taken"] <= torch.tensor(steps, device=DEV).clamp(0, d.max_steps)).all() and (full["taken"] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- 4. the drawn step
@pytest.mark.parametrize("T", [0, 5, 99, 255])
def test_the_drawn_step_is_draw_2_to_the_19_minus_1(T):
    d = desc_of("target-hard-44", 8)
    assert d.max_steps == 100
    for w, seed in enumerate(SEEDS):
        idx = indices(130, w)
        u = np.stack([uniforms_at(seed, i, W.WALK_DRAW0 - 1) for i in idx])
        t = np.floor(u.astype(np.float64) * (T + 1)).astype(np.int64)
        assert t.tolist() == [W.drawn_step(v, T) for v in u] and t.min() >= 0 and t.max() <= T
        drawn = rollout(d, seed, idx, max_step=T)
        explicit = rollout(d, seed, idx, steps=t.tolist())
        assert bits_equal(drawn, explicit)
        taken = drawn["taken"].cpu().numpy()
        assert (taken <= np.minimum(t, d.max_steps - 1)).all() and (taken >= 0).all()
        if T >= 99:
            assert len(set(t.tolist())) > 40 and t.max() > 0.8 * T and len(set(taken.tolist())) > 10      # 130 draws over T + 1 values
        if T == 0:
            assert not taken.any()


def uniforms_at(seed, i, j):
    """draw j of the episode of scene index i"""
    from ocrl_amd import _bridge, _lib
    i &= (1 << 44) - 1
    out = torch.full((1,), math.nan, dtype=torch.float32, device=DEV)
    _bridge.launch(torch.device(DEV), _lib.lib().ocrl_sprite_env_uniforms, seed, i >> 24, 1, i & 0xFFFFFF, j, 1, _lib.ptr(out))
    return out.cpu().numpy()[0]


# ---------------------------------------------------------------------------------------------------------------- 5. the pixels
@pytest.mark.parametrize("H, B", [(8, 130), (16, 67), (64, 3)])             # 64 rows: 4 bands, a workgroup to each
@pytest.mark.parametrize("task", list(TASKS))
def test_pixels_equal_the_sprite_renderer_of_the_walked_rows(task, H, B):
    from ocrl_amd.utils.tools import obs_from_uint8
    d = desc_of(task, H)
    for w, seed in enumerate(SEEDS):
        got = rollout(d, seed, indices(B, w), steps=some_steps(B, d.max_steps)[::-1])
        rows = raw_rows(got["objs"])
        assert torch.equal(got["u8"], sprite_render(rows, H, 1))
        want = obs_from_uint8(got["u8"])
        assert torch.equal(got["obs"], want) and same_bits(got["obs"].cpu().numpy(), want.cpu().numpy())
        m = sprite_render(rows, H, 2)[..., 0]
        assert m.shape == got["masks"].shape and torch.equal(got["masks"], m.float())
        assert set(got["masks"].unique().tolist()) <= {0.0, 1.0} and got["u8"].any()


# ---------------------------------------------------------------------------------------------------------------- 6. the loader
def loader(task="target-hard-44", **kw):
    from ocrl_amd.utils.device_scenes import DeviceTaskScenes
    args = dict(n=22, seed=5, batch_size=4, device=DEV, with_masks=True, with_objs=True, rollout_steps=30)
    args.update(kw)
    return DeviceTaskScenes(desc_of(task, 16), **args)


def test_the_loader_shards_and_shuffles_as_the_first_frame_loader_does():
    from ocrl_amd.utils.device_scenes import epoch_indices
    d = desc_of("target-hard-44", 16)
    dl = loader()
    batches = list(dl)
    assert len(dl) == len(batches) == 6 and [b["obss"].shape[0] for b in batches] == [4, 4, 4, 4, 4, 2]
    b = batches[0]
    assert list(b) == ["obss", "masks", "objs", "labels"]
    assert b["obss"].shape == (4, 3, 16, 16) and b["masks"].shape == (4, 6, 16, 16, 1) and b["objs"].shape == (4, 5, 5) and b["labels"].shape == (4, 1)
    want = rollout(d, 5, list(range(22)), max_step=30)
    cat = lambda k: torch.cat([x[k] for x in batches])
    assert torch.equal(cat("obss"), want["obs"]) and torch.equal(cat("objs"), want["objs"]) and torch.equal(cat("masks")[..., 0], want["masks"])
    assert torch.equal(cat("labels")[:, 0], want["labels"])
    s = dl.dataset[21]
    assert all(torch.equal(s[k], batches[5][k][1]) for k in s)
    # explicit steps through the loader, whatever rollout_steps is
    idx = torch.arange(4, dtype=torch.int64, device=DEV)
    st = torch.tensor([0, 3, 9, 50], dtype=torch.int32, device=DEV)
    for dl2 in (dl, loader(rollout_steps=None)):
        x = dl2.batch(idx, st)
        y = rollout(d, 5, idx, steps=st)
        assert torch.equal(x["obss"], y["obs"]) and torch.equal(x["objs"], y["objs"]) and torch.equal(x["masks"][..., 0], y["masks"])
    assert torch.equal(loader(rollout_steps=None).batch(idx)["objs"], generate(d, 5, idx)["objs"])     # None: the first frames, as before
    with pytest.raises(ValueError, match="int32"):
        dl.batch(idx, st.long())
    # a shuffled, sharded epoch: the scenes of epoch_indices, batch by batch; set_epoch changes the order
    for rank in range(2):
        a = loader(n=23, shuffle=True, drop_last=True, rank=rank, world=2)
        a.set_epoch(3)
        want_idx = epoch_indices(23, 5, 3, rank, 2, 4, True)
        got = list(a)
        assert len(got) == len(want_idx) == 2
        for x, i in zip(got, want_idx):
            assert torch.equal(x["objs"], rollout(d, 5, i.tolist(), max_step=30)["objs"])
        a.set_epoch(4)
        assert not torch.equal(torch.cat([x["objs"] for x in a]), torch.cat([x["objs"] for x in got]))

    def scene_set(dl):
        return {bytes(o.cpu().numpy().tobytes()) for b in dl for o in b["objs"]}
    everything = scene_set(loader(n=23))
    s0, s1 = (scene_set(loader(n=23, shuffle=True, rank=r, world=2)) for r in range(2))
    assert len(everything) == 23 and len(s0) == len(s1) == 11 and not (s0 & s1) and (s0 | s1) < everything


def test_the_agent_moves_across_a_batch_only_without_only_initial():
    from ocrl_amd.utils.config import compose
    from ocrl_amd.utils.datasets import get_dataloaders
    d = desc_of("target-hard-44", 16)
    args = ["ocr=vae", "dataset=target-N4C4S3S1", "dataset.obs_size=16", "dataset.synthetic_train=32", "dataset.synthetic_val=32", "dataset.with_objs=True"]
    first = get_dataloaders(compose(CFG, "train_ocr", args).dataset, 32, 0, seed=2, device=DEV)[1]
    later = get_dataloaders(compose(CFG, "train_ocr", args + ["dataset.only_initial=False"]).dataset, 32, 0, seed=2, device=DEV)[1]
    a, b = next(iter(first)), next(iter(later))
    agent = lambda x: {tuple(r) for r in x["objs"][:, 4, 3:].cpu().tolist()}
    assert agent(a) == {(0.5, 0.5)} and len(agent(b)) > 8
    assert torch.equal(a["objs"][:, :4], b["objs"][:, :4]) and torch.equal(a["labels"], b["labels"])      # the same episodes, seen later
    assert later.rollout_steps == 99 and torch.equal(b["objs"], rollout(d, 6, list(range(32)), max_step=99)["objs"])
    assert not torch.equal(a["obss"], b["obss"])


def test_train_ocr_runs_on_later_frames(tmp_path):
    from tests.test_gpu_ari import TINY_RUN
    cmd = [sys.executable, os.path.join(ROOT, "train_ocr.py"), *TINY_RUN["slate"], "dataset=target-N4C4S3S1", "dataset.only_initial=False",
           "dataset.obs_size=16", f"run_dir={tmp_path}", "max_steps=3", "batch_size=8", "eval_interval=2", "dataset.synthetic_train=64",
           "dataset.synthetic_val=8", "log_interval=1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    train = [l["train/loss"] for l in lines if "train/loss" in l]
    assert len(train) == 3 and all(np.isfinite(np.asarray(v)).all() for v in train)
