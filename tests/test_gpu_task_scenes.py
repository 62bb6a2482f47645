"""GPU checks of the task datasets (ocrl_task_scenes_batch, ocrl_amd.utils.device_scenes.DeviceTaskScenes): the first frames of the
sprite tasks' episodes, and train_ocr.py / get_ari_mse.py / the probe on them.

Bounds.  Everything is exact.  The rows are compared bit for bit with the numpy restatements of the environments (tests/sprite_env_ref.py,
tests/oddoneout_ref.py: they follow the episode's fp32 operations one rounding at a time) on the kernel's own uniforms, after the
state observation's scale-to-index mapping.  The pixels are compared byte for byte and bit for bit with entry points that predate the
dataset: ocrl_sprite_render of the same rows (both evaluate the same fp32 predicates, so no pixel is excluded) and ocrl_obs_u8_to_f32.
The tie to the environment is exact too: the frames and rows of a vectorised environment against the scenes of its (e, k).  Every
output buffer starts as NaN / 77 / -1, so an element the kernel leaves out fails."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ocrl_amd.utils.config import compose
from tests import oddoneout_ref as O
from tests import sprite_env_ref as R
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs")
DEV = "cuda:0"
F = np.float32
# name -> (env file, overrides).  The 15 objects are placed as tests/test_gpu_oddoneout.py places its 15: with occlusion and no wall distance
TASKS = {
    "target-hard-44": ("target-N4C4S3S1", []),
    "target-hard-13": ("target-N4C4S3S1", ["env.num_objects_range=[1,3]"]),
    "target-easy-24": ("target-N4C4S3S1", ["env.mode=easy", "env.num_objects_range=[2,4]"]),
    "target-hi15": ("target-N4C4S3S1", ["env.num_objects_range=[9,15]", "env.occlusion=True", "env.distance_to_wall=0.0", "env.SCALES=[0.15,0.22]"]),
    "ooo-N4C2S2S1": ("odd-one-out-N4C2S2S1", []),
    "ooo-N4C2S2S1-oc": ("odd-one-out-N4C2S2S1-oc", []),
}
BATCHES = [1, 3, 67, 130]
SEEDS = [0, 0x9E3779B97F4A7C15]                                 # the second one has a high word: both halves of the key
HEAD = [0, 7, 7, (5 << 24) | 3, 2 ** 43 + 1, -5]                # index 0, a repeated one, environment 5's episode 3, bit 43, a negative one
MASK44 = (1 << 44) - 1


def env_config(task, *over):
    name, own = TASKS[task]
    return compose(CFG, "train_sb3", ["ocr=slate", "pooling=transformer", "sb3=ppo", "sb3_acnet=mlp", f"env={name}", "device=cuda:0", *own, *over])


def desc_of(task, H=8):
    from ocrl_amd import envs
    d = envs.env_desc(env_config(task).env, 1)
    d.H = H
    return d


def indices(B, which):
    """the B scene indices of seed number `which`: between them the two lists of every B hold every index of HEAD"""
    if B == 1:
        return [[HEAD[0]], [HEAD[4]]][which]
    head = HEAD[:3] if (B == 3 and which == 0) else (HEAD[3:] if B == 3 else HEAD)
    return (head + list(range(100, 100 + B)))[:B]


def e_k(i):
    i &= MASK44
    return i >> 24, i & 0xFFFFFF


def generate(d, seed, idx, obs=True, u8=True, masks=True, objs=True, labels=True):
    """one ocrl_task_scenes_batch call -> dict of the requested outputs (device tensors), prefilled with NaN / 77 / -1"""
    from ocrl_amd import _bridge, _lib
    idx = torch.as_tensor(idx, dtype=torch.int64).to(DEV)
    B, H, R_ = idx.shape[0], d.H, d.hi + 1
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
    _bridge.launch(torch.device(DEV), _lib.lib().ocrl_task_scenes_batch, d, seed, _lib.ptr(idx), B, _lib.ptr(out.get("obs")), _lib.ptr(out.get("u8")),
                   _lib.ptr(out.get("masks")), _lib.ptr(out.get("objs")), _lib.ptr(out.get("labels")))
    return out


def uniforms(seed, idx, n):
    """the first n uniforms of the episode of every index of idx -> numpy [len(idx), n]"""
    from ocrl_amd import _bridge, _lib
    out = torch.full((len(idx), n), math.nan, dtype=torch.float32, device=DEV)
    for r, i in enumerate(idx):
        e, k = e_k(int(i))
        _bridge.launch(torch.device(DEV), _lib.lib().ocrl_sprite_env_uniforms, seed, e, 1, k, 0, n, _lib.ptr(out[r]))
    u = out.cpu().numpy()
    assert not np.isnan(u).any() and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    return u


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def state_rows(rows):
    """the state observation of the restatement's rows: the scale as its index in [0.15, 0.22], an all-zero row stays zero"""
    out = rows.copy()
    z = rows[:, 2]
    out[:, 2] = np.where((z == F(0.15)) | ~rows.any(axis=1), F(0), np.where(z == F(0.22), F(1), F(-1)))
    return out


def raw_rows(objs, scales=(0.15, 0.22)):
    """the rows ocrl_sprite_render paints from a kernel's objs [B, R, 5]: the scale index back to the scale; a zero row stays undrawn"""
    rows = objs.clone()
    z = torch.tensor(scales, dtype=torch.float32, device=objs.device)[objs[..., 2].long().clamp(0, 1)]
    rows[..., 2] = torch.where(objs.abs().sum(-1) == 0, torch.zeros_like(z), z)
    return rows.contiguous()


def reference(d, u):
    """the restatement's episode from the uniforms u -> (rows, n, target, draws used)"""
    if d.task == 1:
        rows, n, target, _, used = O.reset(O.spec_from_desc(d), u)
    else:
        rows, n, target, used = R.reset(R.spec_from_desc(d), u)
    return rows, n, target, used


# ---------------------------------------------------------------------------------------------------------------- 1. the rows
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("task", list(TASKS))
def test_rows_labels_and_n_equal_the_restatements_bit_for_bit(task, B):
    d = desc_of(task)
    draws, counts = [], set()
    per_seed = []
    for w, seed in enumerate(SEEDS):
        idx = indices(B, w)
        got = generate(d, seed, idx, obs=False, u8=False, masks=False)
        objs, labels = got["objs"].cpu().numpy(), got["labels"].cpu().numpy()
        u = uniforms(seed, idx, 1024)
        for r in range(B):
            try:
                rows, n, target, used = reference(d, u[r])
            except IndexError:                                         # a crowded placement that restarted: the whole stream an episode may use
                rows, n, target, used = reference(d, uniforms(seed, [idx[r]], 80000)[0])
            assert same_bits(objs[r], state_rows(rows)), (task, B, w, idx[r], objs[r], rows)
            assert labels[r] == target and 0 <= target < n
            # n: the agent's row follows the n objects, zero rows follow it
            assert d.lo <= n <= d.hi and tuple(objs[r, n, :2]) == (d.agent_color, d.agent_shape) and not objs[r, n + 1:].any() and objs[r, :n, 2].min() >= 0
            draws.append(used)
            counts.add(n)
        if B > 3:
            assert same_bits(objs[1], objs[2]) and labels[1] == labels[2] and not same_bits(objs[0], objs[1])     # the repeated index
        per_seed.append(objs)
    assert not same_bits(per_seed[0], per_seed[1])                                                               # another seed, other scenes
    if B >= 67 and d.hi > d.lo:
        assert len(counts) == d.hi - d.lo + 1 if d.hi - d.lo < 4 else len(counts) >= 4
    log(f"[task scenes] {task} B {B}: draws per episode {min(draws)} .. {max(draws)}, object counts {sorted(counts)}")


# ---------------------------------------------------------------------------------------------------------------- 2. the pixels
def sprite_render(rows, H, mode):
    from ocrl_amd import _bridge, _lib
    B, R_ = rows.shape[:2]
    shape = {1: (B, H, H, 3), 2: (B, R_ + 1, H, H, 1)}[mode]
    out = torch.full(shape, 77, dtype=torch.uint8, device=DEV)
    _bridge.launch(torch.device(DEV), _lib.lib().ocrl_sprite_render, _lib.ptr(rows), B, R_, H, mode, _lib.ptr(out))
    return out


PIXEL_B = {8: 130, 12: 67, 64: 3, 132: 3}                      # 132 rows: 19 bands of 7, the last one of 6; here a workgroup to every band


@pytest.mark.parametrize("H", [8, 12, 64, 132])
@pytest.mark.parametrize("task", list(TASKS))
def test_pixels_equal_the_sprite_renderer_and_the_byte_conversion(task, H):
    from ocrl_amd.utils.tools import obs_from_uint8
    d, B = desc_of(task, H), PIXEL_B[H]
    for w, seed in enumerate(SEEDS):
        got = generate(d, seed, indices(B, w))
        rows = raw_rows(got["objs"])
        assert torch.equal(got["u8"], sprite_render(rows, H, 1))
        want = obs_from_uint8(got["u8"])
        assert torch.equal(got["obs"], want) and same_bits(got["obs"].cpu().numpy(), want.cpu().numpy())
        m = sprite_render(rows, H, 2)[..., 0]
        assert m.shape == got["masks"].shape and torch.equal(got["masks"], m.float())
        assert set(got["masks"].unique().tolist()) <= {0.0, 1.0}
        n = (got["objs"].abs().sum(-1) != 0).sum(1)                                     # drawn rows: the objects and the agent
        for r in range(B):
            assert not got["masks"][r, int(n[r]):-1].any()                              # the planes of empty rows
            if H >= 64:
                assert got["masks"][r, :int(n[r])].flatten(1).any(1).all()              # every sprite is seen alone
        assert got["u8"].any() and (got["masks"][:, -1] == (got["masks"][:, :-1].sum(1) == 0)).all()
        if not d.occlusion:
            assert torch.equal(got["masks"].sum(1), torch.ones(B, H, H, device=DEV))    # sprites kept apart: a partition


@pytest.mark.parametrize("H,B,per_scene", [(64, 300, 3), (64, 1030, 1), (132, 130, 7)])
def test_pixels_when_a_workgroup_takes_several_bands(H, B, per_scene):
    """a launch holds at most 1024 workgroups where the batch allows: 1024 // B to a scene, each taking every per_scene-th band.  3 of 4
    bands (one workgroup takes two), one workgroup for all 4, 7 for 19 (5 take three, 2 take two)"""
    from ocrl_amd.utils.tools import obs_from_uint8
    assert per_scene == max(1, 1024 // B) < -(-H // max(1, 1024 // H))
    d = desc_of("target-hard-13", H)
    got = generate(d, SEEDS[1], indices(B, 1))
    rows = raw_rows(got["objs"])
    assert torch.equal(got["u8"], sprite_render(rows, H, 1)) and torch.equal(got["obs"], obs_from_uint8(got["u8"]))
    assert torch.equal(got["masks"], sprite_render(rows, H, 2)[..., 0].float())
    small = generate(d, SEEDS[1], indices(B, 1)[:3])                                    # the same scenes at a workgroup to every band
    assert all(torch.equal(small[k], got[k][:3]) for k in got)


# ---------------------------------------------------------------------------------------------------------------- 3. subsets
@pytest.mark.parametrize("task", ["target-hard-13", "ooo-N4C2S2S1"])
def test_any_subset_of_outputs_gives_the_same_outputs(task):
    d = desc_of(task, 12)
    idx = indices(67, 0)
    names = ("obs", "u8", "masks", "objs", "labels")
    full = generate(d, 11, idx)
    for bits in range(1, 31):
        keep = {k: bool(bits >> j & 1) for j, k in enumerate(names)}
        part = generate(d, 11, idx, **keep)
        assert list(part) == [k for k in names if keep[k]]
        for k, t in part.items():
            assert torch.equal(t, full[k]) and same_bits(t.cpu().numpy(), full[k].cpu().numpy()), (bits, k)
    # a scene is its seed and index alone: whichever batch it is in, at whichever position
    alone = generate(d, 11, [idx[4]])
    assert all(torch.equal(alone[k][0], full[k][4]) and not torch.equal(alone[k][0], full[k][5]) for k in ("u8", "objs", "masks"))
    other = generate(d, 12, [idx[4]])
    assert not torch.equal(other["objs"], alone["objs"]) and not torch.equal(other["u8"], alone["u8"])


# ---------------------------------------------------------------------------------------------------------------- 4. the index
def test_an_index_is_taken_modulo_2_to_the_44():
    d = desc_of("target-hard-13", 12)
    a = generate(d, 3, [5, 2 ** 44 - 1, 2 ** 43 + 1, (5 << 24) | 3])
    b = generate(d, 3, [2 ** 44 + 5, -1, 2 ** 43 + 1 - 2 ** 45, ((5 << 24) | 3) + (9 << 44)])
    assert all(torch.equal(a[k], b[k]) and same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)
    c = generate(d, 3, [5 + (1 << 24), 2 ** 43 - 1, 2 ** 43, 3])                            # bits below 44 all count
    assert all(not torch.equal(a["objs"][r], c["objs"][r]) for r in range(4))


# ---------------------------------------------------------------------------------------------------------------- 5. the environment
@pytest.mark.parametrize("task", ["target-hard-44", "target-hard-13", "ooo-N4C2S2S1-oc"])
def test_a_scene_is_what_the_environment_shows_when_that_episode_begins(task):
    from ocrl_amd import envs
    E, H = 5, 16
    for seed in SEEDS:
        cfg = env_config(task, f"env.obs_size={H}")
        env = envs.make_env(cfg, num_envs=E, seed=seed, device="cuda")
        d = desc_of(task, H)
        for k in range(2):                                                                   # the first reset, then a second one
            frames = env.reset()
            st = env.get_state()
            got = generate(d, seed, [(e << 24) | k for e in range(E)])
            assert torch.equal(st["episode"].cpu(), torch.full((E,), k, dtype=torch.int32))
            assert torch.equal(got["u8"].permute(0, 3, 1, 2), frames) and torch.equal(got["u8"], env.render("rgb_array"))
            assert same_bits(got["objs"].cpu().numpy(), env.state_obs(st["rows"]).cpu().numpy())
            assert torch.equal(got["labels"], st["target"].long())
            assert torch.equal(got["masks"], env.render("mask")[..., 0].float())
            assert same_bits(raw_rows(got["objs"]).cpu().numpy(), st["rows"].cpu().numpy())   # one scale list: the very rows
        assert not torch.equal(got["u8"][0], got["u8"][1])


# ---------------------------------------------------------------------------------------------------------------- 6. the loader
def loader(task="target-hard-44", **kw):
    from ocrl_amd.utils.device_scenes import DeviceTaskScenes
    args = dict(n=22, seed=5, batch_size=4, device=DEV, with_masks=True, with_objs=True)
    args.update(kw)
    return DeviceTaskScenes(desc_of(task, 16), **args)


def test_the_loaders_epochs_are_epoch_indices_and_ranks_are_disjoint():
    from train_ocr import batch_inputs
    from ocrl_amd.utils.device_scenes import epoch_indices
    d = desc_of("target-hard-44", 16)
    dl = loader()
    batches = list(dl)
    assert len(dl) == len(batches) == 6 and [b["obss"].shape[0] for b in batches] == [4, 4, 4, 4, 4, 2]
    b = batches[0]
    assert list(b) == ["obss", "masks", "objs", "labels"]
    assert b["obss"].shape == (4, 3, 16, 16) and b["masks"].shape == (4, 6, 16, 16, 1) and b["objs"].shape == (4, 5, 5) and b["labels"].shape == (4, 1)
    assert b["labels"].dtype == torch.int64 and all(t.device == torch.device(DEV) for t in b.values())
    obs, masks = batch_inputs(b, DEV)
    assert obs is b["obss"] and masks.shape == (4, 6, 1, 16, 16) and torch.equal(masks[:, :, 0], b["masks"][..., 0])
    assert list(next(iter(loader(with_masks=False, with_objs=False)))) == ["obss"]
    want = generate(d, 5, list(range(22)))
    cat = lambda k: torch.cat([x[k] for x in batches])
    assert torch.equal(cat("obss"), want["obs"]) and torch.equal(cat("objs"), want["objs"]) and torch.equal(cat("masks")[..., 0], want["masks"])
    assert torch.equal(cat("labels")[:, 0], want["labels"])
    s = dl.dataset[21]
    assert s["obss"].shape == (3, 16, 16) and s["labels"].shape == (1,) and all(torch.equal(s[k], batches[5][k][1]) for k in s)
    # a shuffled, sharded epoch: the scenes of epoch_indices, batch by batch
    for rank in range(2):
        a = loader(n=23, shuffle=True, drop_last=True, rank=rank, world=2)
        a.set_epoch(3)
        idx = epoch_indices(23, 5, 3, rank, 2, 4, True)
        got = list(a)
        assert len(got) == len(idx) == 2
        for x, i in zip(got, idx):
            assert torch.equal(x["objs"], generate(d, 5, i.tolist(), obs=False, u8=False, masks=False, labels=False)["objs"])

    def scene_set(dl):
        return {bytes(o.cpu().numpy().tobytes()) for b in dl for o in b["objs"]}
    everything = scene_set(loader(n=23))
    s0, s1 = (scene_set(loader(n=23, shuffle=True, rank=r, world=2)) for r in range(2))
    assert len(everything) == 23 and len(s0) == len(s1) == 11 and not (s0 & s1) and (s0 | s1) < everything
    with pytest.raises(ValueError, match="num_objects_range"):
        loader("target-hard-13")
    # get_dataloaders: the scenes of seeds 2 * seed + 1 and 2 * seed + 2
    from ocrl_amd.utils.datasets import get_dataloaders
    c = compose(CFG, "train_ocr", ["ocr=vae", "dataset=target-N4C4S3S1", "dataset.obs_size=16", "dataset.synthetic_train=8", "dataset.synthetic_val=6",
                                   "dataset.with_objs=True"])
    tr, va = get_dataloaders(c.dataset, 4, 3, seed=2, device=DEV)
    assert scene_set(tr) == {bytes(o.cpu().numpy().tobytes()) for o in generate(d, 5, list(range(8)))["objs"]}
    assert torch.equal(torch.cat([b["objs"] for b in va]), generate(d, 6, list(range(6)))["objs"])


def test_train_ocr_runs_on_a_task_dataset(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train_ocr.py"), "ocr=vae", "dataset=target-N4C4S3S1", "dataset.obs_size=16", f"run_dir={tmp_path}",
           "max_steps=3", "batch_size=8", "eval_interval=2", "dataset.synthetic_train=64", "dataset.synthetic_val=8", "log_interval=1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (tmp_path / "checkpoints" / "model_latest.pth").exists()
    lines = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    train = [l["train/loss"] for l in lines if "train/loss" in l]
    val = [l["val/loss"] for l in lines if "val/loss" in l]
    assert len(train) == 3 and len(val) == 1 and all(np.isfinite(np.asarray(v)).all() for v in train + val)


def test_get_ari_mse_reads_a_task_datasets_masks(tmp_path):
    import get_ari_mse
    from ocrl_amd.utils.tools import calculate_ari
    from tests.test_gpu_ari import TINY_RUN
    out = get_ari_mse.main(TINY_RUN["slotattn"] + ["dataset=odd-one-out-N4C2S2S1", "dataset.obs_size=16", "dataset.with_masks=True", "dataset.synthetic_val=10",
                                                   "dataset.synthetic_train=4", "batch_size=4", "device=cuda:0", f"run_dir={tmp_path / 'run'}"])
    assert out["num_images"] == 10 and math.isfinite(out["ari"]) and math.isfinite(out["mse"]) and -1 <= out["ari"] <= 1 and out["mse"] > 0
    from train_ocr import batch_inputs
    for b in loader("ooo-N4C2S2S1", n=6, batch_size=6):
        _, masks = batch_inputs(b, DEV)                                                 # [B, 6, 1, H, W]: sprites kept apart, a partition
        assert calculate_ari(masks, masks) == [1.0] * 6


def test_the_probe_reads_a_task_datasets_rows():
    from oracle import slate_oracle as SO
    from ocrl_amd.utils.property_predictor import PropertyPredictor
    from tests.golden import make_golden_probe as G
    from tests.gpu_util import build_wrapper
    cfg = SO.default_cfg(obs_size=16, vocab_size=256, num_slots=6, num_iterations=3, num_dec_blocks=2)
    pp = PropertyPredictor(build_wrapper(cfg, SO.formula_params(cfg)), G.probe_config("slate_mlp3"), G.dataset_config())
    pp.to("cuda:0")
    pp.eval()
    batch = next(iter(loader(batch_size=4)))
    m = pp.get_loss({"obss": batch["obss"], "objs": batch["objs"]})
    torch.cuda.synchronize()
    assert all(v.is_cuda and v.dim() == 0 and torch.isfinite(v) for v in m.values()) and m["loss"].item() > 0
    assert pp.last_matching.shape == (4, 5) and all(len(set(r)) == 5 for r in pp.last_matching.cpu().tolist())
