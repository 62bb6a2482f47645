"""GPU checks of the on-device pre-training scenes (ocrl_scenes_batch, ocrl_scenes_uniforms, ocrl_amd.utils.device_scenes) and of
train_ocr.py / get_ari_mse.py with dataset.on_device=True.

Bounds.  Everything is exact.  The objects are compared bit for bit with the numpy restatement of tests/scenes_ref.py, which follows the
kernel's fp32 operations one rounding at a time on the kernel's own uniforms.  The pixels are compared byte for byte and bit for bit
with code that predates the scenes: ocrl_sprite_render of the same rows (both evaluate the same fp32 predicates, so no pixel is
excluded) and ocrl_obs_u8_to_f32 of the bytes.  Every output buffer starts as NaN / 77, so a pixel the kernel leaves out fails too."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import scenes_ref as S
from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F = np.float32
CASES = [(5, 1), (5, 67), (1, 5), (9, 130), (15, 5)]           # (K, B)
SEEDS = [0, 0x9E3779B97F4A7C15]                                 # the second one has a high word: both halves of the key
HEAD = [0, 7, 7, 10 ** 6 + 5, 2 ** 39 + 1]                      # index 0, a repeated index, a large one, one beyond 2^32 << 7


def indices(B, which):
    """the B scene indices of seed number `which`"""
    if B == 1:
        return [[HEAD[0]], [HEAD[4]]][which]
    return (HEAD + list(range(100, 100 + B)))[:B]


def generate(H, K, seed, idx, obs=True, u8=True, masks=True, objs=True):
    """one ocrl_scenes_batch call -> dict of the requested outputs (device tensors), prefilled with NaN / 77"""
    from ocrl_amd import _bridge, _lib
    idx = torch.as_tensor(idx, dtype=torch.int64).to(DEV)
    B = idx.shape[0]
    out = {}
    if obs:
        out["obs"] = torch.full((B, 3, H, H), math.nan, dtype=torch.float32, device=DEV)
    if u8:
        out["u8"] = torch.full((B, H, H, 3), 77, dtype=torch.uint8, device=DEV)
    if masks:
        out["masks"] = torch.full((B, K + 1, H, H), math.nan, dtype=torch.float32, device=DEV)
    if objs:
        out["objs"] = torch.full((B, K, 5), math.nan, dtype=torch.float32, device=DEV)
    _bridge.launch(torch.device(DEV), _lib.lib().ocrl_scenes_batch, _lib.ScenesDesc(H=H, K=K), seed, _lib.ptr(idx), B, _lib.ptr(out.get("obs")),
                   _lib.ptr(out.get("u8")), _lib.ptr(out.get("masks")), _lib.ptr(out.get("objs")))
    return out


def uniforms(seed, idx, n):
    """the first n uniforms of every scene of idx -> numpy [len(idx), n]"""
    from ocrl_amd import _bridge, _lib
    out = torch.full((len(idx), n), math.nan, dtype=torch.float32, device=DEV)
    for r, i in enumerate(idx):
        _bridge.launch(torch.device(DEV), _lib.lib().ocrl_scenes_uniforms, seed, int(i), 0, n, _lib.ptr(out[r]))
    return out.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def drawn():
    """(K, B, seed number) -> (indices, objs of the kernel [B, K, 5] numpy, the restatement's per-scene results), made once"""
    out = {}
    for K, B in CASES:
        for w, seed in enumerate(SEEDS):
            idx = indices(B, w)
            got = generate(8, K, seed, idx, obs=False, u8=False, masks=False)["objs"].cpu().numpy()
            u = uniforms(seed, idx, K * (S.MAX_DRAWS // 15))
            assert not np.isnan(u).any() and (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
            out[K, B, w] = (idx, got, [S.scene(u[r], K) for r in range(B)])
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. the objects
@pytest.mark.parametrize("K,B", CASES)
def test_objs_equal_the_restatement_bit_for_bit(drawn, K, B):
    exhausted_total, draws = 0, []
    for w in range(len(SEEDS)):
        idx, got, ref = drawn[K, B, w]
        for r in range(B):
            objs, centres, used, exhausted = ref[r]
            assert same_bits(got[r], objs), (K, B, w, idx[r], got[r], objs)
            exhausted_total += len(exhausted)
            draws.append(used)
            if K == 5:
                assert exhausted == [], (idx[r], exhausted)          # of the order 1e-10 per object
            for k in range(K):
                if k in exhausted:
                    continue
                a, b, _ = S.interval(int(objs[k, 2]))
                x, y = objs[k, 3], objs[k, 4]
                assert a <= x <= b and a <= y <= b
                assert not S.dist(F(0.5), F(0.5), x, y) < F(0.15)
                assert all(not S.dist(objs[j, 3], objs[j, 4], x, y) < F(0.15) for j in range(k))
            assert set(objs[:, 0]) <= {0, 1, 2, 3} and set(objs[:, 1]) <= {0, 1, 2, 3} and set(objs[:, 2]) <= {0, 1}
        if B > 2:
            assert same_bits(got[1], got[2]) and not same_bits(got[0], got[1])      # the repeated index; two different scenes
    assert not same_bits(drawn[K, B, 0][1], drawn[K, B, 1][1])                     # another seed, other scenes
    log(f"[device scenes] K {K} B {B}: draws per scene {min(draws)} .. {max(draws)}, exhausted objects {exhausted_total}")


def test_an_index_is_taken_modulo_2_to_the_40():
    a = generate(8, 5, 3, [5, 2 ** 40 - 1, 2 ** 39 + 1])
    b = generate(8, 5, 3, [2 ** 40 + 5, -1, -(2 ** 39) + 1 - 2 ** 40])
    assert all(torch.equal(a[k], b[k]) for k in ("u8", "objs"))
    assert same_bits(uniforms(3, [2 ** 40 + 5], 16), uniforms(3, [5], 16))


# ---------------------------------------------------------------------------------------------------------------- 2. the pixels
def sprite_render(rows, H, mode):
    from ocrl_amd import _bridge, _lib
    B, R = rows.shape[:2]
    shape = {1: (B, H, H, 3), 2: (B, R + 1, H, H, 1)}[mode]
    out = torch.full(shape, 77, dtype=torch.uint8, device=DEV)
    _bridge.launch(torch.device(DEV), _lib.lib().ocrl_sprite_render, _lib.ptr(rows), B, R, H, mode, _lib.ptr(out))
    return out


@pytest.mark.parametrize("H", [16, 36])
@pytest.mark.parametrize("K,B", CASES)
def test_pixels_equal_the_sprite_renderer_and_the_byte_conversion(K, B, H):
    from ocrl_amd.utils.tools import obs_from_uint8
    for w, seed in enumerate(SEEDS):
        got = generate(H, K, seed, indices(B, w))
        rows = torch.from_numpy(S.rows(got["objs"].cpu().numpy())).to(DEV)
        assert torch.equal(got["u8"], sprite_render(rows, H, 1))
        assert torch.equal(got["obs"], obs_from_uint8(got["u8"])) and same_bits(got["obs"].cpu().numpy(), obs_from_uint8(got["u8"]).cpu().numpy())
        assert set(got["obs"].unique().tolist()) <= {0.0, 1.0}
        m = sprite_render(rows, H, 2)[..., 0].float()                                   # [B, K + 1, H, W]: each object alone; the background
        for k in range(K):
            want = m[:, k].clone()
            for j in range(k + 1, K):
                want *= 1 - m[:, j]
            assert torch.equal(got["masks"][:, k], want), (K, B, H, k)
        assert torch.equal(got["masks"][:, K], m[:, K])
        assert torch.equal(got["masks"].sum(1), torch.ones(B, H, H, device=DEV))
        assert set(got["masks"].unique().tolist()) <= {0.0, 1.0}
        assert got["masks"][:, :K].sum() > 0 and got["u8"].any()                        # something is drawn


# ---------------------------------------------------------------------------------------------------------------- 3. a scene is its index
def test_a_scene_depends_on_its_seed_and_index_alone():
    H, K, i = 16, 5, 10 ** 6 + 5
    alone = generate(H, K, 11, [i])
    idx = list(range(200, 267))
    idx[3], idx[66] = i, i
    batch = generate(H, K, 11, idx)
    for name, t in alone.items():
        assert torch.equal(batch[name][3], t[0]) and torch.equal(batch[name][66], t[0]), name
        assert not torch.equal(batch[name][4], t[0]), name
    # whichever other outputs are requested
    for keep in ("obs", "u8", "masks", "objs"):
        only = generate(H, K, 11, idx, **{k: k == keep for k in ("obs", "u8", "masks", "objs")})
        assert list(only) == [keep] and torch.equal(only[keep], batch[keep]), keep
    pair = generate(H, K, 11, idx, obs=False, objs=False)
    assert torch.equal(pair["u8"], batch["u8"]) and torch.equal(pair["masks"], batch["masks"])
    other = generate(H, K, 12, [i])
    assert not torch.equal(other["objs"], alone["objs"]) and not torch.equal(other["u8"], alone["u8"])


# ---------------------------------------------------------------------------------------------------------------- 4. the loader
def loader(**kw):
    from ocrl_amd.utils.device_scenes import DeviceScenes
    args = dict(n=22, size=16, seed=5, batch_size=4, device=DEV, with_masks=True, with_objs=True)
    args.update(kw)
    return DeviceScenes(**args)


def test_device_scenes_batches():
    from train_ocr import batch_inputs
    dl = loader()
    batches = list(dl)
    assert len(dl) == len(batches) == 6 and [b["obss"].shape[0] for b in batches] == [4, 4, 4, 4, 4, 2]
    b = batches[0]
    assert b["obss"].shape == (4, 3, 16, 16) and b["masks"].shape == (4, 6, 16, 16, 1) and b["objs"].shape == (4, 5, 5)
    assert all(t.dtype == torch.float32 and t.device == torch.device(DEV) for t in b.values())
    obs, masks = batch_inputs(b, DEV)
    assert obs is b["obss"] and masks.shape == (4, 6, 1, 16, 16) and torch.equal(masks[:, :, 0], b["masks"][..., 0])
    assert list(loader(with_masks=False, with_objs=False, drop_last=True).__iter__().__next__()) == ["obss"]
    assert len(loader(drop_last=True)) == 5 and len(list(loader(drop_last=True))) == 5
    # fresh tensors, the same scenes from an equal loader; the unshuffled order is the index order
    again = list(loader())
    for x, y in zip(batches, again):
        assert all(torch.equal(x[k], y[k]) and x[k].data_ptr() != y[k].data_ptr() for k in x)
    want = generate(16, 5, 5, list(range(22)))
    assert torch.equal(torch.cat([x["obss"] for x in batches]), want["obs"]) and torch.equal(torch.cat([x["objs"] for x in batches]), want["objs"])
    assert torch.equal(torch.cat([x["masks"] for x in batches])[..., 0], want["masks"])
    # .dataset[i] is row i of an unshuffled batch
    assert len(dl.dataset) == 22
    for i in (0, 5, 21):
        s = dl.dataset[i]
        assert s["obss"].shape == (3, 16, 16) and s["masks"].shape == (6, 16, 16, 1) and s["objs"].shape == (5, 5)
        assert all(torch.equal(s[k], batches[i // 4][k][i % 4]) for k in s)
    with pytest.raises(IndexError):
        dl.dataset[22]


def test_device_scenes_shuffle_shard_and_epochs():
    def scene_set(dl):
        return {bytes(o.cpu().numpy().tobytes()) for b in dl for o in b["objs"]}
    everything = scene_set(loader(n=23))
    assert len(everything) == 23
    r0, r1 = loader(n=23, shuffle=True, rank=0, world=2, drop_last=False), loader(n=23, shuffle=True, rank=1, world=2, drop_last=False)
    s0, s1 = scene_set(r0), scene_set(r1)
    assert len(s0) == len(s1) == 11 and not (s0 & s1) and (s0 | s1) < everything
    # two loaders with the same arguments: equal batches, also when shuffled; set_epoch reorders, and comes back
    a, b = loader(shuffle=True, drop_last=True), loader(shuffle=True, drop_last=True)
    a.set_epoch(3), b.set_epoch(3)
    e3 = [x["objs"] for x in a]
    assert all(torch.equal(x, y["objs"]) for x, y in zip(e3, b))
    a.set_epoch(4)
    e4 = [x["objs"] for x in a]
    assert not torch.equal(torch.stack(e3), torch.stack(e4))
    a.sampler.set_epoch(3)
    assert torch.equal(torch.stack([x["objs"] for x in a]), torch.stack(e3))
    assert not torch.equal(torch.stack([x["objs"] for x in a]), torch.stack(e3))        # a pass without set_epoch moves on, as a DataLoader's
    # the training loader of get_dataloaders: the scenes of seed 2 * seed + 1
    from ocrl_amd.utils.config import compose
    from ocrl_amd.utils.datasets import get_dataloaders
    c = compose(os.path.join(ROOT, "configs"), "train_ocr", ["ocr=vae", "dataset=random-N5C4S4S2", "dataset.on_device=True", "dataset.obs_size=16",
                                                             "dataset.synthetic_train=8", "dataset.synthetic_val=6", "dataset.with_objs=True"])
    tr, va = get_dataloaders(c.dataset, 4, 3, seed=2, device=DEV)
    assert {bytes(o.cpu().numpy().tobytes()) for b in tr for o in b["objs"]} == {bytes(o.cpu().numpy().tobytes()) for o in generate(16, 5, 5, list(range(8)))["objs"]}
    assert torch.equal(torch.cat([b["objs"] for b in va]), generate(16, 5, 6, list(range(6)))["objs"])


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def test_train_ocr_runs_on_device_scenes(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "train_ocr.py"), "ocr=vae", "dataset=random-N5C4S4S2", "dataset.on_device=True", f"run_dir={tmp_path}",
           "max_steps=3", "batch_size=8", "eval_interval=2", "dataset.synthetic_train=64", "dataset.synthetic_val=8", "log_interval=1"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (tmp_path / "checkpoints" / "model_latest.pth").exists()
    lines = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    train = [l["train/loss"] for l in lines if "train/loss" in l]
    val = [l["val/loss"] for l in lines if "val/loss" in l]
    assert len(train) == 3 and len(val) == 1 and all(np.isfinite(np.asarray(v)).all() for v in train + val)


def test_get_ari_mse_reads_device_scenes_and_their_masks_score_one(tmp_path):
    import get_ari_mse
    from ocrl_amd.utils.tools import calculate_ari
    from tests.test_gpu_ari import TINY_RUN
    out = get_ari_mse.main(TINY_RUN["slotattn"] + ["dataset=random-N5C4S4S2", "dataset.on_device=True", "dataset.obs_size=16", "dataset.with_masks=True",
                                                   "dataset.synthetic_val=10", "dataset.synthetic_train=4", "batch_size=4", "device=cuda:0",
                                                   f"run_dir={tmp_path / 'run'}"])
    assert out["num_images"] == 10 and math.isfinite(out["ari"]) and math.isfinite(out["mse"]) and -1 <= out["ari"] <= 1 and out["mse"] > 0
    from train_ocr import batch_inputs
    for b in loader(n=6, batch_size=6):
        _, masks = batch_inputs(b, DEV)                                                 # [B, K + 1, 1, H, W], the background last
        assert calculate_ari(masks, masks) == [1.0] * 6                                 # counted on the GPU: a partition against itself
