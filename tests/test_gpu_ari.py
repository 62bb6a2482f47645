"""Segmentation ARI on the GPU (csrc/ari.hip, ocrl_ari_counts) against torch.argmax + numpy tables on the CPU.  Everything here is an
integer or a float computed from equal integers by shared code, so every comparison is exact: torch.equal / ==, no tolerance.

Shapes of the exact-table test: B in {1, 3, 128} x N in {1, 225, 4096, 16384, 65536} x (Ct, Cp) in {(1,1), (2,7), (6,7), (7,7), (17,17),
(32,32)}, each in the channel-major [B, C, N] layout, the pixel-major [B, N, C] layout (read through a transposed view) and a channel-major
layout with padded rows (16-byte loads with a ragged tail).  The tie / NaN and fused-mode tests choose their own shapes: odd and
power-of-two pixel counts on both sides of one workgroup's share, and channel counts at 1, typical (6, 7) and the limit (32)."""
import json
import os

import numpy as np
import pytest
import torch

from tests.gpu_util import log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(1, 1), (2, 7), (6, 7), (7, 7), (17, 17), (32, 32)]


def _ref_counts(t_cpu, p_cpu):
    """table [B, Ct, Cp] int32 and sums [B, 3] int64 from torch.argmax labels of two CPU stacks [B, C, N], built in numpy"""
    B, Ct, N = t_cpu.shape
    Cp = p_cpu.shape[1]
    t = torch.argmax(t_cpu, dim=1).numpy()
    p = torch.argmax(p_cpu, dim=1).numpy()
    code = (np.arange(B, dtype=np.int64)[:, None] * Ct + t) * Cp + p
    table = np.bincount(code.ravel(), minlength=B * Ct * Cp).reshape(B, Ct, Cp).astype(np.int64)
    comb = lambda x: x * (x - 1) // 2
    sums = np.stack([comb(table).sum((1, 2)), comb(table.sum(2)).sum(1), comb(table.sum(1)).sum(1)], axis=1)
    return torch.from_numpy(table.astype(np.int32)), torch.from_numpy(sums)


def _layouts(x):
    """the same [B, C, N] values in three memory layouts: channel-major, pixel-major (a transposed view of [B, N, C]), channel-major with
    rows padded to a multiple of four floats plus four"""
    B, C, N = x.shape
    pm = x.transpose(1, 2).contiguous().transpose(1, 2)
    pad = torch.full((B, C, (N + 3) // 4 * 4 + 4), 9.0, device=x.device)
    pad[:, :, :N] = x
    out = {"channel_major": x, "pixel_major": pm, "padded_rows": pad[:, :, :N]}
    assert out["pixel_major"].stride() == (N * C, 1, C) or N == 1 or C == 1
    return out


def _check(truth, pred, ref, fuse_fg=False, tag=""):
    from ocrl_amd.utils.tools import ari_counts
    table, sums = ari_counts(truth, pred, fuse_fg)
    assert table.dtype == torch.int32 and sums.dtype == torch.int64
    ok_t, ok_s = torch.equal(table.cpu(), ref[0]), torch.equal(sums.cpu(), ref[1])
    assert ok_t and ok_s, (tag, ok_t, ok_s, (table.cpu() - ref[0]).abs().sum().item())


@pytest.mark.parametrize("N", [1, 225, 4096, 16384, 65536])
@pytest.mark.parametrize("B", [1, 3, 128])
@pytest.mark.parametrize("Ct,Cp", PAIRS)
def test_tables_and_sums_are_exact(B, N, Ct, Cp):
    g = torch.Generator(device="cuda").manual_seed(B * 1000003 + N * 101 + Ct * 7 + Cp)
    truth = torch.rand(B, Ct, N, device="cuda", generator=g)
    pred = torch.rand(B, Cp, N, device="cuda", generator=g)
    ref = _ref_counts(truth.cpu(), pred.cpu())
    assert int(ref[0].sum()) == B * N
    lt, lp = _layouts(truth), _layouts(pred)
    for name in lt:
        _check(lt[name], lp[name], ref, tag=name)
    _check(lt["channel_major"], lp["pixel_major"], ref, tag="mixed")


@pytest.mark.parametrize("N", [225, 4096, 5000])
@pytest.mark.parametrize("Ct,Cp", [(2, 7), (6, 7), (32, 32)])
@pytest.mark.parametrize("kind", ["ties", "ties_and_nan"])
def test_ties_and_nan_follow_torch_argmax(kind, Ct, Cp, N):
    """scores from a grid of four values: most pixels have tied maxima and the first index must win; a tenth of the pixels are zero in
    every channel; with NaNs scattered in, a NaN is the maximum and the first NaN wins"""
    B = 3
    g = torch.Generator().manual_seed(N + Ct)
    truth = torch.randint(0, 4, (B, Ct, N), generator=g).float() * 0.25
    pred = torch.randint(0, 4, (B, Cp, N), generator=g).float() * 0.25
    zero_t, zero_p = torch.rand(B, 1, N, generator=g) < 0.1, torch.rand(B, 1, N, generator=g) < 0.1
    truth, pred = truth.masked_fill(zero_t, 0.0), pred.masked_fill(zero_p, 0.0)
    pred[:, :, ::7] = -pred[:, :, ::7]                   # -0.0 == 0.0: still a tie
    if kind == "ties_and_nan":
        truth = truth.masked_fill(torch.rand(B, Ct, N, generator=g) < 0.05, float("nan"))
        pred = pred.masked_fill(torch.rand(B, Cp, N, generator=g) < 0.05, float("nan"))
    ref = _ref_counts(truth, pred)
    lt, lp = _layouts(truth.cuda()), _layouts(pred.cuda())
    for name in lt:
        _check(lt[name], lp[name], ref, tag=name)


def _masks(kind, B, Ct, S, g):
    if kind == "one_hot":
        lab = torch.randint(0, Ct, (B, S, S), generator=g)
        return torch.nn.functional.one_hot(lab, Ct).permute(0, 3, 1, 2).unsqueeze(2).float()
    m = torch.softmax(3.0 * torch.randn(B, Ct, 1, S, S, generator=g), dim=1)
    if kind == "soft_with_exact":                        # soft masks whose background channel is exactly 0.0 or 1.0 on a third of the pixels each
        u = torch.rand(B, 1, S, S, generator=g)
        m[:, -1] = torch.where(u < 1 / 3, torch.zeros(()), torch.where(u < 2 / 3, torch.ones(()), m[:, -1]))
    return m


@pytest.mark.parametrize("S", [15, 64])
@pytest.mark.parametrize("K", [1, 6, 7, 31])
@pytest.mark.parametrize("kind", ["one_hot", "soft", "soft_with_exact"])
def test_fused_foreground_equals_the_three_torch_lines(kind, K, S):
    """attention maps with entries forced to exactly 1.0f and 0.0f: on a foreground pixel (fg == 1.0) an attention of 1.0 wins over the
    foreground channel by the first-index rule only, on a background pixel every score is 0.0 and the label is 0"""
    B, Ct = 3, 6
    g = torch.Generator().manual_seed(S * 100 + K)
    masks = _masks(kind, B, Ct, S, g)
    attns = torch.softmax(torch.randn(B, K, 1, S, S, generator=g), dim=1)
    u = torch.rand(B, K, 1, S, S, generator=g)
    attns = torch.where(u < 0.1, torch.ones(()), torch.where(u < 0.3, torch.zeros(()), attns))
    fg_mask = 1 - masks[:, -1].unsqueeze(1)
    cat = torch.cat([attns * fg_mask, fg_mask], dim=1)
    ref = _ref_counts(masks.flatten(2), cat.flatten(2))
    if kind == "one_hot" and K > 1:
        assert int(ref[0][:, :-1, :K].sum()) > 0 and int(ref[0][:, :-1, K].sum()) > 0 and int(ref[0][:, -1, 1:].sum()) == 0
    lm, la = _layouts(masks.flatten(2).cuda()), _layouts(attns.flatten(2).cuda())
    for nm in ("channel_major", "pixel_major"):
        for na in la:
            _check(lm[nm], la[na], ref, fuse_fg=True, tag=f"{nm}/{na}")
    # the plain mode on the concatenated stack sees the same table
    _check(masks.cuda(), cat.cuda(), ref, tag="plain")
    from ocrl_amd.utils.tools import calculate_ari, segmentation_ari
    want = calculate_ari(masks, cat)                     # CPU tensors: the numpy path
    pm = la["pixel_major"].reshape(B, K, 1, S, S)
    assert segmentation_ari(masks.cuda(), attns.cuda()) == want
    assert segmentation_ari(masks.cuda(), pm) == want
    assert calculate_ari(masks.cuda(), cat.cuda()) == want


@pytest.mark.parametrize("B,Ct,Cp,S", [(1, 6, 7, 64), (5, 3, 4, 15), (128, 6, 7, 64), (2, 32, 32, 128), (2, 7, 7, 256)])
def test_calculate_ari_device_equals_cpu(B, Ct, Cp, S):
    from ocrl_amd.utils.tools import calculate_ari
    g = torch.Generator().manual_seed(B + S)
    true = torch.rand(B, Ct, 1, S, S, generator=g)
    pred = torch.softmax(4.0 * torch.randn(B, Cp, 1, S, S, generator=g), dim=1)
    cpu = calculate_ari(true, pred)
    dev = calculate_ari(true.cuda(), pred.cuda())
    assert isinstance(dev, list) and len(dev) == B and all(isinstance(x, float) for x in dev)
    assert dev == cpu
    # a labeling against itself, and other dtypes / wide stacks (these take the torch path on the device tensors)
    assert calculate_ari(true.cuda(), true.cuda()) == [1.0] * B
    assert calculate_ari(true.cuda().double(), pred.cuda().double()) == calculate_ari(true.double(), pred.double())


def test_misaligned_and_expanded_stacks():
    """a stack that starts 4 bytes off a 16-byte boundary takes the scalar loads; a stride-0 (expanded) batch is read as it stands"""
    B, C, N = 2, 6, 1024
    g = torch.Generator(device="cuda").manual_seed(11)
    buf = torch.rand(B * C * N + 1, device="cuda", generator=g)
    x = buf[1:].view(B, C, N)
    assert x.data_ptr() % 16 == 4
    y = torch.rand(1, C + 1, N, device="cuda", generator=g).expand(B, C + 1, N)
    _check(x, y, _ref_counts(x.cpu(), y.cpu()), tag="misaligned/expanded")


def test_stream_order_and_rezeroing():
    """on a side stream, with the inputs produced on that stream immediately before the call and no device-wide synchronise: the counts
    are those of the inputs; a table handed over dirty comes back as if it had been clean"""
    import ctypes
    from ocrl_amd import _lib
    from ocrl_amd.utils.tools import ari_counts
    B, Ct, Cp, N = 16, 6, 7, 128 * 128
    s = torch.cuda.Stream()
    results, inputs = [], []
    with torch.cuda.stream(s):
        g = torch.Generator(device="cuda").manual_seed(5)
        for i in range(4):
            big = torch.randn(B, Ct + Cp, N, device="cuda", generator=g)
            for _ in range(8):
                big = torch.sin(big * 1.5 + 0.25)        # queued work the counting kernel has to wait for
            inputs.append(big)
            results.append(ari_counts(big[:, :Ct], big[:, Ct:]))
        table = torch.full((B, Ct, Cp), 7, dtype=torch.int32, device="cuda")
        sums = torch.full((B, 3), -1, dtype=torch.int64, device="cuda")
        t, p = inputs[0][:, :Ct], inputs[0][:, Ct:]
        for _ in range(3):                               # the same buffers three times: no count survives a call
            _lib.check(_lib.lib().ocrl_ari_counts(_lib.ptr(t), *t.stride(), Ct, _lib.ptr(p), *p.stride(), Cp, 0, B, N, _lib.ptr(table),
                                                  _lib.ptr(sums), ctypes.c_void_p(s.cuda_stream)))
    s.synchronize()
    for big, (tb, sm) in zip(inputs, results):
        ref = _ref_counts(big[:, :Ct].cpu(), big[:, Ct:].cpu())
        assert torch.equal(tb.cpu(), ref[0]) and torch.equal(sm.cpu(), ref[1])
    ref = _ref_counts(t.cpu(), p.cpu())
    assert torch.equal(table.cpu(), ref[0]) and torch.equal(sums.cpu(), ref[1])


def _cpu_path(masks, attns):
    """what get_loss did before the kernel existed: the three torch lines on the device, calculate_ari on CPU tensors"""
    from ocrl_amd.utils.tools import calculate_ari
    fg_mask = 1 - masks[:, -1].unsqueeze(1)
    cat = torch.cat([attns * fg_mask, fg_mask], dim=1)
    return calculate_ari(masks.cpu(), cat.cpu())


def test_slot_attention_get_loss_reports_the_device_ari(golden_dir):
    from oracle import slate_oracle as O
    from tests.gpu_util import build_wrapper
    from tests.test_gpu_surface import BCM, _seeded_masks
    fx = np.load(os.path.join(golden_dir, "slate_masks_bcdec.npz"))
    cfg = O.default_cfg(**BCM)
    B, seed = int(fx["B"]), int(fx["seed"])
    obs = torch.rand(B, 3, 16, 16, generator=torch.Generator().manual_seed(seed + 1000)).cuda()
    masks = _seeded_masks(B, cfg.num_slots + 1, 16, seed).cuda()
    noise = O.make_noise(cfg, B, seed)
    model = build_wrapper(cfg, O.formula_params(cfg))
    model._module.inject_noise(dict(slots=noise["slots"].cuda()))
    m = model._module.get_loss(obs, masks)
    assert isinstance(m["ari"], float) and abs(m["ari"] - float(fx["ari"])) < 1e-6
    cpu = _cpu_path(masks, model._module._attns_image(B))
    assert m["ari"] == float(np.mean(cpu))
    assert model._module.last_ari(masks) == cpu
    # the SLATE branch reports no ari (slate_module.py:231); last_ari gives it to the evaluation script
    cfg2 = O.default_cfg(**dict(BCM, use_bcdec=False))
    model2 = build_wrapper(cfg2, O.formula_params(cfg2))
    model2._module.update_tau(0)
    m2 = model2._module.get_loss(obs, masks)
    assert "ari" not in m2
    assert model2._module.last_ari(masks) == _cpu_path(masks, model2._module._attns_image(B))


def test_iodine_get_loss_reports_the_device_ari():
    from types import SimpleNamespace as NS
    from ocrl_amd import ocrs
    from oracle import iodine_oracle as IO
    from tests.test_gpu_iodine import TINY
    cfg = IO.default_cfg(**TINY)
    ocr = NS(name="Iodine", slot_size=cfg.slot_size, num_iterations=cfg.num_iterations, num_slots=cfg.num_slots, img_channels=3, sigma=cfg.sigma,
             beta=cfg.beta, layer_norm=True, ref_cnn_hidden_size=64, ref_mlp_hidden_size=256, ref_cnn_layers=4, ref_cnn_kernel_size=3,
             ref_cnn_stride_size=2, dec_cnn_hidden_size=64, dec_cnn_layers=4, dec_cnn_kernel_size=3, learning=NS(lr=3e-4, clip=5.0, clip_norm_type=2.0))
    torch.manual_seed(0)
    model = ocrs.Iodine(ocr, NS(obs_size=cfg.obs_size, obs_channels=3))
    model.to("cuda:0")
    B, K, S = 4, cfg.num_slots, cfg.obs_size
    obs = torch.rand(B, 3, S, S, device="cuda")
    ids = torch.randint(0, K + 1, (B, S, S), device="cuda")
    masks = torch.nn.functional.one_hot(ids, K + 1).permute(0, 3, 1, 2)[:, :, None].float()
    m = model.get_loss(obs, masks)
    cpu = _cpu_path(masks, model._module.engine.tensor("masks", (B, K, 1, S, S)))
    assert isinstance(m["ari"], float) and m["ari"] == float(np.mean(cpu))
    assert model._module.last_ari(masks) == cpu


TINY_RUN = {
    "slate": ["ocr=slate", "ocr.dvae.vocab_size=256", "ocr.tfdec.num_dec_blocks=1", "ocr.slotattr.num_iterations=2"],
    "slotattn": ["ocr=slotattn", "ocr.dvae.vocab_size=256", "ocr.tfdec.num_dec_blocks=1", "ocr.slotattr.num_iterations=2"],
    "iodine": ["ocr=iodine", "ocr.num_slots=3", "ocr.num_iterations=2"],
}


def _run_args(kind, tmp_path, extra=()):
    return TINY_RUN[kind] + ["dataset=random-N5C4S4S2", "dataset.obs_size=16", "dataset.with_masks=True", "dataset.synthetic_val=10",
                             "dataset.synthetic_train=4", "batch_size=4", "num_workers=0", "device=cuda:0", f"run_dir={tmp_path / 'run'}",
                             f"ocr_checkpoint.local_file={tmp_path / 'model.pth'}"] + list(extra)


def _fresh_model(config, ckpt):
    from ocrl_amd import ocrs
    ocr = getattr(ocrs, config.ocr.name)(config.ocr, config.dataset)
    ocr._module._max_batch = config.batch_size
    if ckpt is not None:
        ocr.load(torch.load(ckpt, map_location="cpu", weights_only=True))
    ocr.to(config.device)
    ocr.eval()
    return ocr


@pytest.mark.parametrize("kind", ["slate", "slotattn", "iodine"])
def test_get_ari_mse_end_to_end(kind, tmp_path, monkeypatch):
    import get_ari_mse
    from ocrl_amd.utils.config import compose
    from ocrl_amd.utils.datasets import get_dataloaders
    from train_ocr import batch_inputs
    config = compose(os.path.join(ROOT, "configs"), "get_ari_mse", _run_args(kind, tmp_path))
    torch.manual_seed(123)
    src = _fresh_model(config, None)
    torch.save({"step": 0, "epoch": 0, "best_val_loss": 1.0, **src.save()}, tmp_path / "model.pth")
    out = get_ari_mse.main(_run_args(kind, tmp_path))
    disk = json.load(open(tmp_path / "run" / "ari_mse.json"))
    assert disk == out and sorted(disk) == ["ari", "mse", "num_images"] and disk["num_images"] == 10
    # the same loop by hand: a fresh model from the same checkpoint, per-image ARI from the numpy path on the model's own maps
    model = _fresh_model(config, tmp_path / "model.pth")
    _, val_dl = get_dataloaders(config.dataset, config.batch_size, 0, seed=config.seed)
    ari, mse, sizes = 0.0, 0.0, []
    for batch in val_dl:
        obs, masks = batch_inputs(batch, config.device)
        B, mod = obs.shape[0], model._module
        if kind == "slate":
            m = model.get_loss(obs, masks, with_mse=True)
            per_image = _cpu_path(masks, mod._attns_image(B))
            ari += float(np.sum(per_image))                                   # no ari in the metrics: the per-image values are summed
        elif kind == "slotattn":
            m = model.get_loss(obs, masks)
            ari += float(np.mean(_cpu_path(masks, mod._attns_image(B)))) * B   # the batch mean the metrics carry, weighted by its images
        else:
            m = model.get_loss(obs, masks)
            ari += float(np.mean(_cpu_path(masks, mod.engine.tensor("masks", (B, mod.num_slots, 1, 16, 16))))) * B
        mse += float(m["mse"]) * B
        sizes.append(B)
    assert sizes == [4, 4, 2]
    log(f"[get_ari_mse] {kind}: ari {disk['ari']:.6f} (by hand {ari / 10:.6f}), mse {disk['mse']:.6f} (by hand {mse / 10:.6f})")
    assert disk["mse"] == mse / 10 and disk["ari"] == ari / 10
    if kind != "slate":
        return
    # the background stored in channel 0 and named by bg_mask_idx: the same ari as the run above

    def rotated(batch, device):
        obs, masks = batch_inputs(batch, device)
        return obs, masks[:, [masks.shape[1] - 1] + list(range(masks.shape[1] - 1))]

    monkeypatch.setattr(get_ari_mse, "batch_inputs", rotated)
    out0 = get_ari_mse.main(_run_args(kind, tmp_path, ["bg_mask_idx=0"]))
    assert out0["ari"] == disk["ari"] and out0["mse"] == disk["mse"] and out0["num_images"] == 10


def test_get_ari_mse_needs_masks(tmp_path):
    import get_ari_mse
    args = [a for a in _run_args("slotattn", tmp_path) if not a.startswith(("dataset.with_masks", "ocr_checkpoint"))]
    with pytest.raises(RuntimeError, match="with_masks"):
        get_ari_mse.main(args)
    with pytest.raises(RuntimeError, match="wandb"):
        get_ari_mse.main(args + ["dataset.with_masks=True", "ocr_checkpoint.run_id=abc"])
