"""Segmentation-quality evaluation of a pre-trained encoder (the reference ships configs/get_ari_mse.yaml but no script; this loop is the
project's own, shaped like train_property_predictor.py):

    python get_ari_mse.py ocr=slate dataset=random-N5C4S4S2 dataset.with_masks=True \
        ocr_checkpoint.local_file=outputs/train_ocr/SLATE-RandomN5C4S4S2/checkpoints/model_best.pth device=cuda:0

Loads the encoder, runs it in eval() over the validation set and writes <run_dir>/ari_mse.json: the adjusted Rand index of the slot maps
against the ground-truth masks (ocrl_ari_counts on the GPU) and the reconstruction error, both as means over the images.  SLATE reports
the autoregressive reconstruction error (get_loss(..., with_mse=True)); Slot-Attention and IODINE the error of their decoder.
"""
import json
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from ocrl_amd import ocrs  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from ocrl_amd.utils.datasets import get_dataloaders  # noqa: E402
from train_ocr import batch_inputs  # noqa: E402

log = logging.getLogger("get_ari_mse")


def background_last(masks, bg_mask_idx):
    """masks [B, Ct, 1, H, W] with the background in channel bg_mask_idx -> the same masks with that channel moved last, which is where
    the foreground masking of the encoders reads it; -1 and Ct - 1 change nothing"""
    Ct = masks.shape[1]
    if not -Ct <= bg_mask_idx < Ct:
        raise RuntimeError(f"bg_mask_idx={bg_mask_idx}: the dataset's masks have {Ct} channels")
    bg = bg_mask_idx % Ct
    if bg == Ct - 1:
        return masks
    return masks[:, [c for c in range(Ct) if c != bg] + [bg]]


def eval_batch(ocr, batch, device, bg_mask_idx):
    """-> (sum of the per-image ARIs, sum of the per-image mse, images) of one batch"""
    if "masks" not in batch:
        raise RuntimeError("the dataset carries no masks: set dataset.with_masks=True (synthetic scenes) or use an HDF5 file with a `masks` key")
    obs, masks = batch_inputs(batch, device)
    masks = background_last(masks, bg_mask_idx)
    B = obs.shape[0]
    mod = ocr._module
    with torch.no_grad():
        if isinstance(ocr, ocrs.SLATE) and not mod._use_bcdec:
            m = ocr.get_loss(obs, masks, with_mse=True)
        else:
            m = ocr.get_loss(obs, masks)
    ari = float(m["ari"]) * B if "ari" in m else float(np.sum(mod.last_ari(masks)))
    return ari, float(m["mse"]) * B, B


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    config = compose(os.path.join(ROOT, "configs"), "get_ari_mse", argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    os.makedirs(config.run_dir, exist_ok=True)
    np.random.seed(config.seed)
    torch.manual_seed(config.seed)
    _, val_dl = get_dataloaders(config.dataset, config.batch_size, config.num_workers, seed=config.seed, device=config.device)
    ocr = getattr(ocrs, config.ocr.name)(config.ocr, config.dataset)
    if not hasattr(ocr._module, "last_ari"):
        raise RuntimeError(f"ocr={config.ocr.name} produces no slot maps: the ARI is defined for SLATE, Slot-Attention and IODINE")
    if hasattr(ocr._module, "_max_batch"):
        ocr._module._max_batch = config.batch_size
    if config.ocr_checkpoint.local_file:
        ocr.load(torch.load(config.ocr_checkpoint.local_file, map_location="cpu", weights_only=True))
    elif config.ocr_checkpoint.run_id:
        raise RuntimeError("ocr_checkpoint.run_id needs wandb; download the file and set ocr_checkpoint.local_file")
    ocr.to(config.device)
    ocr.eval()
    ari, mse, n = 0.0, 0.0, 0
    for batch in val_dl:
        a, m, b = eval_batch(ocr, batch, config.device, int(config.bg_mask_idx))
        ari, mse, n = ari + a, mse + m, n + b
    out = {"ari": ari / n, "mse": mse / n, "num_images": n}
    with open(os.path.join(config.run_dir, "ari_mse.json"), "w") as f:
        json.dump(out, f)
    log.info(f"{config.ocr.name} on {config.dataset.name}: ari {out['ari']:.6f} / mse {out['mse']:.6f} over {n} images")
    return out


if __name__ == "__main__":
    main()
