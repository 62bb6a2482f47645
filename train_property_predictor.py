"""Property-probe entry point (the reference ships configs/train_property_predictor.yaml and utils/property_predictor.py but no
script; this loop is the project's own, shaped like train_ocr.py):

    python train_property_predictor.py ocr=slate dataset=random-N5C4S4S2 dataset.with_objs=True \
        ocr_checkpoint.local_file=outputs/train_ocr/SLATE-RandomN5C4S4S2/checkpoints/model_best.pth device=cuda:0

Loads the pre-trained encoder, trains the probe head on the frozen encoder (ocrl_amd.utils.property_predictor, HIP), evaluates every
eval_interval steps and writes checkpoints in train_ocr.py's layout (model_<step>.pth / model_latest.pth / model_best.pth with step,
epoch, best_val_loss, property_predictor_module_state_dict, property_predictor_opt_state_dict and the encoder's keys).
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
from ocrl_amd.utils.property_predictor import PropertyPredictor  # noqa: E402
from ocrl_amd.utils.tools import get_item, to_device  # noqa: E402
from train_ocr import batch_inputs, save  # noqa: E402

log = logging.getLogger("train_property_predictor")


def probe_batch(batch, device):
    if "objs" not in batch:
        raise RuntimeError("the dataset carries no object states: set dataset.with_objs=True (synthetic scenes) or use an HDF5 file with an `objs` key")
    return {"obss": batch_inputs(batch, device)[0], "objs": to_device(batch["objs"], device)}


def evaluate(model, val_dl, device):
    metrics = [{k: get_item(v) for k, v in model.get_loss(probe_batch(batch, device)).items()} for batch in val_dl]
    return {k: float(np.mean([m[k] for m in metrics])) for k in metrics[0]}


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    config = compose(os.path.join(ROOT, "configs"), "train_property_predictor", argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    os.makedirs(config.run_dir, exist_ok=True)
    logf = open(os.path.join(config.run_dir, "metrics.jsonl"), "a")

    def logger(d, step):
        logf.write(json.dumps({"step": step, **{k: float(v) for k, v in d.items()}}) + "\n")
        logf.flush()

    np.random.seed(config.seed)
    torch.manual_seed(config.seed)
    train_dl, val_dl = get_dataloaders(config.dataset, config.batch_size, config.num_workers, seed=config.seed, device=config.device)
    ocr = getattr(ocrs, config.ocr.name)(config.ocr, config.dataset)
    if hasattr(ocr._module, "_max_batch"):
        ocr._module._max_batch = config.batch_size
    if config.ocr_checkpoint.local_file:
        ocr.load(torch.load(config.ocr_checkpoint.local_file, map_location="cpu", weights_only=True))
    elif config.ocr_checkpoint.run_id:
        raise RuntimeError("ocr_checkpoint.run_id needs wandb; download the file and set ocr_checkpoint.local_file")
    model = PropertyPredictor(ocr, config.property_predictor, config.dataset)
    model.to(config.device)
    model.eval()                                          # the encoder is frozen; the head has no train-time behaviour
    step, epoch, best_val_loss = 0, 0, 1e10
    log.info(f"probing {config.ocr.name} on {config.dataset.name}: batch {config.batch_size}, head {config.property_predictor.model_type}")
    done = False
    while epoch < config.max_epochs and not done:
        for batch in train_dl:
            metrics = model.update(probe_batch(batch, config.device), step)
            if step % config.log_interval == 0:
                vals = {f"train/{k}": get_item(v) for k, v in metrics.items()}
                logger(vals, step)
                log.info(f"step {step} " + " / ".join(f"{k} {float(v):.4f}" for k, v in vals.items()))
            step += 1
            if step % config.eval_interval == 0:
                out = evaluate(model, val_dl, config.device)
                best = out["loss"] < best_val_loss
                best_val_loss = min(best_val_loss, out["loss"])
                logger({f"val/{k}": v for k, v in out.items()}, step)
                log.info(f"[Epoch {epoch}, Step {step}] " + " / ".join(f"val/{k} {v:.4f}" for k, v in out.items()))
                save(model, config.run_dir, step=step, epoch=epoch, best_val_loss=best_val_loss, best=best)
            if config.max_steps is not None and step >= config.max_steps:
                done = True
                break
        epoch += 1
    if config.max_steps is None or step % config.eval_interval != 0:
        save(model, config.run_dir, step=step, epoch=epoch, best_val_loss=best_val_loss, best=False)
    return step


if __name__ == "__main__":
    main()
