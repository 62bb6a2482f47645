"""MLP-classifier entry point (the reference ships configs/train_classifier.yaml and `num_labels` in its dataset configs but no script
and no module; this loop and the model are the project's own, shaped like train_property_predictor.py):

    python train_classifier.py ocr=slate pooling=transformer dataset=target-N4C4S3S1 dataset.with_objs=True \
        pooling.ocr_checkpoint.local_file=outputs/train_ocr/SLATE-TargetN4C4S3S1/checkpoints/model_best.pth device=cuda:0

Builds the encoder and the pooling head (which loads the pre-trained encoder from pooling.ocr_checkpoint.local_file), trains the
classifier on the pooled representation against the scenes' `labels` (ocrl_amd.utils.classifier, HIP), evaluates every eval_interval
steps and writes checkpoints in train_ocr.py's layout (model_<step>.pth / model_latest.pth / model_best.pth with step, epoch,
best_val_loss, classifier_module_state_dict, classifier_opt_state_dict and the pooling head's and the encoder's keys).
"""
import json
import logging
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from ocrl_amd import ocrs, poolings  # noqa: E402
from ocrl_amd.utils.classifier import Classifier  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402
from ocrl_amd.utils.datasets import get_dataloaders  # noqa: E402
from ocrl_amd.utils.tools import get_item, to_device  # noqa: E402
from train_ocr import batch_inputs, save  # noqa: E402

log = logging.getLogger("train_classifier")


def classifier_batch(batch, device):
    if "labels" not in batch:
        raise RuntimeError("the dataset carries no labels: set dataset.with_objs=True on a task dataset (target-*, odd-one-out-*); "
                           "random-N5C4S4S2 has no target")
    return {"obss": batch_inputs(batch, device)[0], "labels": to_device(batch["labels"], device)}


def evaluate(model, val_dl, device):
    with torch.no_grad():
        metrics = [{k: get_item(v) for k, v in model.get_loss(classifier_batch(batch, device)).items()} for batch in val_dl]
    return {k: float(np.mean([np.mean(m[k]) for m in metrics])) for k in metrics[0]}


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    config = compose(os.path.join(ROOT, "configs"), "train_classifier", argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    os.makedirs(config.run_dir, exist_ok=True)
    logf = open(os.path.join(config.run_dir, "metrics.jsonl"), "a")

    def logger(d, step):
        logf.write(json.dumps({"step": step, **{k: float(np.mean(v)) for k, v in d.items()}}) + "\n")
        logf.flush()

    np.random.seed(config.seed)
    torch.manual_seed(config.seed)
    train_dl, val_dl = get_dataloaders(config.dataset, config.batch_size, config.num_workers, seed=config.seed, device=config.device)
    ocr = getattr(ocrs, config.ocr.name)(config.ocr, config.dataset)
    if hasattr(ocr._module, "_max_batch"):
        ocr._module._max_batch = config.batch_size
    pooling = getattr(poolings, config.pooling.name)(ocr, config.pooling)        # loads pooling.ocr_checkpoint.local_file
    model = Classifier(pooling, config.classifier, config.dataset)
    model.to(config.device)
    step, epoch, best_val_loss = 0, 0, 1e10
    log.info(f"classifying {config.dataset.name} from {config.ocr.name} + {config.pooling.name}: batch {config.batch_size}, "
             f"d_model {config.classifier.d_model}, {config.dataset.num_labels} labels")
    done = False
    while epoch < config.max_epochs and not done:
        model.train()
        for batch in train_dl:
            metrics = model.update(classifier_batch(batch, config.device), step)
            if step % config.log_interval == 0:
                vals = {f"train/{k}": get_item(v) for k, v in metrics.items()}
                logger(vals, step)
                log.info(f"step {step} " + " / ".join(f"{k} {float(np.mean(v)):.4f}" for k, v in vals.items()))
            step += 1
            if step % config.eval_interval == 0:
                model.eval()
                out = evaluate(model, val_dl, config.device)
                model.train()
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
    logf.close()
    return step


if __name__ == "__main__":
    main()
