"""MLP classifier, the fourth downstream model the reference names (configs/train_classifier.yaml, ``num_labels`` in its dataset
configs): a small head reads the pooled representation of a scene and says which object is the target.

The reference ships the configs only, no module, so the model is this project's definition: one hidden layer,
``Linear(pooling.rep_dim, classifier.d_model) -> ReLU -> Linear(classifier.d_model, dataset.num_labels)``, trained with the soft-max
cross-entropy against ``labels`` (the target's row, which the task datasets made on the GPU return beside ``objs``) by Adam at
``classifier.learning.lr``.

``Classifier._module`` holds the parameters (state_dict keys ``0.weight, 0.bias, 2.weight, 2.bias``); its ``forward`` is never called.
The arithmetic -- head, loss, accuracy and gradients -- is ``ocrl_clf_ce_fwd_bwd`` (HIP, include/ocrl_hip_classifier.h) behind a
``torch.autograd.Function``: no CPU fallback (a CPU tensor raises), and ``get_loss`` returns device tensors.  Without a gradient to
take (``torch.no_grad()``, the validation pass) the same entry point evaluates: no backward is launched.

The representation comes through ``poolings.Base.__call__(obs, with_loss=True)``, so ``pooling.learn_downstream_loss`` and
``pooling.learn_aux_loss`` mean what they mean there; ``update`` zeroes and steps the pooling head's own Adam and, when one of the two
flags lets a gradient reach it, the encoder's optimiser.  A row whose label is outside [0, num_labels) adds nothing to the loss, the
accuracy or any gradient while the means keep the batch size as denominator; ``valid_rows`` counts the others."""
import ctypes

import torch
from torch import nn

from .. import _bridge, _lib
from ..ocrs.flat_module import FlatParamModule

_WHO = "ocrl_amd.Classifier"
MAX_LABELS, MAX_WIDTH = 64, 256          # of the head (include/ocrl_hip_dqn.h: the limits of ocrl_qnet_desc)
CLF_SCALARS = ("ce", "acc", "valid_rows")


class _ClfFn(torch.autograd.Function):
    """(features [B, F], labels [B], dims, acts, A, want_grad, *params) -> ce, scalars [3], logits [B, A]; only ``ce`` is differentiable,
    towards the features and the parameters.  The gradients are the forward's own outputs: the backward scales them.  ``want_grad`` is
    the caller's (grad mode cannot be read inside a forward, and ``needs_input_grad`` ignores it): False evaluates, with a null dw."""

    @staticmethod
    def forward(ctx, features, labels, dims, acts, A, want_grad, *params):
        x, ps = _bridge.inputs(_WHO, features, params)
        dev = x.device
        if x.dim() != 2:
            raise ValueError(f"{_WHO}: the pooled representation must be [B, rep_dim] (got {list(x.shape)})")
        B, F = x.shape
        labels = labels.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if labels.numel() != B:
            raise ValueError(f"{_WHO}: labels has {labels.numel()} entries for a batch of {B} ([B, 1] or [B] int64)")
        d = _lib.qnet_desc(B, F, A, dims, acts)
        ws = _bridge.workspace(_WHO, _lib.lib().ocrl_qnet_ws_floats(ctypes.byref(d)), dev,
                               f"batch {B}, rep_dim {F}, {A} labels, hidden widths {list(dims)}")
        need_grad = bool(want_grad)
        scal = torch.empty(3, device=dev, dtype=torch.float32)
        logits = torch.empty(B, A, device=dev, dtype=torch.float32)
        gs = [torch.empty_like(p) for p in ps] if need_grad else None
        dx = torch.empty_like(x) if need_grad and ctx.needs_input_grad[0] else None
        _bridge.launch(dev, _lib.lib().ocrl_clf_ce_fwd_bwd, ctypes.byref(d), _lib.ptr(x), _lib.ptrs(ps), _lib.ptr(labels), _lib.ptr(scal),
                       _lib.ptr(logits), _lib.ptr(dx), _lib.ptrs(gs) if need_grad else None, _lib.ptr(ws), ws.numel())
        ctx.gs, ctx.dx = gs, dx
        ctx.mark_non_differentiable(scal, logits)
        return scal[0].clone(), scal, logits

    @staticmethod
    def backward(ctx, gloss, _gscal, _glogits):
        dx = None if ctx.dx is None else ctx.dx * gloss
        return (dx, None, None, None, None, None, *[g * gloss for g in ctx.gs])


class Classifier:
    def __init__(self, pooling, config, dataset_config) -> None:
        num_labels, d_model = int(dataset_config.num_labels), int(config.d_model)
        task = dataset_config.get("task") if hasattr(dataset_config, "get") else getattr(dataset_config, "task", None)
        rng = (task if task is not None else dataset_config).num_objects_range
        if num_labels < int(rng[1]) or num_labels > MAX_LABELS:
            raise ValueError(f"{_WHO}: dataset.num_labels = {num_labels} must cover the {int(rng[1])} objects of num_objects_range {list(rng)} "
                             f"(a label is the target's row) and be at most {MAX_LABELS}")
        if d_model < 4 or d_model > MAX_WIDTH or d_model % 4:
            raise ValueError(f"{_WHO}: classifier.d_model must be a multiple of 4 in 4 .. {MAX_WIDTH} (got {d_model})")
        ocr = getattr(pooling, "_ocr", None)
        self._learn_aux_loss = bool(getattr(pooling, "_learn_aux_loss", False))
        self._learn_downstream_loss = bool(getattr(pooling, "_learn_downstream_loss", False))
        if self._learn_aux_loss and isinstance(getattr(ocr, "_module", None), FlatParamModule):
            raise NotImplementedError(f"{_WHO}: pooling.learn_aux_loss=True needs an encoder whose loss is a torch graph (VAE, MAE); "
                                      f"{ocr._module.backend}'s loss lives in the library's flat buffers and cannot be added to the cross-entropy")
        self._pooling = pooling
        self._num_labels, self._d_model = num_labels, d_model
        self._module = nn.Sequential(nn.Linear(int(pooling.rep_dim), d_model), nn.ReLU(), nn.Linear(d_model, num_labels))
        self._opt = torch.optim.Adam(self._module.parameters(), lr=config.learning.lr)
        self.last_logits = None                                      # logits [B, num_labels] of the latest get_loss (device tensor)

    def wandb_watch(self, config):
        try:
            import wandb
            wandb.watch(self._module, log=getattr(config, "log", None))
        except Exception:
            pass

    def _params(self):
        return [p for m in self._module if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]

    def get_loss(self, batch) -> dict:
        if "labels" not in batch:
            raise RuntimeError(f"{_WHO}: the batch carries no labels: set dataset.with_objs=True on a task dataset (target-*, odd-one-out-*)")
        state, metrics = self._pooling(batch["obss"], with_loss=True)
        params = self._params()
        want_grad = torch.is_grad_enabled() and (state.requires_grad or any(p.requires_grad for p in params))
        ce, scal, logits = _ClfFn.apply(state, batch["labels"], (self._d_model,), (1,), self._num_labels, want_grad, *params)      # act 1: ReLU
        self.last_logits = logits
        out = {"loss": ce + metrics["aux_loss"] if "aux_loss" in metrics else ce}
        out.update({k: scal[i] for i, k in enumerate(CLF_SCALARS)})
        out.update(metrics)
        return out

    def train(self) -> None:
        self._module.train()
        self._pooling.train()
        return None

    def eval(self) -> None:
        self._module.eval()
        self._pooling.eval()
        return None

    def to(self, device) -> None:
        self._module.to(device)
        self._pooling.to(device)

    def get_samples(self, obs) -> dict:
        return self._pooling.get_samples(obs)

    def update(self, batch, step: int) -> dict:
        self._opt.zero_grad()
        self._pooling.set_zero_grad()                                # the pooling head's and the encoder's
        metrics = self.get_loss(batch)
        metrics["loss"].backward()
        self._opt.step()
        if self._learn_downstream_loss or self._learn_aux_loss:
            self._pooling.do_step()
        elif hasattr(self._pooling, "_opt"):
            # no gradient reaches the encoder: stepping its optimiser on zeros would still move a loaded encoder by its Adam momentum
            # (the reference's habit, which utils/property_predictor.py drops for the same reason)
            self._pooling._opt.step()
        return metrics

    def save(self) -> dict:
        checkpoint = {}
        checkpoint["classifier_module_state_dict"] = self._module.state_dict()
        checkpoint["classifier_opt_state_dict"] = self._opt.state_dict()
        checkpoint.update(self._pooling.save())
        return checkpoint

    def load(self, checkpoint) -> None:
        self._module.load_state_dict(checkpoint["classifier_module_state_dict"])
        self._opt.load_state_dict(checkpoint["classifier_opt_state_dict"])
        self._pooling.load(checkpoint)
