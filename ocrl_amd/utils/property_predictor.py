"""Slot property probe (the reference's utils/property_predictor.py:12-232): a small head reads every slot of a frozen, pre-trained
encoder and predicts the colour, shape, scale and position of an object; slots are matched to the ground-truth objects by an exact
minimum-cost assignment and the matched loss trains the head.

``PropertyPredictor._module`` is the reference's ``nn.Sequential`` (same parameter names, shapes and default initialisation, so
checkpoints load both ways); its ``forward`` is never called.  The arithmetic -- head, cost matrix, assignment, loss, metrics and
gradients -- is ``ocrl_probe_fwd/_bwd`` (HIP) behind a ``torch.autograd.Function``: no host copy between the encoder and the loss, no
CPU fallback (a CPU tensor raises), and ``get_loss`` returns device tensors.

Kept from the reference: the soft-max is taken twice on the class outputs, the loss is a sum over images and objects, ``R^2_xy`` and
``mse_xy`` are its formulas, ``matching_mode`` is read and unused.  Different on purpose: the encoder is called under
``torch.no_grad()`` with frozen weights and ``update`` does not step the encoder's optimiser (the reference steps it on zero
gradients, which moves a loaded encoder by its Adam momentum)."""
from types import SimpleNamespace

import torch
from torch import nn

from .. import _bridge, _lib
from .._bridge import ints as _ints

_WHO = "ocrl_amd.PropertyPredictor"
SLOT_ENCODERS = ("SLATE", "SlotAttn", "Iodine")
MAX_SLOTS = _lib.CONSTANTS["OCRL_PROBE_MAX_SLOTS"]


def property_indices(property_list, properties):
    """property_predictor.py:53-73 -> (target ranges, output ranges, kinds); kind 1 is xy"""
    tgt, out, kind = [], [], []
    t = o = 0
    for name in property_list:
        cfg = properties[name]
        if name == "xy":
            if int(cfg.dims) != 2:
                raise ValueError(f"the xy property needs dims: 2 (got {cfg.dims}); its targets are two coordinates")
            tgt.append([t, t + 2]); out.append([o, o + 2]); kind.append(1)
        else:
            tgt.append([t, t + 1]); out.append([o, o + int(cfg.num_candidates)]); kind.append(0)
        t, o = tgt[-1][1], out[-1][1]
    return tgt, out, kind


class _ProbeFn(torch.autograd.Function):
    """(rows, y, spec, *params) -> loss, out [B, K, O], cost [B, N, K], col [B, N], metrics [P + 2]; only the loss is differentiable,
    and only towards the parameters"""

    @staticmethod
    def forward(ctx, rows, y, spec, *params):
        rows, ps = _bridge.inputs(_WHO, rows.detach(), params)
        y = _bridge.gpu_input(_WHO, y)
        L, dev = _lib.lib(), rows.device
        B, N, T = y.shape
        K, O, D, P = spec.K, spec.O, rows.shape[-1], len(spec.kind)
        if N > K:
            raise ValueError(f"{_WHO}: {N} objects cannot be matched to {K} slots")
        head = (B, K, N, D, O, int(spec.slot_rows), len(spec.dims), _ints(spec.dims))
        ws = _bridge.workspace(_WHO, L.ocrl_probe_ws_floats(*head, P), dev, f"batch {B}, {K} slots (at most {MAX_SLOTS}), {N} objects, "
                               f"rep_dim {D}, {O} outputs per slot, head widths {list(spec.dims)}")
        out = torch.empty(B, K, O, device=dev, dtype=torch.float32)
        cost = torch.empty(B, N, K, device=dev, dtype=torch.float32)
        col = torch.empty(B, N, device=dev, dtype=torch.int32)
        metrics = torch.empty(P + 2, device=dev, dtype=torch.float32)
        _bridge.launch(dev, L.ocrl_probe_fwd, _lib.ptr(rows), _lib.ptrs(ps), _lib.ptr(y), _lib.ptr(out), _lib.ptr(cost), _lib.ptr(col),
                       _lib.ptr(metrics), B, K, N, D, T, O, *head[5:], spec.slope, P, _ints(sum(spec.tgt, [])), _ints(sum(spec.out, [])),
                       _ints(spec.kind), _lib.ptr(ws), ws.numel())
        ctx.save_for_backward(rows, *ps)
        ctx.args, ctx.ws = (*head, spec.slope, P), ws
        ctx.mark_non_differentiable(out, cost, col, metrics)
        return metrics[0].clone(), out, cost, col, metrics

    @staticmethod
    def backward(ctx, dloss, *_):
        rows, *ps = ctx.saved_tensors
        dloss = _bridge.cotangent(dloss)
        gs = [torch.empty_like(p) for p in ps]
        _bridge.launch(rows.device, _lib.lib().ocrl_probe_bwd, _lib.ptr(rows), _lib.ptr(dloss), _lib.ptrs(ps), _lib.ptrs(gs), *ctx.args,
                       _lib.ptr(ctx.ws), ctx.ws.numel())
        return (None, None, None, *gs)


def probe_match(out, y, tgt, outr, kind, dloss=None, want_grad=True):
    """ocrl_probe_match on head outputs a host brings itself: out [B, K, O], y [B, N, T] on the GPU ->
    dict(cost [B, N, K], col [B, N] int32, metrics [P + 2], dout [B, K, O] or None)"""
    out, y = _bridge.gpu_input("ocrl_amd.probe_match", out), _bridge.gpu_input("ocrl_amd.probe_match", y)
    L, dev = _lib.lib(), out.device
    (B, K, O), (_, N, T) = out.shape, y.shape
    P = len(kind)
    ws = _bridge.workspace("ocrl_amd.probe_match", L.ocrl_probe_match_ws_floats(B, P), dev, f"batch {B}, {P} properties",
                           reason="the batch must be at least 1 and the properties 1 .. 8")
    cost = torch.empty(B, N, K, device=dev, dtype=torch.float32)
    col = torch.empty(B, N, device=dev, dtype=torch.int32)
    metrics = torch.empty(P + 2, device=dev, dtype=torch.float32)
    dout = torch.zeros_like(out) if want_grad else None
    _bridge.launch(dev, L.ocrl_probe_match, _lib.ptr(out), O, K * O, _lib.ptr(y), _lib.ptr(dloss), _lib.ptr(cost), _lib.ptr(col), _lib.ptr(metrics),
                   _lib.ptr(dout), B, K, N, T, O, P, _ints(sum(tgt, [])), _ints(sum(outr, [])), _ints(kind), _lib.ptr(ws), ws.numel())
    return dict(cost=cost, col=col, metrics=metrics, dout=dout)


class PropertyPredictor:
    def __init__(self, ocr, config, dataset_config) -> None:
        self._property_list = list(dataset_config.property_order_in_state)
        self._matching_mode = config.matching_mode                   # read and unused, as in the reference
        self._target_prop_indices, self._output_prop_indices, self._kinds = property_indices(self._property_list, dataset_config.properties)
        per_slot = self._output_prop_indices[-1][1]
        if ocr.name in SLOT_ENCODERS:
            input_size = self._input_size = ocr.rep_dim
            output_size = self._output_size = per_slot
            self._use_slot = True
        elif ocr.name in ["VAE"]:
            self._num_slots_for_dist_rep = int(config.num_slots_for_dist_rep)
            input_size = self._input_size = ocr.rep_dim
            output_size = self._output_size = per_slot * self._num_slots_for_dist_rep
            self._use_slot = False
        else:
            raise ValueError(f"{ocr.name} is not supported to predict property.")
        self._per_slot = per_slot
        self._encoder = ocr
        if config.model_type == "linear":
            self._module = nn.Sequential(nn.Linear(input_size, output_size))
        elif config.model_type == "mlp3":
            hidden_size = 256
            self._module = nn.Sequential(
                nn.Linear(input_size, hidden_size), nn.LeakyReLU(),
                nn.Linear(hidden_size, hidden_size), nn.LeakyReLU(),
                nn.Linear(hidden_size, hidden_size), nn.LeakyReLU(),
                nn.Linear(hidden_size, output_size),
            )
        else:
            raise ValueError(f"model_type must be linear or mlp3 (got {config.model_type})")
        self._opt = torch.optim.Adam(self._module.parameters(), lr=config.learning.lr)
        self.last_matching = None                                    # col [B, N] int32 of the latest get_loss (device tensor)

    def wandb_watch(self, config):
        try:
            import wandb
            wandb.watch(self._module, log=getattr(config, "log", None))
        except Exception:
            pass

    def _linears(self):
        return [m for m in self._module if isinstance(m, nn.Linear)]

    def _spec(self, K):
        lin = self._linears()
        slopes = [m.negative_slope for m in self._module if isinstance(m, nn.LeakyReLU)]
        return SimpleNamespace(K=K, O=self._per_slot, slot_rows=self._use_slot, dims=[m.out_features for m in lin],
                               slope=float(slopes[0]) if slopes else 0.01, tgt=self._target_prop_indices, out=self._output_prop_indices,
                               kind=self._kinds)

    def _encode(self, obs):
        mod = getattr(self._encoder, "_module", None)
        if mod is not None and hasattr(mod, "freeze_weights") and not getattr(mod, "_frozen", False):
            mod.freeze_weights(True)                                 # constant weights: no re-packing per call (as OCRExtractor)
        with torch.no_grad():
            x = self._encoder(obs)
        return x.detach()

    def get_loss(self, batch) -> dict:
        y = batch["objs"]
        x = self._encode(batch["obss"])
        if self._use_slot:
            B, K, D = x.shape
            rows = x.reshape(B * K, D)
        else:
            B, D = x.shape
            K, rows = self._num_slots_for_dist_rep, x
        if y.shape[1] > K:
            raise ValueError(f"{_WHO}: {y.shape[1]} objects cannot be matched to {K} slots")
        params = [p for m in self._linears() for p in (m.weight, m.bias)]
        loss, out, cost, col, m = _ProbeFn.apply(rows, y, self._spec(K), *params)
        self.last_matching, self.last_output, self.last_cost = col, out, cost
        metrics = {"loss": loss}
        for i, name in enumerate(self._property_list):
            if self._kinds[i]:
                metrics[f"R^2_{name}"] = m[1 + i]
                metrics[f"mse_{name}"] = m[len(self._kinds) + 1]
            else:
                metrics[f"acc_{name}"] = m[1 + i]
        return metrics

    def train(self) -> None:
        self._module.train()
        self._encoder.train()
        return None

    def eval(self) -> None:
        self._module.eval()
        self._encoder.eval()
        return None

    def to(self, device) -> None:
        self._module.to(device)
        self._encoder.to(device)

    def get_samples(self, obs) -> dict:
        return self._encoder.get_samples(obs)

    def update(self, batch, step: int) -> dict:
        metrics = self.get_loss(batch)
        self._opt.zero_grad()
        metrics["loss"].backward()
        self._opt.step()                                             # the head alone: the encoder is frozen
        return metrics

    def save(self) -> dict:
        checkpoint = {}
        checkpoint["property_predictor_module_state_dict"] = self._module.state_dict()
        checkpoint["property_predictor_opt_state_dict"] = self._opt.state_dict()
        checkpoint.update(self._encoder.save())
        return checkpoint

    def load(self, checkpoint) -> None:
        self._module.load_state_dict(checkpoint["property_predictor_module_state_dict"])
        self._opt.load_state_dict(checkpoint["property_predictor_opt_state_dict"])
        self._encoder.load(checkpoint)
