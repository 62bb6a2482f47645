"""The ``nn.Module`` container both stateful encoders (``SLATE_Module``, ``Iodine_Module``) are built on.

The module holds Parameters under the reference's dotted names so that ``parameters()``, ``state_dict()`` and checkpoints
match it; once it is on the GPU they are views into the flat buffers of an engine (``ocrl_amd.engine``), which is rebuilt
when a larger batch arrives.  A subclass names its engine class and keeps what is its own."""
import torch
from torch import nn


class _Holder(nn.Module):
    """plain container node used to reproduce the reference's dotted state_dict names"""


class FlatParamModule(nn.Module):
    engine_cls = None       # ocrl_amd.engine.Engine subclass
    backend = None          # the model's name in error messages
    engine = None           # built by .to(device); rebuilt when a batch exceeds _max_batch
    _max_batch = 0
    _seed = 0
    _step_seed = 0
    _injected_noise = None

    # ---- container plumbing
    def _query_spec(self):
        return self.engine_cls.param_spec(self._dims)

    def _get(self, path):
        node = self
        for part in path.split("."):
            if part not in node._modules:
                node.add_module(part, _Holder())
            node = node._modules[part]
        return node

    def _register(self, name, param, first=False):
        path, leaf = name.rsplit(".", 1) if "." in name else ("", name)
        node = self._get(path) if path else self
        node.register_parameter(leaf, param)
        if first:       # the parameter is the node's first attribute in the reference -> first in state_dict order
            items = list(node._parameters.items())
            node._parameters.clear()
            node._parameters[leaf] = param
            for k, v in items:
                if k != leaf:
                    node._parameters[k] = v

    # ---- device placement: parameters become views of the library's flat buffer
    def to(self, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"ocrl_amd {self.backend} runs on an AMD GPU only (got device={device!r}); there is no CPU path")
        self._device = dev
        self._ensure_engine(max(self._max_batch, 1))
        return self

    def _grad_view(self, eng, p):
        """what parameter p's .grad becomes: its slice of the flat gradient buffer"""
        return eng.view(eng.flat_g, p)

    def _engine_built(self, eng):
        """the new engine holds the parameters and is self.engine: whatever else has to follow it"""

    def _ensure_engine(self, batch):
        if self.engine is not None and batch <= self._max_batch:
            return
        old = self.engine
        eng = self.engine_cls(self._dims, max_batch=batch, device=self._device)
        named = dict(self.named_parameters())
        for p in eng.params:
            eng.view(eng.flat_p, p).copy_(named[p.name].data.to(eng.device))
        if old is not None:
            eng.flat_m.copy_(old.flat_m)
            eng.flat_v.copy_(old.flat_v)
            eng.adam_step = old.adam_step
        for p in eng.params:
            named[p.name].data = eng.view(eng.flat_p, p)
            named[p.name].grad = self._grad_view(eng, p)
        self.engine = eng
        self._max_batch = batch
        self._engine_built(eng)
        pending, self._pending_opt = getattr(self, "_pending_opt", None), None
        if pending is not None:       # optimiser state loaded before .to(device), as the reference's callers do (sb3s/ocr_extractor.py:33-36)
            pending[0].load_state_dict(pending[1])
        torch.cuda.synchronize(eng.device)

    def _need(self, obs):
        if getattr(self, "_device", None) is None:
            raise RuntimeError("call .to('cuda:N') before using the HIP backend")
        if not obs.is_cuda:
            raise RuntimeError("ocrl_amd: observations must live on the GPU (to_device(batch, device))")
        self._ensure_engine(obs.shape[0])
        return obs.contiguous().float()

    def set_seed(self, seed: int) -> None:
        self._seed = int(seed)
        self._step_seed = 0
