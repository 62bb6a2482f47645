"""Encoder wrapper API of the reference (ocrs/base.py:8-88), kept verbatim at the Python surface.
Subclasses own ``_module`` (parameters, state_dict) and ``_opt``; the arithmetic is in libocrl_hip."""
import torch
from torch.nn.utils import clip_grad_norm_

from ..dist_utils import active_dist


class Base:
    def __init__(self, ocr_config, env_config) -> None:
        self.name = ocr_config.name
        self._config = ocr_config
        self._obs_size = env_config.obs_size
        self._obs_channels = env_config.obs_channels
        # for pooling layer (ocrs/base.py:16-18)
        self.rep_dim = self._module.rep_dim
        self.num_slots = self._module.num_slots

    def __call__(self, obs):
        return self._module(obs)

    def wandb_watch(self, config):
        """wandb.watch(module) in the reference (base.py:30-31); optional here (wandb is not required)."""
        try:
            import wandb
            wandb.watch(self._module, log=getattr(config, "log", None))
        except Exception:
            pass

    def get_loss(self, obs, with_rep=False):
        return self._module.get_loss(obs, with_rep)

    def train(self) -> None:
        self._module.train()
        return None

    def eval(self) -> None:
        self._module.eval()
        return None

    def to(self, device) -> None:
        self._module.to(device)

    def set_zero_grad(self):
        if hasattr(self, "_opt"):
            self._opt.zero_grad()

    def do_step(self):
        if hasattr(self, "_opt"):
            self._opt.step()

    def get_samples(self, obs) -> dict:
        return self._module.get_samples(obs)

    def save(self) -> dict:
        checkpoint = {"ocr_module_state_dict": self._module.state_dict()}
        if hasattr(self, "_opt"):
            checkpoint["ocr_opt_state_dict"] = self._opt.state_dict()
        return checkpoint

    def load(self, checkpoint) -> None:
        self._module.load_state_dict(checkpoint["ocr_module_state_dict"])
        if hasattr(self, "_opt") and "ocr_opt_state_dict" in checkpoint:
            self._opt.load_state_dict(checkpoint["ocr_opt_state_dict"])


class AutogradUpdate:
    """``to`` and ``update`` of the wrappers whose module trains through torch autograd and a torch optimiser in ``_opt`` (VAE, MAE)"""

    def to(self, device) -> None:
        self._module.to(device)
        if hasattr(self, "_opt"):                                 # optimizer_to (utils/tools.py) for a resumed state
            for st in self._opt.state.values():
                for k, v in st.items():
                    if torch.is_tensor(v):
                        st[k] = v.to(device)

    def update(self, obs, masks, step: int) -> dict:
        """ocrs/base.py:60-74: zero_grad, loss, backward, [gradient all-reduce], optional clip_grad_norm_, optimiser step"""
        if not hasattr(self, "_opt"):
            return {}
        self._opt.zero_grad()
        metrics = self._module.get_loss(obs)
        metrics["loss"].backward()
        dist = active_dist()
        if dist is not None:                                      # data-parallel: the mean gradient over the ranks
            for p in self._module.parameters():
                if p.grad is not None:
                    dist.all_reduce(p.grad, op=dist.ReduceOp.SUM)
                    p.grad.div_(dist.get_world_size())
        lr = self._config.learning
        if hasattr(lr, "clip"):
            norm_type = getattr(lr, "clip_norm_type", "inf")
            metrics["norm"] = clip_grad_norm_(self._module.parameters(), lr.clip, float(norm_type))
        self._opt.step()
        return metrics
