"""MultipleCNN encoder (ocrs/multiple_cnns/multiple_cnn.py:10-17, multiple_cnn_module.py:12-38, configs/ocr/multiple_cnn.yaml):
``num_modules`` NatureCNN modules on the same image, their [B, rep_dim] outputs stacked on axis 1 -> [B, num_modules, rep_dim].

The modules live in ``_cnns`` (an ``nn.ModuleList`` of ``NatureCNN_Module``) for the reference's keys and initialisation; the forward is
one ``ocrl_naturecnn_fwd`` call over all of them (``groups`` = num_modules): the first convolution of every module in one launch, the
deeper ones as grouped convolutions, so G modules cost the launches of one plus one Linear GEMM per module.  Each module is built with
cnn_feat_size 4 and use_cnn_feat False on a copy of the config; the caller's config is left as it was."""
import torch
from torch import nn

from .base import Base
from .naturecnn import NatureCNN_Module, forced_config, run_naturecnn


class MultipleCNN_Module(nn.Module):
    trains_through_autograd = True                           # as NatureCNN_Module

    def __init__(self, ocr_config, env_config) -> None:
        super().__init__()
        self.rep_dim = int(ocr_config.rep_dim)
        self.num_slots = int(ocr_config.num_modules)
        self._use_cnn_feat = False
        self._obs_channels = env_config.obs_channels
        sub = forced_config(ocr_config)
        self._cnns = nn.ModuleList([NatureCNN_Module(sub, env_config) for _ in range(self.num_slots)])

    def _param_list(self):
        return [p for m in self._cnns for p in m._param_list()]     # module-major state_dict order

    def forward(self, obs):
        return run_naturecnn(obs, (self.num_slots, 4, 0, self.rep_dim), self._param_list(), self._obs_channels)

    def get_loss(self, obs, with_rep=False):
        if with_rep:
            return {}, self(obs)
        return {}

    def get_samples(self, obs) -> dict:
        return {}


class MultipleCNN(Base):
    def __init__(self, ocr_config, env_config) -> None:
        self._module = MultipleCNN_Module(ocr_config, env_config)
        super().__init__(ocr_config, env_config)
        learning = getattr(ocr_config, "learning", None)
        if learning is not None and hasattr(learning, "lr"):      # ocrs/base.py:20-25
            self._opt = torch.optim.Adam(self._module.parameters(), lr=learning.lr)

    def get_samples(self, obs) -> dict:
        return {}
