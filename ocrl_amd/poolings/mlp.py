"""MLP pooling (poolings/mlp/mlp.py:6-9, mlp_module.py:7-23): the flattened slots through Linear layers, each followed by a ReLU when
its act is "relu" (zip(dims, acts): the shorter list wins).  The Linears run on the library's GEMM (``_HipLinear``) with the ReLU
fused; an ``nn.Identity`` keeps each ReLU's index so that the ``_mlp.{i}`` state_dict keys are the reference's."""
from torch import nn

from .base import Base
from .transformer import _HipLinear


class MLP_Module(nn.Module):
    def __init__(self, ocr_rep_dim: int, ocr_num_slots: int, config, num_stacked_obss: int = 1) -> None:
        super().__init__()
        self.rep_dim = config.dims[-1]
        in_dim = ocr_rep_dim * ocr_num_slots * num_stacked_obss
        net = []
        for dim, act in zip(config.dims, config.acts):
            net.append(_HipLinear(in_dim, dim, relu=act == "relu"))
            if act == "relu":
                net.append(nn.Identity())
            in_dim = dim
        self._mlp = nn.Sequential(*net)

    def forward(self, state):
        state = state.flatten(start_dim=1) if len(state.shape) == 3 else state
        return self._mlp(state)


class MLP(Base):
    def __init__(self, ocr, config, num_stacked_obss: int = 1) -> None:
        self._module = MLP_Module(ocr.rep_dim, ocr.num_slots, config, num_stacked_obss)
        super().__init__(ocr, config)
