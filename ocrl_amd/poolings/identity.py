"""Identity pooling (poolings/identity/identity.py:6-9, identity_module.py:7-12): the slots flattened to one vector.  No parameters,
any device."""
from torch import nn

from .base import Base


class Identity_Module(nn.Module):
    def __init__(self, ocr_rep_dim: int, ocr_num_slots: int, config, num_stacked_obss: int = 1) -> None:
        super().__init__()
        self.rep_dim = ocr_rep_dim * ocr_num_slots * num_stacked_obss

    def forward(self, state):
        return state.flatten(start_dim=1) if len(state.shape) == 3 else state


class Identity(Base):
    def __init__(self, ocr, config, num_stacked_obss: int = 1) -> None:
        self._module = Identity_Module(ocr.rep_dim, ocr.num_slots, config, num_stacked_obss)
        super().__init__(ocr, config)
