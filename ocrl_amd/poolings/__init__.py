"""Drop-in for the reference's ``poolings`` package: ``getattr(poolings, config.pooling.name)(ocr, config.pooling)``
and ``getattr(poolings, name + "_Module")`` (sb3s/ocr_extractor.py:20-35).  All six heads are
built: Transformer, RN, MLP, Identity and the NatureCNN heads CNN_Linear and CNN_Transformer (over ``slot_to_img`` of a CNN feature map)."""
from .base import Base
from .cnn_linear import CNN_Linear, CNN_Linear_Module
from .cnn_transformer import CNN_Transformer, CNN_Transformer_Module
from .identity import Identity, Identity_Module
from .mlp import MLP, MLP_Module
from .rn import RN, RN_Module
from .transformer import Transformer, Transformer_Module

__all__ = ["Base", "Transformer", "Transformer_Module", "RN", "RN_Module", "MLP", "MLP_Module", "Identity", "Identity_Module",
           "CNN_Linear", "CNN_Linear_Module", "CNN_Transformer", "CNN_Transformer_Module"]
