"""Drop-in for the reference's ``ocrs`` package on the SLATE / Slot-Attention / IODINE paths:
``getattr(ocrs, config.ocr.name)(config.ocr, config.dataset)`` (train_ocr.py:37) and
``getattr(ocrs, name + "_Module")`` (utils/tools.py:327-331) resolve here; so do the NatureCNN and MultipleCNN encoders of the RL
baselines, the VAE, the masked autoencoder (MAE) and the ground-truth-state baseline (GT)."""
from .base import Base
from .gt import GT, GT_Module
from .iodine import Iodine, Iodine_Module
from .multiple_cnn import MultipleCNN, MultipleCNN_Module
from .naturecnn import NatureCNN, NatureCNN_Module
from .slate import SLATE, SLATE_Module
from .vae import VAE, VAE_Module
from .mae import MAE, MAE_Module

__all__ = ["Base", "SLATE", "SLATE_Module", "Iodine", "Iodine_Module", "NatureCNN", "NatureCNN_Module", "MultipleCNN", "MultipleCNN_Module", "VAE", "VAE_Module", "MAE", "MAE_Module", "GT", "GT_Module"]
