from .custom_acnets import CustomActorCriticPolicy, CustomNetwork, compute_gae, ppo_loss
from .ocr_extractor import OCRExtractor
from .ppo import PPO, RolloutBuffer

__all__ = ["OCRExtractor", "CustomNetwork", "CustomActorCriticPolicy", "ppo_loss", "compute_gae", "PPO", "RolloutBuffer"]
