from .a2c import A2C
from .c51 import CategoricalQNetwork, c51_loss
from .custom_acnets import CustomActorCriticPolicy, CustomNetwork, a2c_loss, compute_gae, ppo_loss
from .dqn import DQN, DQNPolicy, QNetwork, dqn_loss
from .fqf import FullyParameterizedQuantileQNetwork, fqf_fraction_loss
from .iqn import ImplicitQuantileQNetwork, iqn_loss
from .munchausen import munchausen_targets
from .noisy import NoisyLinear
from .ocr_extractor import OCRExtractor
from .ppo import PPO, RolloutBuffer
from .qr import QuantileQNetwork, qr_loss
from .replay import ReplayBuffer

__all__ = ["OCRExtractor", "CustomNetwork", "CustomActorCriticPolicy", "ppo_loss", "a2c_loss", "compute_gae", "PPO", "A2C", "RolloutBuffer",
           "DQN", "DQNPolicy", "QNetwork", "dqn_loss", "ReplayBuffer", "CategoricalQNetwork", "c51_loss", "NoisyLinear", "QuantileQNetwork", "qr_loss",
           "ImplicitQuantileQNetwork", "iqn_loss", "munchausen_targets", "FullyParameterizedQuantileQNetwork",
           "fqf_fraction_loss"]
