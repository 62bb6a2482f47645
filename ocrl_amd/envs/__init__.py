"""Environments of the RL side (the reference's ``envs`` package): built here are the Target and Odd-One-Out sprite tasks, vectorised on the GPU."""
from .sprite import COLORS, SHAPES, OddOneOutEnv, SpriteEnv, TargetEnv, env_desc, sprite_env_uniforms

_ENVS = {"TargetEnv": TargetEnv, "OddOneOutEnv": OddOneOutEnv}


def make_env(config, num_envs=None, seed=None, device=None):
    """the vectorised environment ``config.env.env`` names, as train_sb3.py builds it: ``num_envs`` (default config.num_envs)
    environments on streams of ``seed`` (default config.seed) on ``device`` (default config.device)"""
    name = config.env.env
    if name not in _ENVS:
        raise NotImplementedError(f"ocrl_amd.envs: env: {name} is not built (built: {', '.join(_ENVS)})")
    return _ENVS[name](config.env, config.num_envs if num_envs is None else num_envs, config.seed if seed is None else seed,
                       config.device if device is None else device)


__all__ = ["TargetEnv", "OddOneOutEnv", "SpriteEnv", "make_env", "env_desc", "sprite_env_uniforms", "COLORS", "SHAPES"]
