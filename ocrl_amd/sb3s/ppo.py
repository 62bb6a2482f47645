"""PPO's update on the shared on-policy loop (on_policy.py: rollout buffer, rollout collection, the flat buffers, ``learn``).

``PPO`` restates stable-baselines3 1.5's ``PPO`` from the published algorithm (the footing of ``ppo_loss``): none of its text is copied.
A minibatch is ``ppo_loss`` (one fused forward + backward) and the update ``ocrl_flat_clip_adam_l2`` on one flat parameter buffer; with a
trainable SLATE encoder behind the extractor ``ocrl_flat_clip_adam_l2_multi`` on that buffer and the encoder's range of its engine's, under
one joint norm (on_policy.py).  Where this departs from stable-baselines3 is listed in DESIGN.md §7."""
import torch

from .custom_acnets import PPO_SCALARS, CustomActorCriticPolicy, ppo_loss
from .on_policy import ADAM_EPS, OnPolicyAlgorithm, RolloutBatch, RolloutBuffer, _check_constant  # noqa: F401


class PPO(OnPolicyAlgorithm):
    """Proximal policy optimisation, clipped surrogate, for Discrete actions (stable-baselines3's PPO on a VecEnv); ``env`` and ``policy``
    as OnPolicyAlgorithm takes them."""
    ALGO = "PPO"
    HYPER = ("learning_rate", "n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "clip_range", "ent_coef", "vf_coef", "max_grad_norm",
             "target_kl", "normalize_advantage")

    def __init__(self, policy, env, learning_rate=3e-4, n_steps=2048, batch_size=64, n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, target_kl=None, normalize_advantage=True, seed=0, device="cuda", policy_kwargs=None,
                 clip_range_vf=None, verbose=0, tensorboard_log=None, **ignored_sb3_kwargs):
        who = f"ocrl_amd.sb3s.{self.ALGO}"
        if clip_range_vf is not None:
            raise NotImplementedError(f"{who}: clip_range_vf is not built (ppo_loss is PPO's loss with clip_range_vf = None)")
        _check_constant(who, "learning_rate", learning_rate)
        self.clip_range = _check_constant(who, "clip_range", clip_range)
        self.batch_size, self.n_epochs = int(batch_size), int(n_epochs)
        self.target_kl = None if target_kl is None else float(target_kl)
        super().__init__(policy, env, learning_rate, n_steps, gamma, gae_lambda, ent_coef, vf_coef, max_grad_norm, normalize_advantage, seed, device,
                         policy_kwargs)

    # ---- the optimiser: Adam's two moments beside flat_p (flat_m, flat_v, adam_step)
    def _init_optimizer(self):
        self._init_adam()

    def _optimizer_step(self):
        self._adam_step()

    def _optimizer_state(self):
        return self._adam_state()

    def _load_optimizer_state(self, opt):
        self._load_adam_state(opt)

    # ---- the update
    def train(self, perms=None):
        """n_epochs passes over the rollout buffer in minibatches (``perms``: one permutation of T * E per epoch instead of drawn ones).
        Returns the means of PPO_SCALARS over the minibatches, ``explained_variance``, ``grad_norm`` (mean over the updates) and
        ``n_updates`` (optimiser steps taken).  The device is read once, at the end; with ``target_kl`` once per minibatch."""
        buf = self.rollout_buffer
        self.policy.train()
        acc = torch.zeros(len(PPO_SCALARS) + 1, device=self.device)      # sums of the six scalars and of the gradient norm
        n_batches = n_updates = 0
        stop = False
        for epoch in range(self.n_epochs):
            for mb in buf.get(self.batch_size, None if perms is None else perms[epoch], self.generator):
                self.flat_g.zero_()
                features = self.policy.extract_features(self._obs(mb.observations))
                loss, m = ppo_loss(self.policy, features, mb.actions, mb.old_log_prob, mb.advantages, mb.returns, self.clip_range, self.vf_coef,
                                   self.ent_coef, self.normalize_advantage)
                acc[:6] += torch.stack([m[k] for k in PPO_SCALARS])
                n_batches += 1
                if self.target_kl is not None and m["approx_kl"].item() > 1.5 * self.target_kl:
                    stop = True                                      # as stable-baselines3: this minibatch takes no step
                    break
                loss.backward()
                self._optimizer_step()
                acc[6] += self._norm[0]
                n_updates += 1
            if stop:
                break
        host = torch.cat([acc, self._explained_variance().reshape(1)]).tolist()   # the one read
        out = {k: host[i] / max(n_batches, 1) for i, k in enumerate(PPO_SCALARS)}
        out.update(explained_variance=host[7], n_updates=n_updates, grad_norm=host[6] / max(n_updates, 1))
        return out


__all__ = ["PPO", "RolloutBuffer", "RolloutBatch", "CustomActorCriticPolicy"]
