"""A2C's update on the shared on-policy loop (on_policy.py: rollout buffer, rollout collection, the flat buffers, ``learn``): what the
reference selects with ``sb3=a2c`` (configs/sb3/a2c.yaml).

``A2C`` restates stable-baselines3 1.5's ``A2C`` from the published algorithm (the footing of ``a2c_loss``): none of its text is copied.
One update is the whole rollout in one batch: ``a2c_loss`` (``ocrl_acnet_a2c_fwd_bwd``: one fused forward + backward), one backward
through the extractor and ``ocrl_flat_clip_rmsprop_l2``, the L2 clip and stable-baselines3's ``RMSpropTFLike`` step (alpha 0.99, epsilon
inside the root, the square average started at ones) on one flat parameter buffer; ``use_rms_prop=False`` takes the Adam step PPO takes."""
import torch

from .. import _lib
from .custom_acnets import A2C_SCALARS, a2c_loss
from .on_policy import OnPolicyAlgorithm

RMSPROP_ALPHA = 0.99            # stable-baselines3's A2C builds RMSpropTFLike(alpha=0.99, eps=rms_prop_eps, weight_decay=0)


class A2C(OnPolicyAlgorithm):
    """Advantage actor-critic (synchronous A3C) for Discrete actions (stable-baselines3's A2C on a VecEnv); ``env`` and ``policy`` as
    OnPolicyAlgorithm takes them.  ``batch_size`` is the rollout's T * E rows."""
    ALGO = "A2C"
    HYPER = ("learning_rate", "n_steps", "gamma", "gae_lambda", "ent_coef", "vf_coef", "max_grad_norm", "rms_prop_eps", "use_rms_prop",
             "normalize_advantage")

    def __init__(self, policy, env, learning_rate=7e-4, n_steps=5, gamma=0.99, gae_lambda=1.0, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 rms_prop_eps=1e-5, use_rms_prop=True, normalize_advantage=False, seed=0, device="cuda", policy_kwargs=None, verbose=0,
                 tensorboard_log=None, **ignored_sb3_kwargs):
        self.rms_prop_eps, self.use_rms_prop = float(rms_prop_eps), bool(use_rms_prop)
        super().__init__(policy, env, learning_rate, n_steps, gamma, gae_lambda, ent_coef, vf_coef, max_grad_norm, normalize_advantage, seed, device,
                         policy_kwargs)

    @property
    def batch_size(self):
        return self.n_steps * self.n_envs

    # ---- the optimiser: the square average beside flat_p, started at ones (square_avg, rmsprop_step), or Adam's moments
    def _init_optimizer(self):
        if not self.use_rms_prop:
            return self._init_adam()
        self.square_avg = torch.ones_like(self.flat_p)
        self.enc_sq = self._new_encoder_state(1.0)               # a trainable encoder's range: its own square average, at ones too
        self.rmsprop_step = 0
        L = _lib.lib()
        self._ws = torch.empty(L.ocrl_flat_clip_rmsprop_ws_floats() if self._encoder is None else L.ocrl_flat_clip_multi_ws_floats(), device=self.device)

    def _optimizer_step(self):
        """L2 clip of the whole gradient to max_grad_norm, then the TF-style RMSprop step: one C call, no host synchronisation.  With a
        trainable encoder the norm is the joint one and the one call steps the policy's and the encoder's segments."""
        if not self.use_rms_prop:
            return self._adam_step()
        self.rmsprop_step += 1
        with torch.cuda.device(self.device):
            if self._encoder is not None:
                seg = self._segments(self.square_avg, None, self.enc_sq, None)
                _lib.check(_lib.lib().ocrl_flat_clip_rmsprop_l2_multi(seg, len(seg), self.max_grad_norm, self.learning_rate, RMSPROP_ALPHA,
                                                                      self.rms_prop_eps, _lib.ptr(self._norm), _lib.ptr(self._ws), self._ws.numel(),
                                                                      _lib.stream(self.device)))
                return
            _lib.check(_lib.lib().ocrl_flat_clip_rmsprop_l2(_lib.ptr(self.flat_p), _lib.ptr(self.flat_g), _lib.ptr(self.square_avg),
                                                            self.flat_p.numel(), self.max_grad_norm, self.learning_rate, RMSPROP_ALPHA,
                                                            self.rms_prop_eps, _lib.ptr(self._norm), _lib.ptr(self._ws), self._ws.numel(),
                                                            _lib.stream(self.device)))

    def _optimizer_state(self):
        if not self.use_rms_prop:
            return self._adam_state()
        out = {"square_avg": self.square_avg, "step": self.rmsprop_step}
        if self._encoder is not None:
            out["enc_sq"] = self.enc_sq
        return out

    def _load_optimizer_state(self, opt):
        if not self.use_rms_prop:
            return self._load_adam_state(opt)
        if "square_avg" not in opt or opt["square_avg"].shape != self.square_avg.shape:
            n = opt["square_avg"].numel() if "square_avg" in opt else "no"
            raise ValueError(f"{self._who}.load: the checkpoint's optimiser state has {n} RMSprop entries, this policy's {self.square_avg.numel()} "
                             "(use_rms_prop and the policy layout must be those of the run that saved it)")
        self._check_encoder_state(opt, ("enc_sq",))
        self.square_avg.copy_(opt["square_avg"])
        if self._encoder is not None:
            self.enc_sq.copy_(opt["enc_sq"])
        self.rmsprop_step = int(opt["step"])

    # ---- the update
    def train(self):
        """one update on the whole rollout buffer, its T * E rows in flattened order as one batch (no permutation is drawn: the generator
        stays where it is).  Returns A2C_SCALARS, ``explained_variance``, ``grad_norm`` and ``n_updates`` (1).  The device is read once."""
        mb = self.rollout_buffer.flat()
        self.policy.train()
        self.flat_g.zero_()
        features = self.policy.extract_features(self._obs(mb.observations))
        loss, m = a2c_loss(self.policy, features, mb.actions, mb.advantages, mb.returns, self.vf_coef, self.ent_coef, self.normalize_advantage)
        loss.backward()
        self._optimizer_step()
        host = torch.cat([torch.stack([m[k] for k in A2C_SCALARS]), self._norm, self._explained_variance().reshape(1)]).tolist()   # the one read
        out = dict(zip(A2C_SCALARS, host))
        out.update(explained_variance=host[5], grad_norm=host[4], n_updates=1)
        return out


__all__ = ["A2C"]
