"""RL entry point with the reference's command line (train_sb3.py:22-120, on this project's config resolver and its own PPO, A2C and
DQN; ``sb3=ppo``, ``sb3=a2c`` or ``sb3=dqn`` (and its extensions ``dqn_per``, ``dqn_c51``, ``rainbow``, ``qrdqn``, ``iqn``, and with Munchausen targets ``sb3=mdqn``, ``sb3=miqn``, and with proposed fractions ``sb3=fqf``) chooses, as the reference's ``getattr(sb3, config.sb3.name)``; DQN steps a frozen or
torch-trained encoder only and calls back every ``sb3.algo_kwargs.log_interval`` (default 100) iterations of ``train_freq`` steps):

    python train_sb3.py ocr=slate pooling=transformer sb3=ppo sb3_acnet=mlp env=target-N4C4S3S1 num_envs=16 device=cuda:0 \
        pooling.ocr_checkpoint.local_file=outputs/train_ocr/SLATE-RandomN5C4S4S2/checkpoints/model_best.pth

Builds the vectorised environment (ocrl_amd.envs: state, step and frames stay on the GPU), the OCRExtractor policy over the pre-trained
encoder and the algorithm with ``n_steps = max(1, sb3.algo_kwargs.n_steps // num_envs)``, then alternates rollouts and updates until
``max_steps``.  Whenever ``num_timesteps`` passes a multiple of ``eval.freq`` the policy plays ``eval.n_episodes`` episodes (sampled actions, as the reference's
EvalCallback with deterministic=False) on a separate environment seeded ``seed + num_envs``.  ``run_dir`` receives metrics.jsonl (one line
per iteration: the train() statistics, the rollout's episode window, and the evaluation when one ran) and checkpoints/model_latest.pth,
model_best.pth (PPO.save / A2C.save).  No video and no wandb.  ``ocr=slate`` / ``ocr=slotattn`` without a checkpoint train the encoder
end to end through the agent's loss, and with ``pooling.ocr_checkpoint.finetuning=True`` fine-tune a pre-trained one: PPO and A2C clip
and step the encoder's slice together with the policy.  An IODINE encoder needs its pre-trained checkpoint
(pooling.ocr_checkpoint.local_file, no finetuning); NatureCNN / MultipleCNN train from scratch.  ``ocr=gt`` is the ground-truth-state
baseline: the environments hand out their state rows (render_mode: state) and no frame is rendered.
"""
import json
import logging
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from ocrl_amd import envs, sb3s  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402

log = logging.getLogger("train_sb3")
ALGOS = {"PPO": sb3s.PPO, "A2C": sb3s.A2C, "DQN": sb3s.DQN}
POLICIES = {"DQN": sb3s.DQNPolicy}          # every other algorithm takes the actor-critic policy
EVAL_ROW_OFFSET = 1 << 40          # the evaluation samples from its own rows of the policy's stream: training draws do not move


def build(config):
    """(env, eval_env, model) of a composed train_sb3 config"""
    if config.sb3.name not in ALGOS:
        raise NotImplementedError(f"train_sb3: sb3: {config.sb3.name} is not built (built: {', '.join(ALGOS)})")
    if config.ocr.name == "GT":
        config.env.render_mode = "state"          # train_sb3.py:41-42, 72-73: the GT encoder reads the state rows, not frames
    env = envs.make_env(config)
    eval_env = envs.make_env(config, num_envs=min(config.num_envs, config.eval.n_episodes), seed=config.seed + config.num_envs)
    kwargs = dict(device=config.device, seed=config.seed,
                  policy_kwargs=dict(config=config, features_extractor_class=sb3s.OCRExtractor, features_extractor_kwargs=dict(config=config)))
    if hasattr(config.sb3, "algo_kwargs"):
        kwargs.update(config.sb3.algo_kwargs.to_dict())
    if "n_steps" in kwargs and issubclass(ALGOS[config.sb3.name], sb3s.on_policy.OnPolicyAlgorithm):
        kwargs["n_steps"] = max(1, kwargs["n_steps"] // config.num_envs)
    return env, eval_env, ALGOS[config.sb3.name](POLICIES.get(config.sb3.name, sb3s.CustomActorCriticPolicy), env, **kwargs)


def evaluate(model, env, n_episodes, calls):
    """the first ``n_episodes`` episodes, in (step, environment) order, that end on ``env`` under sampled actions ->
    (success rate, mean return, mean length).  The device is read every 16 steps."""
    E = env.num_envs
    obs = env.reset()
    done_rows, episodes = [], []
    model.policy.eval()
    rows = EVAL_ROW_OFFSET + calls * (1 << 24)
    limit = 16 * (2 + n_episodes * int(env.config.max_steps) // E)
    with torch.no_grad():
        for t in range(limit):
            actions, _, _ = model.policy.act(model.policy.extract_features(model._obs(obs)), row_offset=rows + t * E)
            obs, _, dones, ex = env.step_device(actions)
            done_rows.append(torch.stack([dones.double(), ex["is_success"].double(), ex["episode_return"], ex["episode_length"].double()]))
            if (t + 1) % 16 == 0:
                host = torch.stack(done_rows).cpu().numpy()
                episodes = [(host[i, 1, e], host[i, 2, e], host[i, 3, e]) for i in range(host.shape[0]) for e in range(E) if host[i, 0, e]]
                if len(episodes) >= n_episodes:
                    break
    episodes = episodes[:n_episodes]
    if not episodes:
        return float("nan"), float("nan"), float("nan")
    return tuple(sum(ep[k] for ep in episodes) / len(episodes) for k in range(3))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    config = compose(os.path.join(ROOT, "configs"), "train_sb3", argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    ckpt_dir = os.path.join(config.run_dir, "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    logf = open(os.path.join(config.run_dir, "metrics.jsonl"), "a")
    env, eval_env, model = build(config)
    log.info(f"{config.ocr.name}-{config.pooling.name}-{config.sb3.name} on {config.env.name} ({config.env.mode} mode, {config.env.rew_type} reward): "
             f"{config.num_envs} environments, n_steps {model.n_steps}, batch {model.batch_size}")
    state = dict(next_eval=int(config.eval.freq), best=-math.inf, evals=0)

    def finite(v):
        return float(v) if isinstance(v, (int, float)) and math.isfinite(v) else None

    def after_iteration(loc):
        row = {"step": loc["num_timesteps"], "iteration": loc["iteration"]}
        row.update({f"train/{k}": finite(v) for k, v in loc["train"].items()})
        row.update({"rollout/ep_rew_mean": finite(loc["ep_rew_mean"]), "rollout/ep_len_mean": finite(loc["ep_len_mean"]),
                    "rollout/success_rate": finite(model.success_rate)})
        if loc["num_timesteps"] >= state["next_eval"]:
            while state["next_eval"] <= loc["num_timesteps"]:
                state["next_eval"] += int(config.eval.freq)
            success, ret, length = evaluate(model, eval_env, int(config.eval.n_episodes), state["evals"])
            state["evals"] += 1
            row.update({"eval/success_rate": finite(success), "eval/mean_reward": finite(ret), "eval/mean_ep_length": finite(length)})
            model.save(os.path.join(ckpt_dir, "model_latest.pth"))
            if math.isfinite(ret) and ret > state["best"]:
                state["best"] = ret
                model.save(os.path.join(ckpt_dir, "model_best.pth"))
            log.info(f"[step {loc['num_timesteps']}] eval success {success:.3f} / return {ret:.3f} / length {length:.1f}")
        logf.write(json.dumps(row) + "\n")
        logf.flush()
        log.info(f"step {loc['num_timesteps']} ep_rew_mean {loc['ep_rew_mean']:.3f} success {model.success_rate:.3f} loss {loc['train']['loss']:.4f}")

    model.learn(int(config.max_steps), callback=after_iteration)
    model.save(os.path.join(ckpt_dir, "model_latest.pth"))
    if not os.path.exists(os.path.join(ckpt_dir, "model_best.pth")):
        model.save(os.path.join(ckpt_dir, "model_best.pth"))
    logf.close()
    return model


if __name__ == "__main__":
    main()
