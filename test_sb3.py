"""Evaluates a trained agent on another environment (what the reference's configs/test_sb3.yaml is for; its script is not shipped), e.g.
an agent trained on the unseen-combination training side against the test side:

    python test_sb3.py ocr=slate pooling=transformer sb3=ppo sb3_acnet=mlp env=odd-one-out-N4C3S1S1-ood-unseen-combi-test1 \
        pooling.ocr_checkpoint.local_file=outputs/train_ocr/SLATE-RandomN5C4S4S2/checkpoints/model_best.pth \
        agent_checkpoint.local_file=outputs/train_sb3/SLATE-Transformer-PPO-OddOneOutN4C3S1S1Env/checkpoints/model_best.pth

Composes configs/test_sb3.yaml, builds the environment and the model as train_sb3.py does (the choices must be those the agent was
trained with: PPO.load checks the policy layout), loads the agent (a PPO.save file) and plays ``n_eval_episodes`` episodes under sampled
actions with train_sb3.evaluate, on the environment train_sb3.py evaluates on (seeded ``seed + num_envs``).  ``run_dir``/eval.jsonl
receives one JSON line: env, episodes, success_rate, mean_reward, mean_ep_length.  No video and no wandb."""
import json
import logging
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import train_sb3  # noqa: E402
from ocrl_amd.utils.config import compose  # noqa: E402

log = logging.getLogger("test_sb3")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    config = compose(os.path.join(ROOT, "configs"), "test_sb3", argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    path = config.agent_checkpoint.local_file
    if not path:
        raise ValueError("test_sb3: agent_checkpoint.local_file is empty: give the agent's checkpoint (train_sb3.py's checkpoints/model_best.pth)")
    if not os.path.exists(path):
        raise FileNotFoundError(f"test_sb3: agent_checkpoint.local_file: {path} does not exist")
    episodes = int(config.n_eval_episodes)
    if episodes < 1:
        raise ValueError(f"test_sb3: n_eval_episodes >= 1 (got {episodes})")
    config.eval = {"freq": 0, "n_episodes": episodes}          # what train_sb3.build sizes the evaluation environment by
    _, env, model = train_sb3.build(config)
    model.load(path)
    success, ret, length = train_sb3.evaluate(model, env, episodes, 0)
    row = {"env": config.env.name, "episodes": episodes, "success_rate": success, "mean_reward": ret, "mean_ep_length": length}
    os.makedirs(config.run_dir, exist_ok=True)
    with open(os.path.join(config.run_dir, "eval.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")
    log.info(f"{config.env.name}: {episodes} episodes, success {success:.3f} / return {ret:.3f} / length {length:.1f}")
    return row


if __name__ == "__main__":
    main()
