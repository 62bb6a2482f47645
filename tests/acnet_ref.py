"""CPU restatement of the actor-critic head, the PPO minibatch loss and GAE (plain torch, any dtype): what the tests hold
``ocrl_acnet_*`` and ``ocrl_gae`` to.  The trunks are sb3s/custom_acnets.py:8-96; the heads (action_net, value_net, a categorical
distribution) and the loss restate stable-baselines3's ActorCriticPolicy and PPO.train (clip_range_vf = None) from the published
algorithm.  Needs neither the reference nor a GPU."""
import torch

ACT = {0: lambda t: t, 1: torch.relu, 2: torch.tanh, "relu": torch.relu, "tanh": torch.tanh, "none": lambda t: t}
SCALARS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")


def n_params(dims, heads=True):
    return 2 * sum(len(d) for d in dims) + (4 if heads else 0)


def param_shapes(F, A, dims):
    """shapes in the C ABI's order: shared, policy, value trunks as (weight, bias), then action_net and value_net"""
    h = dims[0][-1] if dims[0] else F
    shapes = []
    for t in range(3):
        k = F if t == 0 else h
        for n in dims[t]:
            shapes += [(n, k), (n,)]
            k = n
    if A > 0:
        lp = dims[1][-1] if dims[1] else h
        lv = dims[2][-1] if dims[2] else h
        shapes += [(A, lp), (A,), (1, lv), (1,)]
    return shapes


def trunk(x, ws, acts):
    for l, a in enumerate(acts):
        x = ACT[a](x @ ws[2 * l].t() + ws[2 * l + 1])
    return x


def forward(x, w, dims, acts, heads=True):
    """latent_pi, latent_vf, logits, values (the last two None without heads); w in the C ABI's order"""
    q = [0, 2 * len(dims[0]), 2 * (len(dims[0]) + len(dims[1])), 2 * (len(dims[0]) + len(dims[1]) + len(dims[2]))]
    h = trunk(x, w[q[0]:q[1]], acts[0])
    lp = trunk(h, w[q[1]:q[2]], acts[1])
    lv = trunk(h, w[q[2]:q[3]], acts[2])
    if not heads:
        return lp, lv, None, None
    wa, ba, wv, bv = w[q[3]:q[3] + 4]
    return lp, lv, lp @ wa.t() + ba, (lv @ wv.t() + bv)[:, 0]


def ppo(logits, values, actions, old_log_prob, advantages, returns, clip_range, vf_coef, ent_coef, normalize_advantage=True):
    """dict of the six scalars"""
    logsm = torch.log_softmax(logits, dim=-1)
    logp = logsm.gather(1, actions.long().reshape(-1, 1))[:, 0]
    entropy = -(logsm.exp() * logsm).sum(-1)
    adv = advantages
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(logp - old_log_prob)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    value_loss = ((returns - values) ** 2).mean()
    entropy_loss = -entropy.mean()
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        lr = logp - old_log_prob
        approx_kl = ((ratio - 1) - lr).mean()
        clip_fraction = ((ratio - 1).abs() > clip_range).to(logits.dtype).mean()
    return dict(loss=loss, policy_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss, approx_kl=approx_kl, clip_fraction=clip_fraction)


def gae(rewards, values, episode_starts, last_values, dones, gamma, lam):
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    a = torch.zeros_like(last_values)
    for t in reversed(range(T)):
        if t == T - 1:
            nt, nv = 1.0 - dones, last_values
        else:
            nt, nv = 1.0 - episode_starts[t + 1], values[t + 1]
        delta = rewards[t] + gamma * nv * nt - values[t]
        a = delta + gamma * lam * nt * a
        adv[t] = a
    return adv, adv + values
