"""CPU restatement of what A2C adds (plain torch in a chosen dtype: fp64 is the reference, fp32 measures rounding): the loss of
``ocrl_acnet_a2c_fwd_bwd`` with its closed-form cotangents, the L2 clip + TF-style RMSprop step of ``ocrl_flat_clip_rmsprop_l2``
(stable-baselines3's RMSpropTFLike with momentum 0, not centred, no weight decay, restated from its published update rule) and one
``A2C.train()``.  The network is tests/acnet_ref.py's, the flatten order and the Adam step tests/ppo_ref.py's.  Needs neither the reference
nor a GPU."""
from types import SimpleNamespace

import torch

from tests import acnet_ref as R
from tests import ppo_ref as P

SCALARS = ("loss", "policy_loss", "value_loss", "entropy_loss")
ALPHA = 0.99


def normalized(adv):
    return (adv - adv.mean()) / (adv.std() + 1e-8)


def a2c(logits, values, actions, advantages, returns, vf_coef, ent_coef, normalize_advantage=False):
    """dict of the four scalars (actions are clamped into [0, A), as the kernel clamps them)"""
    logsm = torch.log_softmax(logits, dim=-1)
    act = actions.long().clamp(0, logits.shape[1] - 1)
    logp = logsm.gather(1, act.reshape(-1, 1))[:, 0]
    entropy = -(logsm.exp() * logsm).sum(-1)
    adv = normalized(advantages) if normalize_advantage else advantages
    policy_loss = -(adv * logp).mean()
    value_loss = ((values - returns) ** 2).mean()
    entropy_loss = -entropy.mean()
    return dict(loss=policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, policy_loss=policy_loss, value_loss=value_loss,
                entropy_loss=entropy_loss)


def cotangents(logits, values, actions, advantages, returns, vf_coef, ent_coef, normalize_advantage=False):
    """dL/dlogits [B, A] and dL/dvalues [B] in closed form:
    dL/dz_a = (1/B)(-adv ([a == act] - q_a) + ent_coef q_a ((z_a - lse) + H)),  dL/dv = (1/B) vf_coef 2 (v - ret)"""
    B, A = logits.shape
    lq = torch.log_softmax(logits, dim=-1)
    q = lq.exp()
    H = -(q * lq).sum(-1, keepdim=True)
    adv = (normalized(advantages) if normalize_advantage else advantages).reshape(B, 1)
    onehot = torch.zeros_like(q).scatter_(1, actions.long().clamp(0, A - 1).reshape(B, 1), 1.0)
    return (-adv * (onehot - q) + ent_coef * q * (lq + H)) / B, vf_coef * 2 * (values - returns) / B


def a2c_loss(x, params, layout, actions, advantages, returns, vf_coef, ent_coef, normalize_advantage=False, dtype=torch.float64):
    """(scalars [4], dfeatures, [dw]) of the loss through tests/acnet_ref.forward and autograd, in `dtype`"""
    xs = x.detach().to(dtype).requires_grad_(True)
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    _, _, lg, vl = R.forward(xs, ps, *layout)
    s = a2c(lg, vl, actions, advantages.to(dtype), returns.to(dtype), vf_coef, ent_coef, normalize_advantage)
    g = torch.autograd.grad(s["loss"], [xs] + ps)
    return torch.stack([s[k].detach() for k in SCALARS]), g[0], list(g[1:])


def rmsprop_tf_l2(p, g, sq, max_norm, lr, alpha=ALPHA, eps=1e-5, dtype=torch.float64):
    """one step on flat tensors in `dtype`: coef = min(1, max_norm / (||g||_2 + 1e-6)) (max_norm <= 0 or None: 1), g' = coef g,
    sq <- alpha sq + (1 - alpha) g'^2, p <- p - lr g' / sqrt(sq + eps): the epsilon inside the root, sq started at ones by the caller.
    Returns copies p, sq and the norm."""
    p, g, sq = (t.detach().to(dtype).clone() for t in (p, g, sq))
    norm = g.pow(2).sum().sqrt()
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm and max_norm > 0 else torch.ones((), dtype=dtype)
    g = g * coef
    sq = sq * alpha + (1 - alpha) * g * g
    p = p - lr * (g / (sq + eps).sqrt())
    return SimpleNamespace(p=p, sq=sq, norm=norm, coef=coef)


def adam_l2(p, g, m, v, max_norm, lr, t, dtype=torch.float64):
    """the clip + Adam step (eps 1e-5) of use_rms_prop=False in `dtype`, written out as tests/ppo_ref.clip_adam_l2 computes it"""
    p, g, m, v = (x.detach().to(dtype).clone() for x in (p, g, m, v))
    norm = g.pow(2).sum().sqrt()
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm and max_norm > 0 else torch.ones((), dtype=dtype)
    g = g * coef
    m = m + (g - m) * (1 - 0.9)
    v = v * 0.999 + (1 - 0.999) * g * g
    bc1, bc2 = 1 - 0.9 ** t, 1 - 0.999 ** t
    p = p - (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + P.ADAM_EPS))
    return SimpleNamespace(p=p, m=m, v=v, norm=norm, coef=coef)


def train(params, layout, buf, hyper, dtype=torch.float64, state=None):
    """one A2C.train(): params in the C ABI's order; buf: features [T, E, F], actions, advantages, returns [T, E], taken as one batch in
    flattened order; hyper: vf_coef, ent_coef, normalize_advantage, max_grad_norm, learning_rate, rms_prop_eps, use_rms_prop.  ``state``
    is the optimiser's (None: a fresh one, square average at ones) and is returned for the next update.
    Returns (parameters after the update, the four scalars in fp64, the state)."""
    ps = [p.detach().to(dtype) for p in params]
    sizes = [p.numel() for p in ps]
    n = sum(sizes)
    flat = {k: P.flatten(buf[k]) for k in ("features", "actions", "advantages", "returns")}
    scal, _, gs = a2c_loss(flat["features"], ps, layout, flat["actions"], flat["advantages"], flat["returns"], hyper["vf_coef"], hyper["ent_coef"],
                           hyper["normalize_advantage"], dtype)
    fp, fg = torch.cat([p.reshape(-1) for p in ps]), torch.cat([g.reshape(-1) for g in gs])
    if hyper.get("use_rms_prop", True):
        state = state or dict(sq=torch.ones(n, dtype=dtype), step=0)
        r = rmsprop_tf_l2(fp, fg, state["sq"], hyper["max_grad_norm"], hyper["learning_rate"], ALPHA, hyper.get("rms_prop_eps", 1e-5), dtype)
        state = dict(sq=r.sq, step=state["step"] + 1, norm=r.norm)
    else:
        state = state or dict(m=torch.zeros(n, dtype=dtype), v=torch.zeros(n, dtype=dtype), step=0)
        r = adam_l2(fp, fg, state["m"], state["v"], hyper["max_grad_norm"], hyper["learning_rate"], state["step"] + 1, dtype)
        state = dict(m=r.m, v=r.v, step=state["step"] + 1, norm=r.norm)
    return [q.view_as(p) for q, p in zip(r.p.split(sizes), ps)], scal.double(), state
