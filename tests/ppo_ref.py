"""CPU restatement of what ocrl_amd.sb3s.ppo and its two C entry points add (plain torch, fp64 unless a dtype is given): the sampling
rule of ``ocrl_acnet_act`` (include/ocrl_hip.h), the rollout buffer's flatten order, the L2 clip + Adam step of
``ocrl_flat_clip_adam_l2`` and one ``PPO.train()``.  The network, the loss and GAE are tests/acnet_ref.py's, the norm and the Adam
update tests/optim_ref.py's and the oracle's.  Needs neither the reference nor a GPU."""
from types import SimpleNamespace

import torch

from oracle import slate_oracle as O
from tests import acnet_ref as R
from tests.optim_ref import grad_norm

ADAM_EPS = 1e-5
gae = R.gae


SITE_ACNET_ACT = 400           # csrc/acnet.h


def uniforms(seed, row_offset, n):
    """host restatement of the uniforms ocrl_acnet_act draws (csrc/acnet.hip act_uniform): the top 24 bits of rng_bits1_keyed at the
    counter row_offset + i under the key of (seed, SITE_ACNET_ACT), times 2^-24; float32 [n] (counters below 2^32)"""
    import numpy as np
    from tests.gpu_util import _M32, _mix32k, rng_key
    assert row_offset + n <= 2 ** 32
    key = rng_key(seed, SITE_ACNET_ACT, 0)
    idx = np.arange(row_offset, row_offset + n, dtype=np.uint64)
    bits = _mix32k(idx ^ np.uint64(key), np.uint64((key * 0x9E3779B9 + 0x7F4A7C15) & _M32))
    return torch.from_numpy(((bits >> np.uint64(8)).astype(np.float64) / 2.0 ** 24).astype(np.float32))


def cdf(logits):
    """c [B, A] in fp64: c_a = p_0 + ... + p_a of softmax(logits), summed in index order"""
    return torch.cumsum(torch.softmax(logits.double(), dim=-1), dim=-1)


def sample(logits, u):
    """the sampling rule: action = the number of a in [0, A - 2] with c_a <= u (u [B] in [0, 1)); int64 [B]"""
    c = cdf(logits)
    return (c[:, :-1] <= u.double().reshape(-1, 1)).sum(-1)


def argmax_lowest(logits):
    """the deterministic action: the lowest index of the maximum"""
    lg = logits.double()
    A = lg.shape[1]
    idx = torch.arange(A).expand_as(lg)
    return torch.where(lg == lg.max(-1, keepdim=True).values, idx, torch.full_like(idx, A)).min(-1).values


def intervals(logits):
    """(midpoints, widths) [B, A] of the intervals of u that map to each action: [c_{a-1}, c_a), the last one reaching up to 1"""
    c = cdf(logits)
    lo = torch.cat([torch.zeros_like(c[:, :1]), c[:, :-1]], dim=1)
    hi = torch.cat([c[:, :-1], torch.ones_like(c[:, :1])], dim=1)
    return (lo + hi) / 2, hi - lo


def log_prob(logits, actions):
    return torch.log_softmax(logits.double(), dim=-1).gather(1, actions.long().reshape(-1, 1))[:, 0]


def flatten(t):
    """[T, E, ...] -> [E * T, ...] with row e * T + t (stable-baselines3's swap_and_flatten)"""
    T, E = t.shape[:2]
    out = torch.empty(E * T, *t.shape[2:], dtype=t.dtype)
    for e in range(E):
        for s in range(T):
            out[e * T + s] = t[s, e]
    return out


def clip_adam_l2(p, g, m, v, max_norm, lr, t, eps=ADAM_EPS):
    """one step on flat tensors, fp64: coef = min(1, max_norm / (||g||_2 + 1e-6)) (max_norm <= 0 or None: 1), then Adam with bias
    correction, t counted from 1.  Returns copies p, m, v and the norm."""
    p, m, v = (x.detach().double().clone() for x in (p, m, v))
    g = g.detach().double()
    norm = grad_norm([g], 2)
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0) if max_norm and max_norm > 0 else torch.ones((), dtype=torch.float64)
    O.adam_update(p, g * coef, m, v, t, float(lr), eps=eps)
    return SimpleNamespace(p=p, m=m, v=v, norm=norm, coef=coef)


def torch_clip_adam_l2(p, g, m, v, max_norm, lr, t, dtype=torch.float32, eps=ADAM_EPS):
    """the same step as torch runs it in `dtype`: clip_grad_norm_ + torch.optim.Adam(eps) with the planted state; returns p after it"""
    q = torch.nn.Parameter(p.detach().to(dtype).clone())
    q.grad = g.detach().to(dtype).clone()
    opt = torch.optim.Adam([q], lr=lr, eps=eps)
    opt.state[q] = dict(step=torch.tensor(float(t - 1)), exp_avg=m.detach().to(dtype).clone(), exp_avg_sq=v.detach().to(dtype).clone())
    if max_norm and max_norm > 0:
        torch.nn.utils.clip_grad_norm_([q], max_norm)
    opt.step()
    return q.detach()


def train(params, layout, buf, perms, hyper, dtype=torch.float64, torch_step=False):
    """one PPO.train(): params in the C ABI's order; buf: features [T, E, F], actions, values, log_probs, advantages, returns [T, E];
    perms: one permutation of T * E per epoch; hyper: batch_size, clip_range, vf_coef, ent_coef, normalize_advantage, max_grad_norm,
    learning_rate.  ``torch_step``: clip_grad_norm_ + torch.optim.Adam in `dtype` instead of the fp64 step above.
    Returns (parameters after the updates, the means of the six scalars, the number of updates)."""
    dims, acts = layout
    ps = [p.detach().to(dtype).clone().requires_grad_(True) for p in params]
    flat = {k: flatten(buf[k]) for k in ("features", "actions", "log_probs", "advantages", "returns")}
    opt = torch.optim.Adam(ps, lr=hyper["learning_rate"], eps=ADAM_EPS) if torch_step else None
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    sums, n = torch.zeros(6, dtype=torch.float64), 0
    for perm in perms:
        for start in range(0, perm.numel(), hyper["batch_size"]):
            idx = perm[start:start + hyper["batch_size"]]
            _, _, lg, vl = R.forward(flat["features"][idx].to(dtype), ps, dims, acts)
            s = R.ppo(lg, vl, flat["actions"][idx], flat["log_probs"][idx].to(dtype), flat["advantages"][idx].to(dtype), flat["returns"][idx].to(dtype),
                      hyper["clip_range"], hyper["vf_coef"], hyper["ent_coef"], hyper["normalize_advantage"])
            sums += torch.stack([s[k].detach().double() for k in R.SCALARS])
            n += 1
            gs = torch.autograd.grad(s["loss"], ps)
            if torch_step:
                for p, g in zip(ps, gs):
                    p.grad = g
                if hyper["max_grad_norm"]:
                    torch.nn.utils.clip_grad_norm_(ps, hyper["max_grad_norm"])
                opt.step()
            else:
                sizes = [p.numel() for p in ps]
                r = clip_adam_l2(torch.cat([p.detach().reshape(-1) for p in ps]), torch.cat([g.reshape(-1) for g in gs]),
                                 torch.cat([m.reshape(-1) for m in ms]), torch.cat([v.reshape(-1) for v in vs]), hyper["max_grad_norm"],
                                 hyper["learning_rate"], n)
                with torch.no_grad():
                    for p, q, m, mq, v, vq in zip(ps, r.p.split(sizes), ms, r.m.split(sizes), vs, r.v.split(sizes)):
                        p.copy_(q.view_as(p)); m.copy_(mq.view_as(m)); v.copy_(vq.view_as(v))
    return [p.detach() for p in ps], sums / max(n, 1), n
