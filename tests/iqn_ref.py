"""fp64 torch restatement of DQN's implicit quantile head, from the text of include/ocrl_hip_iqn.h: the cosine features, the head, the
mean q, the quantile Huber loss of the TD step at given fractions (gradients by autograd), and a whole ``train_step`` (the restatement of
``DQN._train_step_iqn``: next quantile values from the target parameters at N' fractions, bootstrap action from the online ones under
double Q at N' fractions of their own, the loss at N fractions, clip + Adam of tests/dqn_ref.py).  Restated from the published algorithm
(Dabney, Ostrovski, Silver and Munos 2018) in the form the header writes it.  The fractions are inputs everywhere: the tests read them
back from the GPU (``ocrl_iqn_taus``) and never re-derive them.

Hand-worked values (test_iqn_cpu.py):
  * cosines c_k = cos(pi k tau): tau = 0.5 gives 1, 0, -1, 0, ...; tau = 0 gives all 1; tau = 1/3, k = 1 gives 0.5.
  * loss, B = A = N = N' = 1, the row not done with gamma 1 and reward 0, so T = next_quantiles; tau = 0.25, theta = 0.25, kappa = 1:
      T = 0.75:   u = 0.5 >= 0, weight |0.25 - 0| = 0.25, L = 0.5 * 0.25 = 0.125:   ql = 0.25 * 0.125 = 0.03125
      T = -2.75:  u = -3 < 0,   weight |0.25 - 1| = 0.75, L = 1 * (3 - 0.5) = 2.5:  ql = 0.75 * 2.5  = 1.875"""
import math

import torch

from . import dqn_ref as R
from . import qr_ref as Q


def make_params(F, A, C, dims, seed=0, dtype=torch.float32):
    """the kernels' order: the embedding's We [F, C] and be [F], then the chain and the output Linear [A, last] (dqn_ref.make_params)"""
    g = torch.Generator().manual_seed(seed + 2000)
    emb = [((torch.rand(F, C, generator=g) * 2 - 1) / C ** 0.5).to(dtype), ((torch.rand(F, generator=g) * 2 - 1) * 0.5).to(dtype)]
    return emb + R.make_params(F, A, dims, seed, dtype)


def cos_features(taus, C, dtype=torch.float64):
    """c [..., C] of fractions [...]: the fp32 product k * tau is formed first (one rounding), then cos(pi .) in fp64, then ``dtype``.
    The fp32 restatement rounds the fp64 cosine too: the device's cospif reduces its argument exactly, where an fp32 product with pi
    would lose 1e-5 of a cosine at k * tau near 63."""
    prod = taus.to(torch.float32).unsqueeze(-1) * torch.arange(C, dtype=torch.float32)
    return torch.cos(math.pi * prod.double()).to(dtype)


def quantiles(x, taus, params, acts, A, C):
    """(theta [B, A, N], q [B, A]) of features [B, F] at fractions taus [B, N], in the dtype of x and params"""
    We, be, chain = params[0], params[1], params[2:]
    phi = torch.relu(cos_features(taus, C, x.dtype) @ We.T + be)             # [B, N, F]
    h = x.unsqueeze(1) * phi
    for l, a in enumerate(acts):
        h = R.ACTS[a](h @ chain[2 * l].T + chain[2 * l + 1])
    theta = (h @ chain[-2].T + chain[-1]).transpose(1, 2)
    assert theta.shape[1] == A
    return theta, theta.mean(-1)


def iqn_loss(theta, taus, next_quantiles, next_q, actions, rewards, dones, gamma, kappa=1.0, discounts=None, weights=None):
    """(loss, mean q[a], mean of the targets, row_loss [B]) of ocrl_iqn_td_fwd_bwd in the dtype of the quantile values theta [B, A, N] at
    the fractions taus [B, N]; next_quantiles [B, A, N']"""
    B, A, N = theta.shape
    Np = next_quantiles.shape[2]
    dtype = theta.dtype
    a = actions.clamp(0, A - 1)
    disc = torch.full((B,), gamma, dtype=dtype) if discounts is None else discounts
    T = Q.targets(next_quantiles, next_q, rewards, dones, disc).detach()       # [B, N']
    ta = theta[torch.arange(B), a]
    u = T.unsqueeze(1) - ta.unsqueeze(2)                                         # [B, i, j]
    w = (taus.to(dtype).reshape(B, N, 1) - (u.detach() < 0).to(dtype)).abs()
    ql = (w * Q.huber(u, kappa)).sum(2).sum(1) / Np                              # summed over the head's fractions i, averaged over the target's j
    l = ql if weights is None else weights * ql
    return l.mean(), ta.mean(-1).mean(), T.mean(-1).mean(), ql.detach()


def iqn_step(x, taus, params, acts, A, C, next_quantiles, next_q, actions, rewards, dones, gamma, kappa=1.0, discounts=None, weights=None,
             dtype=torch.float64):
    """(scalars [3], dfeatures, [dw], row_loss [B]) of the TD step in `dtype`, by autograd"""
    x = x.detach().to(dtype).requires_grad_(True)
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, mt, ql = iqn_loss(quantiles(x, taus, ps, acts, A, C)[0], taus, next_quantiles.to(dtype), next_q.to(dtype), actions, rewards.to(dtype),
                                dones, gamma, kappa, opt(discounts), opt(weights))
    grads = torch.autograd.grad(loss, [x] + ps)
    return torch.stack([loss, mq, mt]).detach(), grads[0], list(grads[1:]), ql


def features(obs, ext):
    """the extractor's MLP on flattened observations: every Linear of ``ext`` = [W, b, ...] followed by a ReLU"""
    h = obs.flatten(1)
    for l in range(len(ext) // 2):
        h = torch.relu(h @ ext[2 * l].T + ext[2 * l + 1])
    return h


def train_step(cur, target, m, v, step, batch, taus, acts, A, C, gamma, kappa, double_q, lr, max_norm, split_cur, split_tgt, dtype=torch.float64):
    """one update of ``DQN._train_step_iqn`` on a given batch (observations, next observations, actions, rewards or n-step returns,
    dones, discounts or None, weights or None) and the step's fractions ``taus`` = (online [B, N], target [B, N'], online-on-next
    [B, N'] or None): (new parameters, new m, new v, scalars, row_loss).  ``cur`` / ``target``: the trainable parameters;
    ``split_cur`` / ``split_tgt`` map them to (the extractor's MLP, the head's parameters in make_params' order) (noisy heads: through
    ``qr_ref.noisy_chain`` of the step's draws)."""
    obs, nxt, a, r, d, disc, w = batch
    t_on, t_tg, t_dq = taus
    cur = [p.detach().to(dtype).requires_grad_(True) for p in cur]
    ext, head = split_cur(cur)
    with torch.no_grad():
        text, thead = split_tgt([p.to(dtype) for p in target])
        next_quantiles, next_q = quantiles(features(nxt.to(dtype), text), t_tg, thead, acts, A, C)
        if double_q:
            next_q = quantiles(features(nxt.to(dtype), [p.detach() for p in ext]), t_dq, [p.detach() for p in head], acts, A, C)[1]
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, mt, ql = iqn_loss(quantiles(features(obs.to(dtype), ext), t_on, head, acts, A, C)[0], t_on, next_quantiles, next_q, a, r.to(dtype), d,
                                gamma, kappa, opt(disc), opt(w))
    grads = torch.autograd.grad(loss, cur)
    new, m, v, _ = R.adam_update([p.detach() for p in cur], grads, m, v, step, lr, max_norm)
    return new, m, v, torch.stack([loss, mq, mt]).detach(), ql
