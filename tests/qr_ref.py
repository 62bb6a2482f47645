"""fp64 torch restatement of DQN's quantile head, from the text of include/ocrl_hip_qr.h: the head with the dueling rule, the mean q, the
quantile Huber loss of the TD step (gradients by autograd), and a whole ``train_step`` (the restatement of ``DQN._train_step_qr``: next
quantiles from the target parameters, bootstrap action from the online ones under double Q, the loss, clip + Adam of tests/dqn_ref.py).
Restated from the published algorithm (Dabney et al. 2018) in the form the header writes it.

Hand-worked values (test_qr_cpu.py), B = 1, A = 1, the row not done with next quantiles 0, so T = r:
  * N = 1: tau = 0.5 whatever the sign of u, so ql = 0.5 L(T - theta): theta 0.25, T 0.75, kappa 1 gives 0.5 * 0.5 * 0.25 = 0.0625, and
    T 3.25 gives 0.5 * 1 * (3 - 0.5) = 1.25.
  * N = 2, theta = (0, 1), T = (0.5, 3), kappa = 1, tau = (0.25, 0.75):
      i = 0: u = (0.5, 3), both >= 0, weights 0.25:  0.25 * 0.125 + 0.25 * 2.5 = 0.65625
      i = 1: u = (-0.5, 2), weights (0.25, 0.75):    0.25 * 0.125 + 0.75 * 1.5 = 1.15625
    ql = 0.5 * 0.65625 + 0.5 * 1.15625 = 0.90625;  dL/dtheta = -(1 / 2) (0.25 * 0.5 + 0.25 * 1, -0.25 * 0.5 + 0.75 * 1) = (-0.1875, -0.3125)."""
import numpy as np
import torch

from . import dqn_ref as R


def make_params(F, A, N, dims, dueling, seed=0, dtype=torch.float32):
    """the chain and the advantage Linear [A * N, last] in state_dict order (dqn_ref.make_params), then the value Linear [N, last]"""
    ps = R.make_params(F, A * N, dims, seed, dtype)
    if dueling:
        k = dims[-1] if len(dims) else F
        g = torch.Generator().manual_seed(seed + 1000)
        ps += [((torch.rand(N, k, generator=g) * 2 - 1) / k ** 0.5).to(dtype), ((torch.rand(N, generator=g) * 2 - 1) * 0.5).to(dtype)]
    return ps


def taus(N, dtype=torch.float64):
    """tau_i = (i + 0.5) / N"""
    return (torch.arange(N, dtype=dtype) + 0.5) / N


def quantiles(x, params, acts, A, N, dueling):
    """(theta [B, A, N], q [B, A]) of features [B, F] in the dtype of its inputs; params as make_params orders them"""
    chain = params[:-2] if dueling else params
    h = x
    for l, a in enumerate(acts):
        h = R.ACTS[a](h @ chain[2 * l].T + chain[2 * l + 1])
    theta = (h @ chain[-2].T + chain[-1]).reshape(-1, A, N)
    if dueling:
        theta = (h @ params[-2].T + params[-1]).unsqueeze(1) + theta - theta.mean(dim=1, keepdim=True)
    return theta, theta.mean(-1)


def targets(next_quantiles, next_q, rewards, dones, disc):
    """T [B, N]: r + g * the quantiles of the action with the largest next_q (the first of a tie); r alone for a finished row, whose
    next_quantiles and next_q are never read"""
    B = next_q.shape[0]
    done = dones.bool()
    nq = torch.where(done.unsqueeze(1), torch.zeros(1, dtype=next_q.dtype), next_q)
    star = torch.as_tensor(np.argmax(nq.detach().numpy(), axis=1))                                               # numpy: the first of a tie
    boot = torch.where(done.unsqueeze(1), torch.zeros(1, dtype=next_quantiles.dtype), next_quantiles[torch.arange(B), star])
    return rewards.unsqueeze(1) + torch.where(done.unsqueeze(1), torch.zeros(1, dtype=boot.dtype), disc.unsqueeze(1) * boot)


def huber(u, kappa):
    """L(u) = 0.5 u^2 if |u| <= kappa, else kappa (|u| - 0.5 kappa)"""
    au = u.abs()
    return torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa))


def pair_terms(theta_a, T, kappa):
    """(u [B, i, j], |tau_i - [u < 0]| [B, i, j]) of the chosen action's quantiles theta_a [B, N] and the targets T [B, N]"""
    u = T.unsqueeze(1) - theta_a.unsqueeze(2)
    tau = taus(theta_a.shape[1], theta_a.dtype).reshape(1, -1, 1)
    return u, (tau - (u.detach() < 0).to(theta_a.dtype)).abs()


def qr_loss(theta, next_quantiles, next_q, actions, rewards, dones, gamma, kappa=1.0, discounts=None, weights=None):
    """(loss, mean q[a], mean of the targets, row_loss [B]) of ocrl_qr_td_fwd_bwd in the dtype of the quantile values theta [B, A, N]"""
    B, A, N = theta.shape
    dtype = theta.dtype
    a = actions.clamp(0, A - 1)
    disc = torch.full((B,), gamma, dtype=dtype) if discounts is None else discounts
    T = targets(next_quantiles, next_q, rewards, dones, disc).detach()
    ta = theta[torch.arange(B), a]
    u, w = pair_terms(ta, T, kappa)
    ql = (w * huber(u, kappa)).sum(2).sum(1) / N                    # summed over the head's quantiles i, averaged over the target's j
    l = ql if weights is None else weights * ql
    return l.mean(), ta.mean(-1).mean(), T.mean(-1).mean(), ql.detach()


def qr_step(x, params, acts, A, N, dueling, next_quantiles, next_q, actions, rewards, dones, gamma, kappa=1.0, discounts=None, weights=None,
            dtype=torch.float64):
    """(scalars [3], dfeatures, [dw], row_loss [B]) of the TD step in `dtype`, by autograd"""
    x = x.detach().to(dtype).requires_grad_(True)
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, mt, ql = qr_loss(quantiles(x, ps, acts, A, N, dueling)[0], next_quantiles.to(dtype), next_q.to(dtype), actions, rewards.to(dtype), dones,
                               gamma, kappa, opt(discounts), opt(weights))
    grads = torch.autograd.grad(loss, [x] + ps)
    return torch.stack([loss, mq, mt]).detach(), grads[0], list(grads[1:]), ql


def noisy_chain(params, n_plain, layers, fac):
    """the chain the kernels receive when the head's Linears are noisy: the first ``n_plain`` tensors as they are, then per layer of
    ``layers`` = (in, out) the four tensors (weight, bias, weight_sigma, bias_sigma) folded into weight + weight_sigma * (f_out f_in^T)
    and bias + bias_sigma * f_out with the factors ``fac`` of a draw (the layout of tests/noisy_ref.py); differentiable"""
    from . import noisy_ref as NR
    out = list(params[:n_plain])
    dtype = params[0].dtype
    for l, (fi, fo) in enumerate(NR.split(layers, fac.to(dtype))):
        w, b, ws, bs = params[n_plain + 4 * l:n_plain + 4 * l + 4]
        out += [w + ws * (fo.unsqueeze(1) * fi.unsqueeze(0)), b + bs * fo]
    return out


def train_step(cur, target, m, v, step, batch, acts, A, N, dueling, gamma, kappa, double_q, lr, max_norm, dtype=torch.float64, chain_cur=None,
               chain_tgt=None):
    """one update of ``DQN._train_step_qr`` on a given batch (observations, next observations, actions, rewards or n-step returns, dones,
    discounts or None, weights or None; observations flattened into feature rows of the chain): (new parameters, new m, new v, scalars,
    row_loss).  ``cur`` / ``target``: the trainable parameters; ``chain_cur`` / ``chain_tgt`` map them to the whole chain (extractor MLP,
    then the head) in the order of make_params (None: they are that chain already; noisy heads: ``noisy_chain`` of the step's draws)."""
    obs, nxt, a, r, d, disc, w = batch
    same = lambda ps: ps
    cur = [p.detach().to(dtype).requires_grad_(True) for p in cur]
    online = (chain_cur or same)(cur)
    with torch.no_grad():
        tgt = (chain_tgt or same)([p.to(dtype) for p in target])
        nx = nxt.flatten(1).to(dtype)
        next_quantiles, next_q = quantiles(nx, tgt, acts, A, N, dueling)
        if double_q:
            next_q = quantiles(nx, [p.detach() for p in online], acts, A, N, dueling)[1]
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, mt, ql = qr_loss(quantiles(obs.flatten(1).to(dtype), online, acts, A, N, dueling)[0], next_quantiles, next_q, a, r.to(dtype), d, gamma, kappa,
                               opt(disc), opt(w))
    grads = torch.autograd.grad(loss, cur)
    new, m, v, _ = R.adam_update([p.detach() for p in cur], grads, m, v, step, lr, max_norm)
    return new, m, v, torch.stack([loss, mq, mt]).detach(), ql
