"""Torch restatement of DQN's Munchausen targets, from the text of include/ocrl_hip_munchausen.h: the soft-max policy of a row of action
values, the clipped log-policy bonus, the soft value and the policy's mixture of the quantile values, in the dtype of its inputs (fp64 for
the truth, fp32 for the facts that hold bit for bit), with every sum serial in ascending a as the header orders it.  With them the
restatements of ``DQN._train_step_dqn`` / ``_train_step_qr`` / ``_train_step_iqn`` under ``munchausen=True``: the target parameters
evaluated on the observations as well, ``targets``, then the unchanged losses of tests/replay_ext_ref.py, tests/qr_ref.py and
tests/iqn_ref.py, clip + Adam of tests/dqn_ref.py.  Restated from the published algorithm (Vieillard, Pietquin and Geist 2020) in the form
the header writes it.

Hand-worked rows (test_munchausen_cpu.py), alpha = 0.9, clip_lo = -1:
  * A = 1: v = x, s = 0, Z = 1, logpi = 0, pi = 1: the bonus is 0, V = next_q, M = next_quantiles.
  * an all-equal row of A entries x: s = 0, Z = A, logpi = -ln A, pi = 1 / A, c = tau logpi = -tau ln A: V = x + tau ln A,
    M_j = mean_a next_quantiles[a, j] + tau ln A, and the bonus is -alpha tau ln A while tau ln A <= 1.
  * the action taken lies more than 1000 tau below the maximum: c_a = (x_a - v) - tau ln Z < -1000 tau, which is below clip_lo = -1
    at tau >= 0.001: the bonus is alpha * clip_lo exactly.
  * a finished row: next_v = 0 and next_m = 0 whatever next_q and next_quantiles hold (NaN, inf); the bonus is still added."""
import torch

from . import dqn_ref as R
from . import iqn_ref as I
from . import qr_ref as Q
from . import replay_ext_ref as X


def policy(x, tau):
    """(logpi, pi, c = tau logpi) [B, A] of action values x [B, A] in the dtype of x: s = (x - max) / tau, Z = the serial sum of exp(s),
    logpi = s - log Z, pi = exp(logpi)"""
    v = x.max(dim=1, keepdim=True).values
    s = (x - v) / tau
    e = torch.exp(s)
    Z = torch.zeros_like(x[:, 0])
    for a in range(x.shape[1]):
        Z = Z + e[:, a]
    logpi = s - torch.log(Z).unsqueeze(1)
    return logpi, torch.exp(logpi), tau * logpi


def targets(cur_q, next_q, actions, rewards, dones, alpha, tau, clip_lo, next_quantiles=None):
    """(rewards_out [B], next_v [B, A], next_m [B, A, N'] or None) of ocrl_munchausen_targets in the dtype of cur_q.  A finished row's
    next_q and next_quantiles are never read: they are replaced before any arithmetic"""
    dtype = cur_q.dtype
    B, A = cur_q.shape
    done = dones.bool()
    a = actions.clamp(0, A - 1)
    c = policy(cur_q, tau)[2][torch.arange(B), a]
    zero = torch.zeros((), dtype=dtype)
    bonus = alpha * torch.minimum(zero, torch.maximum(torch.full((), clip_lo, dtype=dtype), c))
    rewards_out = rewards.to(dtype) + bonus
    nq = torch.where(done.unsqueeze(1), zero, next_q.to(dtype))
    _, pi, cn = policy(nq, tau)
    V = torch.zeros(B, dtype=dtype)
    for k in range(A):
        V = V + pi[:, k] * (nq[:, k] - cn[:, k])
    next_v = torch.where(done.unsqueeze(1), zero, V.unsqueeze(1).expand(B, A))
    if next_quantiles is None:
        return rewards_out, next_v, None
    Np = next_quantiles.shape[2]
    nqt = torch.where(done.reshape(B, 1, 1), zero, next_quantiles.to(dtype))
    M = torch.zeros(B, Np, dtype=dtype)
    for k in range(A):
        M = M + pi[:, k].unsqueeze(1) * (nqt[:, k] - cn[:, k].unsqueeze(1))
    next_m = torch.where(done.reshape(B, 1, 1), zero, M.unsqueeze(1).expand(B, A, Np))
    return rewards_out, next_v.contiguous(), next_m.contiguous()


def _finish(cur, loss, scal, row, m, v, step, lr, max_norm):
    grads = torch.autograd.grad(loss, cur)
    new, m, v, _ = R.adam_update([p.detach() for p in cur], grads, m, v, step, lr, max_norm)
    return new, m, v, scal.detach(), row


def dqn_train_step(cur, target, m, v, step, batch, acts, mun, gamma, lr, max_norm, dtype=torch.float64, chain_cur=None, chain_tgt=None):
    """one update of ``DQN._train_step_dqn`` with munchausen = (alpha, tau, clip_lo) on a given batch (observations, next observations,
    actions, rewards or n-step returns, dones, discounts or None, weights or None; observations flattened into feature rows of the
    chain): (new parameters, new m, new v, scalars, |delta| [B]).  ``chain_cur`` / ``chain_tgt`` as tests/qr_ref.py's train_step takes
    them"""
    obs, nxt, a, r, d, disc, w = batch
    same = lambda ps: ps
    cur = [p.detach().to(dtype).requires_grad_(True) for p in cur]
    online = (chain_cur or same)(cur)
    ob, nx = obs.flatten(1).to(dtype), nxt.flatten(1).to(dtype)
    with torch.no_grad():
        tgt = (chain_tgt or same)([p.to(dtype) for p in target])
        rm, nv, _ = targets(R.q_forward(ob, tgt, acts), R.q_forward(nx, tgt, acts), a, r.to(dtype), d, *mun)
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, my, ad = X.td_loss_ext(R.q_forward(ob, online, acts), nv, a, rm, d, gamma, None, opt(disc), opt(w))
    return _finish(cur, loss, torch.stack([loss, mq, my]), ad, m, v, step, lr, max_norm)


def qr_train_step(cur, target, m, v, step, batch, acts, A, N, dueling, mun, gamma, kappa, lr, max_norm, dtype=torch.float64, chain_cur=None,
                  chain_tgt=None):
    """the same of ``DQN._train_step_qr``: (new parameters, new m, new v, scalars, row_loss [B])"""
    obs, nxt, a, r, d, disc, w = batch
    same = lambda ps: ps
    cur = [p.detach().to(dtype).requires_grad_(True) for p in cur]
    online = (chain_cur or same)(cur)
    ob, nx = obs.flatten(1).to(dtype), nxt.flatten(1).to(dtype)
    with torch.no_grad():
        tgt = (chain_tgt or same)([p.to(dtype) for p in target])
        next_quantiles, next_q = Q.quantiles(nx, tgt, acts, A, N, dueling)
        rm, nv, nm = targets(Q.quantiles(ob, tgt, acts, A, N, dueling)[1], next_q, a, r.to(dtype), d, *mun, next_quantiles=next_quantiles)
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, mt, ql = Q.qr_loss(Q.quantiles(ob, online, acts, A, N, dueling)[0], nm, nv, a, rm, d, gamma, kappa, opt(disc), opt(w))
    return _finish(cur, loss, torch.stack([loss, mq, mt]), ql, m, v, step, lr, max_norm)


def iqn_train_step(cur, target, m, v, step, batch, taus, acts, A, C, mun, gamma, kappa, lr, max_norm, split_cur, split_tgt, dtype=torch.float64):
    """the same of ``DQN._train_step_iqn``; ``taus`` = (online [B, N], target on the next observations [B, N'], target on the
    observations [B, N']: draws 0, 1 and 2 of the update); ``split_cur`` / ``split_tgt`` as tests/iqn_ref.py's train_step takes them"""
    obs, nxt, a, r, d, disc, w = batch
    t_on, t_nx, t_ob = taus
    cur = [p.detach().to(dtype).requires_grad_(True) for p in cur]
    ext, head = split_cur(cur)
    with torch.no_grad():
        text, thead = split_tgt([p.to(dtype) for p in target])
        next_quantiles, next_q = I.quantiles(I.features(nxt.to(dtype), text), t_nx, thead, acts, A, C)
        cur_q = I.quantiles(I.features(obs.to(dtype), text), t_ob, thead, acts, A, C)[1]
        rm, nv, nm = targets(cur_q, next_q, a, r.to(dtype), d, *mun, next_quantiles=next_quantiles)
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, mt, ql = I.iqn_loss(I.quantiles(I.features(obs.to(dtype), ext), t_on, head, acts, A, C)[0], t_on, nm, nv, a, rm, d, gamma, kappa, opt(disc),
                                  opt(w))
    return _finish(cur, loss, torch.stack([loss, mq, mt]), ql, m, v, step, lr, max_norm)
