"""fp64 torch restatement of DQN's categorical head, from the text of include/ocrl_hip_c51.h: the head with the dueling rule, the support,
the projection of the target distribution in its gather form (what the kernel computes) and in the textbook scatter form (Bellemare et
al. 2017, algorithm 1), the cross-entropy loss (gradients by autograd), and a whole ``train_step`` (the restatement of
``DQN._train_step_c51``: next distribution from the target parameters, bootstrap action from the online ones under double Q, the loss,
clip + Adam of tests/dqn_ref.py).

Hand-worked batch (test_c51_cpu.py checks it through ``project_gather`` and ``project_scatter``): Z = 5 atoms on [0, 2], so dz = 0.5 and
z = (0, 0.5, 1, 1.5, 2); gamma = 0.5.
  * row 0 is done with reward 1.0, exactly atom 2: beta = 2, m = (0, 0, 1, 0, 0) whatever next_probs holds (NaN here).
  * row 1 is not done with reward 3.0: every T_j = clamp(3 + 0.5 z_j, 0, 2) = 2, beta_j = 4, m = (0, 0, 0, 0, 1) for any next_probs.
A third row shows the split: reward 0.25, next_probs (0.5, 0, 0, 0, 0.5): T_0 = 0.25 (beta 0.5: halves to atoms 0 and 1) and
T_4 = 1.25 (beta 2.5: halves to atoms 2 and 3) give m = (0.25, 0.25, 0.25, 0.25, 0)."""
import numpy as np
import torch

from . import dqn_ref as R

WORKED = dict(Z=5, v_min=0.0, v_max=2.0, gamma=0.5,
              next_probs=[[float("nan")] * 5, [0.1, 0.2, 0.3, 0.25, 0.15], [0.5, 0.0, 0.0, 0.0, 0.5]],
              rewards=[1.0, 3.0, 0.25], dones=[1, 0, 0],
              m=[[0.0, 0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 1.0], [0.25, 0.25, 0.25, 0.25, 0.0]])


def make_params(F, A, Z, dims, dueling, seed=0, dtype=torch.float32):
    """the chain and the advantage Linear [A * Z, last] in state_dict order (dqn_ref.make_params), then the value Linear [Z, last]"""
    ps = R.make_params(F, A * Z, dims, seed, dtype)
    if dueling:
        k = dims[-1] if len(dims) else F
        g = torch.Generator().manual_seed(seed + 1000)
        ps += [((torch.rand(Z, k, generator=g) * 2 - 1) / k ** 0.5).to(dtype), ((torch.rand(Z, generator=g) * 2 - 1) * 0.5).to(dtype)]
    return ps


def support(v_min, v_max, Z, dtype=torch.float64):
    """z_j = v_min + j dz"""
    dz = (v_max - v_min) / (Z - 1)
    return v_min + torch.arange(Z, dtype=dtype) * dz


def dueling_rule(adv, v):
    """logit[b, a, j] = V[b, j] + Adv[b, a, j] - mean_a' Adv[b, a', j]"""
    return v.unsqueeze(1) + adv - adv.mean(dim=1, keepdim=True)


def logits(x, params, acts, A, Z, dueling):
    """[B, A, Z] of features [B, F] in the dtype of its inputs; params as make_params orders them"""
    chain = params[:-2] if dueling else params
    h = x
    for l, a in enumerate(acts):
        h = R.ACTS[a](h @ chain[2 * l].T + chain[2 * l + 1])
    adv = (h @ chain[-2].T + chain[-1]).reshape(-1, A, Z)
    return dueling_rule(adv, h @ params[-2].T + params[-1]) if dueling else adv


def distribution(x, params, acts, A, Z, dueling, v_min, v_max):
    """(probs [B, A, Z], q [B, A])"""
    p = torch.softmax(logits(x, params, acts, A, Z, dueling), dim=-1)
    return p, (p * support(v_min, v_max, Z, p.dtype)).sum(-1)


def _betas(rewards, dones, disc, v_min, v_max, Z, dtype):
    """beta [B, Z]: where the target of atom j lands, in atoms; a done row's every column is the reward's own position"""
    z = support(v_min, v_max, Z, dtype)
    dz = (v_max - v_min) / (Z - 1)
    boot = torch.where(dones.bool().unsqueeze(1), torch.zeros(1, dtype=dtype), disc.unsqueeze(1) * z)
    return ((rewards.unsqueeze(1) + boot).clamp(v_min, v_max) - v_min) / dz


def project_gather(next_p, rewards, dones, disc, v_min, v_max, Z):
    """m [B, Z], the header's form: m_i = sum_j next_p[j] max(0, 1 - |beta_j - i|); a done row is the triangle at its reward (a select:
    its next_p is not read)"""
    dtype = rewards.dtype
    beta = _betas(rewards, dones, disc, v_min, v_max, Z, dtype)
    tri = (1 - (beta.unsqueeze(1) - torch.arange(Z, dtype=dtype).reshape(1, Z, 1)).abs()).clamp(min=0)         # [B, i, j]
    done = dones.bool()
    mass = torch.where(done.unsqueeze(1), torch.zeros(1, dtype=dtype), next_p)
    return torch.where(done.unsqueeze(1), tri[:, :, 0], (tri * mass.unsqueeze(1)).sum(-1))


def project_scatter(next_p, rewards, dones, disc, v_min, v_max, Z):
    """m [B, Z], the textbook form: the mass of target atom j goes to l = floor(beta_j) and u = ceil(beta_j) in the shares (u - beta_j)
    and (beta_j - l), and whole to l when beta_j is an integer; a done row carries mass 1 at its reward"""
    dtype = rewards.dtype
    beta = _betas(rewards, dones, disc, v_min, v_max, Z, dtype).numpy()
    p = next_p.numpy()
    m = np.zeros((len(beta), Z), dtype=beta.dtype)
    for b in range(len(beta)):
        cols = [(beta[b, 0], 1.0)] if dones[b] else [(beta[b, j], p[b, j]) for j in range(Z)]
        for bt, mass in cols:
            l, u = int(np.floor(bt)), int(np.ceil(bt))
            if l == u:
                m[b, l] += mass
            else:
                m[b, l] += mass * (u - bt)
                m[b, u] += mass * (bt - l)
    return torch.as_tensor(m)


def c51_loss(lg, next_probs, next_q, actions, rewards, dones, gamma, v_min, v_max, discounts=None, weights=None):
    """(loss, mean q[a], mean sum m z, row_loss [B]) of ocrl_c51_td_fwd_bwd in the dtype of the logits lg [B, A, Z]"""
    B, A, Z = lg.shape
    dtype = lg.dtype
    a = actions.clamp(0, A - 1)
    done = dones.bool()
    nq = torch.where(done.unsqueeze(1), torch.zeros(1, dtype=next_q.dtype), next_q)                             # a select: never read
    star = torch.as_tensor(np.argmax(nq.detach().numpy(), axis=1))                                               # numpy: the first of a tie
    disc = torch.full((B,), gamma, dtype=dtype) if discounts is None else discounts
    m = project_gather(next_probs[torch.arange(B), star], rewards, dones, disc, v_min, v_max, Z).detach()
    la = lg[torch.arange(B), a]
    logp = torch.log_softmax(la, dim=-1)
    ce = -(m * logp).sum(-1)
    z = support(v_min, v_max, Z, dtype)
    qa = (torch.softmax(la, dim=-1) * z).sum(-1)
    l = ce if weights is None else weights * ce
    return l.mean(), qa.mean(), (m * z).sum(-1).mean(), ce.detach()


def c51_step(x, params, acts, A, Z, dueling, v_min, v_max, next_probs, next_q, actions, rewards, dones, gamma, discounts=None, weights=None,
             dtype=torch.float64):
    """(scalars [3], dfeatures, [dw], row_loss [B]) of the TD step in `dtype`, by autograd"""
    x = x.detach().to(dtype).requires_grad_(True)
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, mt, ce = c51_loss(logits(x, ps, acts, A, Z, dueling), next_probs.to(dtype), next_q.to(dtype), actions, rewards.to(dtype), dones, gamma,
                                v_min, v_max, opt(discounts), opt(weights))
    grads = torch.autograd.grad(loss, [x] + ps)
    return torch.stack([loss, mq, mt]).detach(), grads[0], list(grads[1:]), ce


def train_step(cur, target, m, v, step, batch, acts, A, Z, dueling, v_min, v_max, gamma, double_q, lr, max_norm, dtype=torch.float64):
    """one update of ``DQN._train_step_c51`` on a given batch (observations, next observations, actions, rewards or n-step returns, dones,
    discounts or None, weights or None; observations flattened into feature rows of the chain): (new parameters, new m, new v, scalars,
    row_loss).  ``cur`` / ``target``: the whole chain (extractor MLP, then the head) in the order of make_params."""
    obs, nxt, a, r, d, disc, w = batch
    tgt = [p.to(dtype) for p in target]
    cur = [p.to(dtype) for p in cur]
    nx = nxt.flatten(1).to(dtype)
    next_probs, next_q = distribution(nx, tgt, acts, A, Z, dueling, v_min, v_max)
    if double_q:
        next_q = distribution(nx, cur, acts, A, Z, dueling, v_min, v_max)[1]
    scal, _, grads, ce = c51_step(obs.flatten(1), cur, acts, A, Z, dueling, v_min, v_max, next_probs.detach(), next_q.detach(), a, r, d, gamma, disc, w, dtype)
    new, m, v, _ = R.adam_update(cur, grads, m, v, step, lr, max_norm)
    return new, m, v, scal, ce
