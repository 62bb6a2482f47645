"""torch restatement of DQN's fully parameterized quantile function, from the text of include/ocrl_hip_fqf.h: the proposal of the
fractions, the interval-weighted q, the collection step's q, the fraction loss's gradient into the proposal's Linear, and a whole
``train_step`` (the restatement of ``DQN._train_step_fqf``).  Every function works in the dtype of its inputs: fp64 is the reference, fp32
the measure of what fp32 arithmetic may cost (the bound of tests/test_gpu_fqf.py).  The head is tests/iqn_ref.py's.  Restated from the
published algorithm (Yang, Zhao, Lin, Qin, Bian and Liu 2019) in the form the header writes it.

The fraction loss.  For a quantile function F^-1 and boundaries 0 = tau_0 <= ... <= tau_N = 1 with midpoints tau_hat_i, the 1-Wasserstein
error of the staircase is W1 = sum_i int_{tau_i}^{tau_{i+1}} |F^-1(w) - F^-1(tau_hat_i)| dw, and for a non-decreasing F^-1
dW1 / dtau_i = 2 F^-1(tau_i) - F^-1(tau_hat_i) - F^-1(tau_hat_{i-1}) (the paper's Proposition 1): ``w1_exact`` and ``g_analytic`` hold the
two sides for closed-form F^-1, and test_fqf_cpu.py compares them through autograd."""
import torch

from . import a2c_ref as A2
from . import dqn_ref as R
from . import iqn_ref as I

RMS_ALPHA, RMS_EPS = 0.95, 1e-5


def fractions(x, Wf, bf):
    """(taus [B, N + 1], tau_hats [B, N], eval_taus [B, 2 N - 1], logp [B, N], entropy [B]) of features [B, F]: the prefix sums are
    formed on the un-normalised e and divided once, as the header writes it"""
    z = x @ Wf.T + bf
    zm = z - z.max(dim=1, keepdim=True).values
    e = zm.exp()
    c = e.cumsum(1)
    Z = c[:, -1:]
    logp = zm - Z.log()
    p = logp.exp()
    taus = torch.cat([torch.zeros_like(Z), c / Z], dim=1)
    tau_hats = 0.5 * (taus[:, :-1] + taus[:, 1:])
    return taus, tau_hats, torch.cat([taus[:, 1:-1], tau_hats], dim=1), logp, -(p * logp).sum(1)


def weighted_q(theta, taus):
    """q [B, A] = sum_i (tau_{i+1} - tau_i) theta[b, a, i]"""
    return (theta * (taus[:, 1:] - taus[:, :-1]).unsqueeze(1)).sum(-1)


def act_q(x, taus, params, acts, A, C):
    """(theta at the midpoints of taus, the weighted q): what ocrl_fqf_act evaluates"""
    theta = I.quantiles(x, 0.5 * (taus[:, :-1] + taus[:, 1:]), params, acts, A, C)[0]
    return theta, weighted_q(theta, taus)


def g_analytic(theta_tau, theta_hat):
    """dW1 / dtau_i, i = 1 .. N-1, of quantile values theta_tau [..., N - 1] at tau_1 .. tau_{N-1} and theta_hat [..., N] at the midpoints"""
    return 2 * theta_tau - theta_hat[..., 1:] - theta_hat[..., :-1]


def fraction_dz(logp, entropy, g, ent_coef=0.0):
    """dz [B, N], the cotangent of the proposal's logits, of g [B, N - 1] = g_1 .. g_{N-1} (scaled by w_b / B already)"""
    B = logp.shape[0]
    p = logp.exp()
    gz = torch.cat([g, torch.zeros(B, 1, dtype=g.dtype)], dim=1)                  # g_{k+1} at column k
    dp = gz.flip(1).cumsum(1).flip(1)                                             # dp_k = sum_{i > k} g_i
    s = (p * dp).sum(1, keepdim=True)
    return p * (dp - s) + (ent_coef / B) * p * (logp + entropy.unsqueeze(1))


def fraction_grads(x, logp, entropy, theta_eval, actions, weights=None, ent_coef=0.0):
    """(dWf [N, F], dbf [N], scalars [2] = (fraction loss, mean entropy)) of ocrl_fqf_fraction_bwd, the header's formulas written out:
    theta_eval [B, A, 2 N - 1] is the head at eval_taus, logp / entropy what ``fractions`` gave"""
    B, N = logp.shape
    A = theta_eval.shape[1]
    th = theta_eval[torch.arange(B), actions.clamp(0, A - 1)]                     # [B, 2 N - 1]
    w = torch.ones(B, dtype=x.dtype) if weights is None else weights.to(x.dtype)
    g = (w / B).unsqueeze(1) * g_analytic(th[:, :N - 1], th[:, N - 1:])           # [B, N - 1]: g_1 .. g_{N-1}
    t = logp.exp().cumsum(1)[:, :-1]                                              # tau_1 .. tau_{N-1}
    dz = fraction_dz(logp, entropy, g, ent_coef)
    return dz.T @ x, dz.sum(0), torch.stack([(g * t).sum(), entropy.mean()])


def fraction_objective(z, g, ent_coef=0.0):
    """the scalar whose gradient with respect to the logits z [B, N] is ``fraction_dz``, for autograd: sum_b sum_i g_i tau_i with g held
    constant (the paper's way of following dW1 / dtau) minus ent_coef * mean_b H_b, through log_softmax and cumsum"""
    logp = torch.log_softmax(z, dim=1)
    p = logp.exp()
    return (g * p.cumsum(1)[:, :-1]).sum() - ent_coef * (-(p * logp).sum(1)).mean()


def w1_exact(taus, Finv, prim):
    """the exact 1-Wasserstein error of the staircase at boundaries taus [N + 1] (fp64, attached) for a non-decreasing quantile function
    ``Finv`` with primitive ``prim``: on [tau_i, tau_hat_i] the staircase lies above F^-1, on [tau_hat_i, tau_{i+1}] below"""
    lo, hi = taus[:-1], taus[1:]
    mid = 0.5 * (lo + hi)
    fm = Finv(mid)
    return (fm * (mid - lo) - (prim(mid) - prim(lo)) + (prim(hi) - prim(mid)) - fm * (hi - mid)).sum()


def train_step(cur, target, m, v, step, batch, fr, acts, A, C, gamma, kappa, double_q, lr, max_norm, split_cur, split_tgt, frac, frac_sq, frac_lr,
               ent_coef, dtype=torch.float64):
    """one update of ``DQN._train_step_fqf`` on a given batch (tests/iqn_ref.train_step's tuple) and the step's fractions ``fr`` = (taus,
    tau_hats, eval_taus, logp, entropy) as the run proposed them: (new parameters, new m, new v, scalars, row_loss, new (Wf, bf), new
    frac_sq, the fraction scalars).  ``cur`` / ``target`` are the trainable parameters without the proposal's, ``frac`` = (Wf, bf)."""
    obs, nxt, a, r, d, disc, w = batch
    taus, tau_hats, eval_taus, logp, entropy = fr
    cur = [p.detach().to(dtype).requires_grad_(True) for p in cur]
    ext, head = split_cur(cur)
    opt = lambda t: None if t is None else t.to(dtype)
    with torch.no_grad():
        text, thead = split_tgt([p.to(dtype) for p in target])
        next_quantiles = I.quantiles(I.features(nxt.to(dtype), text), tau_hats, thead, acts, A, C)[0]
        next_q = weighted_q(next_quantiles, taus.to(dtype))
        if double_q:
            next_q = weighted_q(I.quantiles(I.features(nxt.to(dtype), [p.detach() for p in ext]), tau_hats, [p.detach() for p in head], acts, A, C)[0],
                                taus.to(dtype))
    x = I.features(obs.to(dtype), ext)
    loss, mq, mt, ql = I.iqn_loss(I.quantiles(x, tau_hats, head, acts, A, C)[0], tau_hats, next_quantiles, next_q, a, r.to(dtype), d, gamma, kappa,
                                  opt(disc), opt(w))
    grads = torch.autograd.grad(loss, cur)
    with torch.no_grad():
        theta_eval = I.quantiles(x.detach(), eval_taus, [p.detach() for p in head], acts, A, C)[0]
        dW, db, fscal = fraction_grads(x.detach(), logp.to(dtype), entropy.to(dtype), theta_eval, a, opt(w), ent_coef)
    new, m, v, _ = R.adam_update([p.detach() for p in cur], grads, m, v, step, lr, max_norm)
    Wf, bf = (t.to(dtype) for t in frac)
    rms = A2.rmsprop_tf_l2(torch.cat([Wf.flatten(), bf]), torch.cat([dW.flatten(), db]), frac_sq, 0.0, frac_lr, RMS_ALPHA, RMS_EPS, dtype)
    nW = rms.p[:Wf.numel()].view_as(Wf)
    return new, m, v, torch.stack([loss, mq, mt]).detach(), ql, (nW, rms.p[Wf.numel():]), rms.sq, fscal
