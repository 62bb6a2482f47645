"""fp64 torch restatement of the DQN pieces, from the text of include/ocrl_hip_dqn.h: the Q head, the TD target with its select on
`done`, the Huber loss (gradients by autograd), one update (clip_grad_norm_ + Adam, eps 1e-8), and the integer rules of ocrl_dqn_act and
ocrl_replay_sample on the counter RNG of tests/gpu_util.py.

Hand-worked Huber example (test_dqn_cpu.py checks it through `td_loss`): three rows with delta = Q[a] - y = 0.5, -3, 1 give
    loss = (0.5 * 0.5^2 + (3 - 0.5) + (1 - 0.5)) / 3 = (0.125 + 2.5 + 0.5) / 3
    dQ[b, a_b] = clamp(delta, -1, 1) / 3 = (0.5, -1, 1) / 3."""
import numpy as np
import torch

from .gpu_util import _M32, _mix32k, rng_key

SITE_ACT, SITE_SAMPLE = 410, 420
ACTS = {0: lambda v: v, 1: torch.relu, 2: torch.tanh}


def make_params(F, A, dims, seed=0, dtype=torch.float32, scale=1.0):
    """[W_0, b_0, ..., W_out, b_out] in state_dict order; weights ~ U(-1, 1) / sqrt(fan_in) * scale"""
    g = torch.Generator().manual_seed(seed)
    ps, k = [], F
    for n in list(dims) + [A]:
        ps += [((torch.rand(n, k, generator=g) * 2 - 1) * scale / k ** 0.5).to(dtype), ((torch.rand(n, generator=g) * 2 - 1) * 0.5).to(dtype)]
        k = n
    return ps


def q_forward(x, params, acts):
    """features [B, F] through the hidden layers (activation codes `acts`) and the output Linear, in the dtype of its inputs"""
    h = x
    for l, a in enumerate(acts):
        h = ACTS[a](h @ params[2 * l].T + params[2 * l + 1])
    return h @ params[-2].T + params[-1]


def td_target(next_q, rewards, dones, gamma):
    """y = r + (done ? 0 : gamma max_a next_q): a select, so a non-finite next_q of a finished row does not reach y"""
    boot = gamma * next_q.max(dim=1).values
    return rewards + torch.where(dones.bool(), torch.zeros_like(boot), boot)


def td_loss(q, next_q, actions, rewards, dones, gamma):
    """(loss, mean Q[a], mean y): Huber with threshold 1 of Q[a] - y, a clamped into [0, A), mean over rows"""
    a = actions.clamp(0, q.shape[1] - 1).reshape(-1, 1)
    qa = q.gather(1, a).squeeze(1)
    y = td_target(next_q, rewards, dones, gamma)
    delta = qa - y
    l = torch.where(delta.abs() < 1, 0.5 * delta * delta, delta.abs() - 0.5)
    return l.mean(), qa.mean(), y.mean()


def td_step(x, params, acts, next_q, actions, rewards, dones, gamma, dtype=torch.float64):
    """(scalars [3], dfeatures, [dw]) of the TD step in `dtype`, by autograd"""
    x = x.detach().to(dtype).requires_grad_(True)
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    loss, mq, my = td_loss(q_forward(x, ps, acts), next_q.to(dtype), actions, rewards.to(dtype), dones, gamma)
    grads = torch.autograd.grad(loss, [x] + ps)
    return torch.stack([loss, mq, my]).detach(), grads[0], list(grads[1:])


# ---- the integer rules
def _bits(seed, site, hi, counters):
    """the two 32-bit words of the counter RNG (csrc/common.h rng_bits4_keyed) at key high word `hi`, as uint64 arrays"""
    c = np.asarray(counters, dtype=np.uint64)
    key = rng_key(seed, site, hi)
    k2 = np.uint64((key * 0x9E3779B9 + 0x7F4A7C15) & _M32)
    c = c ^ np.uint64(key)
    return _mix32k(c, k2), (_mix32k(c ^ np.uint64(0x68E31DA4), k2) + np.uint64(key)) & np.uint64(_M32)


def act_uniforms(seed, row_offset, n):
    """[n, 2] float32: (u0, u1) of rows row_offset .. row_offset + n - 1 (all below 2^32) of stream `seed`"""
    rows = np.arange(row_offset, row_offset + n, dtype=np.uint64)
    assert int(rows.max()) < 2 ** 32
    x, y = _bits(seed, SITE_ACT, 0, rows)
    return np.stack([(x >> np.uint64(8)).astype(np.float32), (y >> np.uint64(8)).astype(np.float32)], axis=1) / np.float32(16777216.0)


def act_rule(q, uniforms, epsilon):
    """(actions, explore) of q [B, A] and uniforms [B, 2] (numpy): u0 < epsilon takes (bits24(u1) * A) >> 24, else the lowest argmax"""
    q, u = np.asarray(q), np.asarray(uniforms, dtype=np.float32)
    A = q.shape[1]
    explore = u[:, 0] < np.float32(epsilon)
    b1 = (u[:, 1].astype(np.float64) * 16777216.0).astype(np.int64)
    return np.where(explore, (b1 * A) >> 24, q.argmax(axis=1)), explore


def sample_rule(seed, update, B, N, E, pos, full):
    """idx int64 [B] of ocrl_replay_sample"""
    x, y = _bits(seed, SITE_SAMPLE, update & _M32, np.arange(B, dtype=np.uint64))
    below = lambda w, m: ((w * np.uint64(m)) >> np.uint64(32)).astype(np.int64)          # w < 2^32, m < 2^31: no overflow
    t = (pos + 1 + below(x, N - 1)) % N if full else below(x, pos)
    return t * E + below(y, E)


# ---- the loop's counters
def loop_counts(total_timesteps, n_envs, train_freq, gradient_steps, learning_starts, target_update_interval):
    """(vec steps, gradient steps, target updates) that ``learn(total_timesteps)`` takes from a fresh DQN: an iteration is train_freq vec
    steps of n_envs timesteps, then gradient_steps updates once num_timesteps > learning_starts; the target follows every
    max(target_update_interval // n_envs, 1) vec steps"""
    t = calls = updates = targets = 0
    every = max(target_update_interval // n_envs, 1)
    while t < total_timesteps:
        for _ in range(train_freq):
            t += n_envs
            calls += 1
            targets += calls % every == 0
        if t > learning_starts:
            updates += gradient_steps
    return calls, updates, targets


# ---- one update
def adam_update(params, grads, m, v, step, lr, max_norm, eps=1e-8, b1=0.9, b2=0.999):
    """clip_grad_norm_(max_norm) then Adam, out of place: (new params, new m, new v, the norm before clipping)"""
    norm = torch.sqrt(sum((g * g).sum() for g in grads))
    c = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    out_p, out_m, out_v = [], [], []
    for p, g, mm, vv in zip(params, grads, m, v):
        g = g * c
        mm = b1 * mm + (1 - b1) * g
        vv = b2 * vv + (1 - b2) * g * g
        out_p.append(p - lr * (mm / (1 - b1 ** step)) / ((vv / (1 - b2 ** step)).sqrt() + eps))
        out_m.append(mm)
        out_v.append(vv)
    return out_p, out_m, out_v, norm
