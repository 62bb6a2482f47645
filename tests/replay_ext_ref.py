"""numpy float32 / Python-int restatement of DQN's replay extensions, from the text of include/ocrl_hip_replay.h: the n-step sampling
rule, the n-step walk over the ring, the extended TD step (fp64 torch, gradients by autograd), the priority's fixed point, the prefix
search of the priority store and its importance weights.

Hand-worked examples (test_replay_ext_cpu.py checks them through the functions below):
  * a 3-step return that stops on a done at k = 1: rewards (1, 2, 4), dones (0, 1, 0), gamma = 0.5 give R = 1 + 0.5 * 2 = 2,
    discount = 0.25 (two steps were taken), done = 1 and the next observation is the one two slots on.
  * leaves (3, 0, 2, 5): inclusive prefixes (3, 3, 5, 10).  target 2 -> id 0; target 3, exactly the boundary, -> id 2 (the smallest i whose
    prefix exceeds 3; the zero leaf 1 is skipped); target 4 -> id 2; target 5 -> id 3; target 9 -> id 3.
  * the fixed point at alpha = 1, eps = 0: |delta| = 0 -> 1 (the floor is clamped up), 1 -> 65536, 1e4 -> 2^24 (clamped down),
    inf and NaN -> 2^24."""
import numpy as np
import torch

from .dqn_ref import SITE_SAMPLE, _bits, sample_rule, td_target  # noqa: F401  (sample_rule: the n = 1 rule, re-exported for the tests)
from .gpu_util import _M32

SITE_PER = 430
FAN = 64
Q_ONE, Q_MAX = 1 << 16, 1 << 24
f32 = np.float32


# ---- n-step sampling and the walk
def sample_nstep_rule(seed, update, B, N, E, pos, full, n):
    """idx int64 [B] of ocrl_replay_sample_nstep"""
    x, y = _bits(seed, SITE_SAMPLE, update & _M32, np.arange(B, dtype=np.uint64))
    below = lambda w, m: ((w * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
    t = (pos + 1 + below(x, N - n)) % N if full else below(x, pos - n + 1)
    return t * E + below(y, E)


def valid_slots(N, pos, full, n):
    """the slots whose n-step window and the observation after it are stored"""
    return {(pos + 1 + k) % N for k in range(N - n)} if full else set(range(pos - n + 1))


def nstep_walk(rewards, dones, N, E, n, gamma, idx):
    """(returns f32 [B], discounts f32 [B], dones uint8 [B], steps m int [B]) of ocrl_replay_gather_nstep: a float32 loop in the written
    order; rewards, dones [N, E]"""
    rewards, dones = np.asarray(rewards, dtype=f32), np.asarray(dones)
    out = []
    for i in np.clip(np.asarray(idx, dtype=np.int64), 0, N * E - 1):
        t, e = divmod(int(i), E)
        R, g, stop, m = f32(0), f32(1), 0, 0
        for k in range(n):
            s = (t + k) % N
            R = f32(R + f32(g * rewards[s, e]))
            g = f32(g * f32(gamma))
            m = k + 1
            stop = int(dones[s, e])
            if stop:
                break
        out.append((R, g, stop, m))
    R, g, stop, m = zip(*out)
    return np.array(R, dtype=f32), np.array(g, dtype=f32), np.array(stop, dtype=np.uint8), np.array(m, dtype=np.int64)


# ---- the extended TD step, fp64
def td_loss_ext(q, next_q, actions, rewards, dones, gamma, next_q_online=None, discounts=None, weights=None):
    """(loss, mean Q[a], mean y, |delta| [B]) of ocrl_dqn_td_fwd_bwd_ext in the dtype of q"""
    B, A = q.shape
    a = actions.clamp(0, A - 1).reshape(-1, 1)
    qa = q.gather(1, a).squeeze(1)
    star = torch.as_tensor(np.argmax((next_q if next_q_online is None else next_q_online).detach().numpy(), axis=1)).reshape(-1, 1)      # numpy: the first of a tie
    boot = next_q.gather(1, star).squeeze(1)
    disc = torch.full_like(boot, gamma) if discounts is None else discounts
    y = rewards + torch.where(dones.bool(), torch.zeros_like(boot), disc * boot)
    delta = qa - y
    l = torch.where(delta.abs() < 1, 0.5 * delta * delta, delta.abs() - 0.5)
    if weights is not None:
        l = weights * l
    return l.mean(), qa.mean(), y.mean(), delta.abs().detach()


def td_step_ext(x, params, acts, next_q, actions, rewards, dones, gamma, next_q_online=None, discounts=None, weights=None, dtype=torch.float64):
    """(scalars [3], dfeatures, [dw], |delta| [B]) of the extended TD step in `dtype`, by autograd"""
    from .dqn_ref import q_forward
    x = x.detach().to(dtype).requires_grad_(True)
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    opt = lambda t: None if t is None else t.to(dtype)
    loss, mq, my, ad = td_loss_ext(q_forward(x, ps, acts), next_q.to(dtype), actions, rewards.to(dtype), dones, gamma, opt(next_q_online), opt(discounts),
                                   opt(weights))
    grads = torch.autograd.grad(loss, [x] + ps)
    return torch.stack([loss, mq, my]).detach(), grads[0], list(grads[1:]), ad


# ---- the priority store
def quantise(abs_td, alpha, eps):
    """q uint32-valued int64 [B] in float32, in the header's order of roundings (numpy's float32 power where alpha is neither 0 nor 1)"""
    with np.errstate(all="ignore"):
        v = (np.abs(np.asarray(abs_td, dtype=f32)) + f32(eps)).astype(f32)
        if alpha == 0:
            v = np.ones_like(v)
        elif alpha != 1:
            v = np.power(v, f32(alpha)).astype(f32)
        x = ((v * f32(65536)).astype(f32) + f32(0.5)).astype(f32)
        q = np.where(x < f32(Q_MAX), np.where(x >= 1, np.floor(x), 1), Q_MAX)
    return np.where(np.isnan(x), Q_MAX, q).astype(np.int64)


def quantise64(abs_td, alpha, eps):
    """the same in float64 (what the GPU's q is held against)"""
    with np.errstate(all="ignore"):
        v = np.abs(np.asarray(abs_td, dtype=np.float64)) + float(f32(eps))
        v = np.ones_like(v) if alpha == 0 else v if alpha == 1 else np.power(v, float(f32(alpha)))
        x = v * 65536.0 + 0.5
        q = np.where(x < Q_MAX, np.where(x >= 1, np.floor(x), 1), Q_MAX)
    return np.where(np.isnan(x), Q_MAX, q).astype(np.int64)


def level_sizes(NE):
    """[n_1, .., n_L]: nodes of the levels of sums above NE leaves"""
    out, n = [], NE
    while True:
        n = (n + FAN - 1) // FAN
        out.append(n)
        if n == 1:
            return out


def store_bytes(NE):
    return (((NE + 1) * 4 + 7) & ~7) + 8 * sum(level_sizes(NE))


def parse_store(raw, NE):
    """(leaves int64 [NE], maxq, [level arrays as Python-int lists]) of a store's bytes (a uint8 numpy array of store_bytes(NE))"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    assert raw.size == store_bytes(NE)
    leaves = raw[:4 * NE].view(np.uint32).astype(np.int64)
    maxq = int(raw[4 * NE:4 * NE + 4].view(np.uint32)[0])
    off, levels = ((NE + 1) * 4 + 7) & ~7, []
    for n in level_sizes(NE):
        levels.append([int(v) for v in raw[off:off + 8 * n].view(np.uint64)])
        off += 8 * n
    return leaves, maxq, levels


def level_sums(leaves):
    """the levels of exact sums above `leaves`, as lists of Python ints"""
    cur, out = [int(v) for v in leaves], []
    while True:
        cur = [sum(cur[i:i + FAN]) for i in range(0, len(cur), FAN)]
        out.append(cur)
        if len(cur) == 1:
            return out


def draw_targets(seed, update, B, total):
    """targets [B] (Python ints) of ocrl_per_sample's draw"""
    x, y = _bits(seed, SITE_PER, update & _M32, np.arange(B, dtype=np.uint64))
    return [(((int(a) << 32) | int(b)) * int(total)) >> 64 for a, b in zip(x, y)]


def search(leaves, targets):
    """idx [B]: the smallest i with leaves[0] + .. + leaves[i] > target (targets clamped to total - 1)"""
    prefix = np.cumsum(np.asarray(leaves, dtype=np.int64))
    total = int(prefix[-1])
    assert total > 0
    return np.searchsorted(prefix, np.minimum(np.asarray(targets, dtype=np.uint64), np.uint64(total - 1)).astype(np.int64), side="right").astype(np.int64)


def weights_rule(q, beta, dtype=f32):
    """(q_min / q)^beta of a batch's leaves q in `dtype` (float32: the header's order; float64: what the GPU is held against)"""
    q = np.asarray(q, dtype=f32).astype(dtype)
    ratio = (q.min() / q).astype(dtype)
    if beta == 0:
        return np.ones_like(ratio)
    return ratio if beta == 1 else np.power(ratio, dtype(f32(beta))).astype(dtype)
